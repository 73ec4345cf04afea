"""CPU validation of the row-count ladder and the solver-output invariants (tests/solver_cases.py) on the
oracle: the ladder hits every target of every case, the invariants hold on the fp64 build at 1e-12 and on the
fp32 build at 1e-5 without a state mismatch or a boundary row, and a corrupted copy of an oracle output is
flagged by the invariant that covers it."""

import numpy as np
import pytest

from tests import solver_cases as sc

IDS = [c.id for c in sc.CASES]


@pytest.fixture(scope="module")
def runs():
  """case id -> (mjm, {real_bits: OracleData after forward}), efc_force pre-filled with the NaN sentinel."""
  cache = {}

  def get(case):
    if case.id not in cache:
      mjm = case.model()
      states = case.states(mjm)
      ods = {}
      for bits in (64, 32):
        od = case.oracle(mjm, states, bits)
        od.efc_force[:] = np.nan
        od.forward()
        ods[bits] = od
      cache[case.id] = (mjm, ods)
    return cache[case.id]

  return get


@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_ladder_hits_every_target(runs, case):
  mjm, ods = runs(case)
  od = ods[64]
  assert mjm.nv == 3 * case.nfeet + case.nhinge
  ne, nf = (0, 0) if case.bare else (1, 2)
  assert od.nefc[:, 0].tolist() == list(case.targets)
  assert (od.ne[:, 0] == ne).all() and (od.nf[:, 0] == nf).all()
  rest = np.array(case.targets) - ne - nf
  ncon = np.minimum(rest // 4, 4 * case.nfeet)
  assert od.ncon[:, 0].tolist() == ncon.tolist()
  assert od.nl[:, 0].tolist() == (rest - 4 * ncon).tolist()
  assert ods[32].nefc[:, 0].tolist() == list(case.targets)


def test_ladder_reaches_every_state():
  """Satisfied, quadratic, linear-negative and linear-positive rows all occur on the full ladder."""
  case = next(c for c in sc.CASES if c.num == 5)
  mjm = case.model()
  od = case.oracle(mjm, case.states(mjm))
  od.forward()
  seen = set()
  for w in range(od.nworld):
    seen |= set(od.efc_state[w, : int(od.nefc[w, 0])].tolist())
  assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_invariants_hold_on_the_oracle(runs, case):
  mjm, ods = runs(case)
  for bits, tol in ((64, 1e-12), (32, sc.TOL)):
    inv = sc.solver_invariants(sc.oracle_worlds(ods[bits], mjm.nv), case.njmax, sentinel=True)
    for k in sc.VALUES:
      assert inv[k] <= tol, (bits, k, inv[k])
    assert inv["state_bad"] == 0 and inv["nonfinite"] == 0 and inv["touched"] == 0 and inv["qfrc_abs"] == 0.0, (bits, inv)
    assert inv["boundary_share"] <= sc.BOUNDARY_CAP and inv["boundary"] == 0, (bits, inv["boundary"])
    assert inv["rows"] == sum(min(t, case.njmax) for t in case.targets)
  assert sc.cost_excess(ods[64], ods[32].qacc) <= sc.COST_TOL
  assert sc.cost_excess(ods[64], ods[64].qacc) == 0.0
  t32, t64, margin = sc.niter_margin(ods[32], ods[64])
  assert margin >= len(case.targets) and t32 > 0 and t64 > 0


@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_last_kept_row_carries_a_force(runs, case):
  """Row min(nefc, njmax) - 1 of every world has a non-zero force (and, where the Newton Hessian's last row pair
  is half empty, is quadratic): a kernel that drops it at a row-count edge changes qfrc_constraint, the cost and
  the Newton iteration count."""
  mjm, ods = runs(case)
  for od in ods.values():
    for w, t in enumerate(case.targets):
      n = min(t, case.njmax)
      if n and (case.num, t) not in sc.LAST_ROW_FREE:
        assert od.efc_force[w, n - 1] != 0.0, (t, n)
        if n > 3:  # past the equality / friction rows: a limit or contact row, quadratic when active
          assert od.efc_state[w, n - 1] == 1, (t, n)


def _worlds(runs, case, bits=64):
  mjm, ods = runs(case)
  return [{k: np.array(v, dtype=np.float64 if k != "state" else int) for k, v in a.items()} for a in sc.oracle_worlds(ods[bits], mjm.nv)]


CORRUPT = [c for c in sc.CASES if c.num in (1, 5, 9, 10, 11)]


@pytest.mark.parametrize("case", CORRUPT, ids=[c.id for c in CORRUPT])
def test_corrupted_outputs_are_flagged(runs, case):
  """Every single-entry corruption of an output, at every row that carries a force (above 1e-3 of the row's own
  scale D s; nearly all do), fails its invariant at the
  1e-4 cap of the bars: one force zeroed (force_row), one state flipped (state), one J'f term dropped (qfrc_dof).
  The world-normalised force and qfrc flag the rows near the world's largest only (test_world_norms_alone_miss_small_rows)."""
  worlds = _worlds(runs, case)
  checked = 0
  for a in worlds:
    n = min(int(a["nefc"]), case.njmax)
    for r in range(n):
      b = dict(a, state=a["state"].copy())
      b["state"][r] = (b["state"][r] + 1) % 4
      inv = sc.world_invariants(b, case.njmax)
      assert inv["state_bad"] == 1 and inv["force"] <= 1e-12
      s_r = np.abs(a["J"][r]) @ np.abs(a["qacc"]) + abs(a["aref"][r])
      if abs(a["force"][r]) <= 10 * sc.TOL_CAP * a["D"][r] * s_r:  # no force, or one at the rounding level of the row
        continue
      checked += 1
      b = dict(a, force=a["force"].copy())
      b["force"][r] = 0.0
      inv = sc.world_invariants(b, case.njmax)
      assert inv["force_row"] > sc.TOL_CAP and inv["state_bad"] == 0, (r, inv)
      b = dict(a, qfrc_constraint=a["qfrc_constraint"] - a["J"][r] * a["force"][r])
      inv = sc.world_invariants(b, case.njmax)
      assert inv["qfrc_dof"] > sc.TOL_CAP and inv["force_row"] <= 1e-12, (r, inv)
  assert checked > 0


def test_corrupted_ma_and_row_range_are_flagged(runs):
  case = next(c for c in sc.CASES if c.num == 10)
  a = _worlds(runs, case)[3]  # nefc 21 > njmax 20
  assert int(a["nefc"]) > case.njmax
  b = dict(a, Ma=a["Ma"].copy())
  b["Ma"][np.argmax(np.abs(b["Ma"]))] *= 1.001
  assert sc.world_invariants(b, case.njmax)["Ma"] > sc.TOL_CAP
  case = next(c for c in sc.CASES if c.num == 5)
  a = _worlds(runs, case)[2]  # nefc 8
  n = int(a["nefc"])
  assert sc.world_invariants(a, case.njmax, sentinel=True)["touched"] == 0
  b = dict(a, force=a["force"].copy())
  b["force"][n] = 0.0  # a store one row past the end
  assert sc.world_invariants(b, case.njmax, sentinel=True)["touched"] == 1
  b = dict(a, force=a["force"].copy())
  b["force"][n - 1] = np.nan  # the last row never stored
  inv = sc.world_invariants(b, case.njmax, sentinel=True)
  assert inv["nonfinite"] == 1 and inv["force"] > sc.TOL_CAP


def test_boundary_rows_may_match_either_side():
  """A one-sided row with jar within BAND * s of zero passes with either branch's force and state, as long as
  the two agree; a friction row likewise at +-fl / D."""
  M = np.eye(1)
  base = dict(M=M, J=np.array([[1.0], [1.0]]), D=np.array([2.0, 2.0]), aref=np.array([1.0 - 1e-6, 0.5]), fl=np.array([0.0, 0.0]), ne=0, nf=0,
              nefc=2, qacc=np.array([1.0]), Ma=np.array([1.0]))
  jar0 = 1e-6  # row 0 sits on the boundary (satisfied side), row 1 is satisfied
  for f0, s0, ok in ((0.0, 0, True), (-2.0 * jar0, 1, True), (0.0, 1, False), (-1.0, 1, False)):
    a = dict(base, force=np.array([f0, 0.0]), state=np.array([s0, 0]), qfrc_constraint=np.array([f0]))
    inv = sc.world_invariants(a, 2)
    assert inv["boundary"] == 1
    assert (inv["state_bad"] == 0 and inv["force"] <= 1e-12) == ok, (f0, s0, inv)
  fr = dict(base, nf=1, fl=np.array([0.3, 0.0]), aref=np.array([1.0 + 0.15 - 1e-6, 0.5]))  # jar = -rf + 1e-6
  for f0, s0, ok in ((-2.0 * (-0.15 + 1e-6), 1, True), (0.3, 2, True), (0.3, 1, False), (-0.3, 3, False)):
    a = dict(fr, force=np.array([f0, 0.0]), state=np.array([s0, 0]), qfrc_constraint=np.array([f0]))
    inv = sc.world_invariants(a, 2)
    assert inv["boundary"] == 1
    assert (inv["state_bad"] == 0 and inv["force"] <= 1e-12) == ok, (f0, s0, inv)


def test_expected_kernels_cover_the_dispatch_table():
  """The case list reaches every solve kernel and switch point the dispatch has (pure bookkeeping, no device)."""
  kinds = {(c.kernel, c.solver) for c in sc.CASES}
  for k in ("dense16", "dense28", "dense32", "generic", "sparse"):
    assert (k, "CG") in kinds and ((k, "Newton") in kinds)
  assert ("fused", "CG") in kinds
  nvs = {3 * c.nfeet + c.nhinge for c in sc.CASES}
  assert {16, 17, 28, 29, 32, 33} <= nvs
  assert all(len(c.targets) <= 16 for c in sc.CASES)
  names = ["mjw::mjw_kernel<79, false, false>", "mjw::dense_kernel<3, true, false, 28>", "mjw::dense_kernel<4, true, false, 28>"]
  assert sc.solve_kernels(names) == names[1:2]
  sc.check_kernels(next(c for c in sc.CASES if c.num == 5 and c.solver == "Newton"), names)
  with pytest.raises(AssertionError):
    sc.check_kernels(next(c for c in sc.CASES if c.num == 7 and c.solver == "Newton"), names)
  assert sc.solve_kernels(["mjw::sp::solve_kernel<0>", "mjw::sp::solve_kernel<2>", "mjw::sp::euler_kernel"]) == ["mjw::sp::solve_kernel<2>"]
  assert sc.solve_kernels(["mjw::mjw_kernel<63, false, false>"]) == ["mjw::mjw_kernel<63, false, false>"]


def test_world_norms_alone_miss_small_rows():
  """Why force_row / qfrc_dof exist: next to a stiff row, a zeroed force of a soft row (or its dropped J'f term on
  a dof of its own) stays under the 1e-4 cap in the world-normalised `force` / `qfrc`, and is far above it in the
  row's / dof's own scale."""
  a = dict(M=np.eye(2), J=np.array([[1.0, 0.0], [0.0, 1.0]]), D=np.array([1e6, 1.0]), aref=np.array([2.0, 2.0]), fl=np.zeros(2), ne=0, nf=0,
           nefc=2, qacc=np.array([1.0, 1.0]), Ma=np.array([1.0, 1.0]), force=np.array([1e6, 1.0]), state=np.array([1, 1]),
           qfrc_constraint=np.array([1e6, 1.0]))
  inv = sc.world_invariants(a, 2)
  assert max(inv[k] for k in sc.VALUES) <= 1e-12 and inv["state_bad"] == 0
  inv = sc.world_invariants(dict(a, force=np.array([1e6, 0.0]), qfrc_constraint=np.array([1e6, 0.0])), 2)
  assert inv["force"] < sc.TOL < sc.TOL_CAP < inv["force_row"], inv
  inv = sc.world_invariants(dict(a, qfrc_constraint=np.array([1e6, 0.0])), 2)
  assert inv["qfrc"] < sc.TOL < sc.TOL_CAP < inv["qfrc_dof"], inv
