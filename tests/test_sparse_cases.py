"""The sparse edge fixtures (tests/sparse_cases.py) on the CPU oracle: the zoo holds every tree path at the sizes named,
the pad models hit ntree / nv / nbody / njnt at 255 / 256 / 257 (ntree 513 too), the big-subtree models have the counts of
block-summed subtrees they are named after, the ladder states give their exact row counts, the column model's J-transpose
columns have exactly k entries, every tree of the lowered zoo carries a contact row, and on every case the fp32 build of the
oracle stays within half of every bar the device is held to (so the inputs leave the device headroom) with its boundary
rows under the cap.  The checker rejects small edits of a view.  No GPU."""

import copy

import numpy as np
import pytest

from tests import sparse_cases as sp

_CACHE = {}


def _case(case):
  """What the tests read of a case, computed once (the oracle runs themselves are dropped: nv reaches 1941)."""
  if case.id in _CACHE:
    return _CACHE[case.id]
  mjm = case.model()
  f = sp.fields(mjm)
  states = case.states(mjm)
  ref = sp.oracle_run(case, mjm, states, 64)
  v32 = sp.oracle_run(case, mjm, states, 32)
  od = ref["od"]
  nt = int(f["ntree"])
  out = dict(counts=f["counts"], values=sp.measure(case, mjm, f, v32, ref), self_values=sp.measure(case, mjm, f, ref, ref), nefc=ref["counts"]["nefc"],
             nefc32=v32["counts"]["nefc"], ne=ref["counts"]["ne"], paths=[(int(f["tree_dofadr"][t + 1] - f["tree_dofadr"][t]), sp.tree_path(f, t), sp.tree_branched(f, t))
                                                                          for t in range(nt)],
             big=sp.big_bodies(f), subtree=[int(e) - b for b, e in enumerate(f["body_subtree_end"])], xmax=float(np.abs(ref["fields"]["xipos"]).max()),
             states_equal=bool(np.array_equal(states[0][3], states[0][0]) and np.array_equal(states[1][3], states[1][0])),
             states_differ=bool(not np.array_equal(states[0][1], states[0][0]) or not np.array_equal(states[1][1], states[1][0])))
  if case.kind in ("columns", "contact"):
    starts = np.asarray(f["tree_dofadr"])
    cols, tree_rows, nnz = [], [], set()
    for w in range(4):
      n = int(od.nefc[w, 0])
      J = od.efc_J[w].reshape(case.njmax, mjm.nv)[:n]
      cols.append([int(c) for c in (J != 0).sum(axis=0)])
      tree_rows.append([int((J[:, starts[t]:starts[t + 1]] != 0).any(axis=1).sum()) for t in range(nt)])
      nnz |= {int(c) for c in (J != 0).sum(axis=1)}
    out.update(cols=cols, tree_rows=tree_rows, row_nnz=nnz)
  if case.id == "zoo":
    out["views"] = (mjm, f, ref)  # nv = 98: kept for the checker test
  _CACHE[case.id] = out
  return out


@pytest.mark.parametrize("case", sp.CASES, ids=[c.id for c in sp.CASES])
def test_fp32_oracle_leaves_headroom(case):
  c = _case(case)
  assert c["states_equal"] and c["states_differ"]  # world 3 repeats world 0, the others differ
  assert not sp.failures(c["self_values"], 1e-6)  # the fp64 oracle against itself: fp64 rounding only
  bad = sp.failures(c["values"], 0.5)
  assert not bad, bad
  assert c["values"]["boundary_share"] <= sp.sc.BOUNDARY_CAP
  assert c["nefc"] == c["nefc32"]
  if case.kind != "ladder":  # (solver_cases.ladder_xml spreads its feet to x = 38)
    assert c["xmax"] <= 2.0, c["xmax"]


def test_zoo_holds_every_path():
  c = _case(sp.CASES[0])
  assert sp.CASES[0].id == "zoo" and c["counts"] == dict(ntree=18, nv=98, nbody=73, njnt=72)
  have = set(c["paths"])
  for n in (1, 2, 3, 4):
    assert (n, "chain", False) in have
  assert (3, "small", True) in have and (4, "small", True) in have  # branched: never the chain path
  for n in (5, 6, 7):
    assert (n, "small", False) in have
  assert (8, "small", False) in have and (8, "small", True) in have
  assert (9, "general", False) in have and (9, "general", True) in have
  assert not [p for p in have if p[1] == "chain" and (p[0] > sp.CHAIN or p[2])]
  assert not [p for p in have if (p[1] == "general") != (p[0] > sp.TREE)]
  assert sorted(n for n, _, _ in c["paths"]) == sorted([1, 2, 3, 4, 5, 8, 9, 3, 4, 5, 6, 7, 8, 9, 3, 4, 8, 9])


def test_pads_hit_every_count():
  hit = {k: set() for k in sp.PAD_COUNTS}
  for case in sp.CASES:
    if case.kind not in ("zoo", "contact"):
      continue
    c = _case(case)
    assert [p[:2] for p in c["paths"][:18]] == [p[:2] for p in _case(sp.CASES[0])["paths"]]  # the zoo stays, first
    assert all(p == (1, "chain", False) for p in c["paths"][18:])
    if case.kind == "zoo":
      for k in hit:
        hit[k].add(c["counts"][k])
      for e in case.expect:
        k, v = e.split("=")
        assert c["counts"][k] == int(v)
  for k, want in sp.PAD_COUNTS.items():
    assert set(want) <= hit[k], (k, hit[k])
  # a one-dof tree is the last tree of a stride round (ntree 256) and the first of the next (257); the zoo's trees are the
  # first of round one in every model
  assert {256, 257, 513} <= hit["ntree"]
  assert {c["counts"]["nv"] for c in (_case(x) for x in sp.CASES if x.kind == "contact")} == {255, 256, 257}


BIG_EXPECT = {"big-nbig1": 1, "big-star64-65": 2, "big-nbig15": 15, "big-nbig16": 16, "big-nbig17": 17, "big-chains6": 37, "big-stars16-900": 18,
              "big-900-stars16": 18}


def test_big_subtrees():
  seen = set()
  for case in sp.CASES:
    if case.kind != "big":
      continue
    c = _case(case)
    assert len(c["big"]) == BIG_EXPECT[case.id] and c["big"][0] == 0, (case.id, c["big"])
    seen |= set(c["subtree"][1:])
  assert set(BIG_EXPECT) == {c.id for c in sp.CASES if c.kind == "big"}
  assert {sp.BIG, sp.BIG + 1, 901} <= seen
  c = _case(next(x for x in sp.CASES if x.id == "big-star64-65"))
  assert c["subtree"][1] == 64 and c["subtree"][65] == 65 and c["big"] == [0, 65]
  c = _case(next(x for x in sp.CASES if x.id == "big-chains6"))
  assert c["counts"]["nbody"] == 421 and [b for b in c["big"] if c["subtree"][b] == 70] == [1, 71, 141, 211, 281, 351]
  assert {b // 64 % 4 for b in c["big"][1:]} == {0, 1, 2, 3} and {b // sp.BLK for b in c["big"][1:]} == {0, 1}  # every wave, both rounds
  last = _case(next(x for x in sp.CASES if x.id == "big-stars16-900"))
  first = _case(next(x for x in sp.CASES if x.id == "big-900-stars16"))
  assert last["subtree"][last["big"][-1]] == 901 and first["subtree"][first["big"][1]] == 901


@pytest.mark.parametrize("case", [c for c in sp.CASES if c.kind == "ladder"], ids=[c.id for c in sp.CASES if c.kind == "ladder"])
def test_ladder_rows(case):
  c = _case(case)
  assert c["nefc"] == [case.target] * 4 and c["ne"] == [1] * 4
  assert case.njmax == case.target or case.njmax > max(sp.LADDER_TARGETS)


def test_ladder_and_columns_cases_are_all_present():
  ids = {c.id for c in sp.CASES}
  for s in ("CG", "Newton"):
    assert f"columns-{s}" in ids
    for t in (255, 256, 257, 1023, 1024, 1025):
      assert f"ladder-{t}-njmax{t}-{s}" in ids and f"ladder-{t}-njmax1040-{s}" in ids
    for integ in ("Euler", "implicitfast"):
      for nv in (255, 256, 257):
        assert f"contact-nv{nv}-{s}-{integ}" in ids
  assert sp.BLK * sp.RU == 1024


@pytest.mark.parametrize("solver", ["CG", "Newton"])
def test_column_lengths(solver):
  c = _case(next(x for x in sp.CASES if x.id == f"columns-{solver}"))
  assert sp.COLUMN_K == (1, 3, 4, 5, 31, 32, 33, 64) and sp.SORTN == 32
  for w in range(4):
    assert c["cols"][w] == list(sp.COLUMN_K) + [0]  # the body left up: an empty column
  assert c["nefc"] == [sum(sp.COLUMN_K)] * 4


@pytest.mark.parametrize("case", [c for c in sp.CASES if c.kind == "contact"], ids=[c.id for c in sp.CASES if c.kind == "contact"])
def test_every_zoo_tree_carries_a_contact_row(case):
  c = _case(case)
  for w in range(4):
    assert all(n >= 1 for n in c["tree_rows"][w][:18]), c["tree_rows"][w][:18]
  assert set(range(1, 10)) <= c["row_nnz"], c["row_nnz"]


def test_checker_rejects_edits():
  mjm, f, ref = _case(sp.CASES[0])["views"]
  case = sp.CASES[0]

  def bad(fn):
    v = copy.deepcopy({k: x for k, x in ref.items() if k != "od"})
    v["od"] = ref["od"]
    fn(v)
    return {b[0] for b in sp.failures(sp.measure(case, mjm, f, v, ref))}

  assert bad(lambda v: None) == set()
  # the one-dof hinge tree's body is body 1: its entries are far below the heaviest tree's
  assert "subtree_com_tree" in bad(lambda v: v["fields"]["subtree_com"].__setitem__((0, slice(3, 6)), v["fields"]["subtree_com"][0, 3:6] * (1 + 1e-4)))
  assert "cinert_tree" in bad(lambda v: v["fields"]["cinert"].__setitem__((1, 19), v["fields"]["cinert"][1, 19] * (1 + 1e-4)))
  assert "qM_tree" in bad(lambda v: v["qM"][2].__setitem__((1, 2), v["qM"][2][1, 2] * (1 + 1e-4)))
  assert "solve_trees_backward" in bad(lambda v: v["qacc_smooth"].__setitem__((0, slice(89, 98)), v["qacc_smooth"][0, 89:98] * (1 + 1e-4)))
  assert "mul_m_trees" in bad(lambda v: v["Ma"].__setitem__((3, 0), v["Ma"][3, 0] * (1 + 1e-4)))
  assert "step3_qpos" in bad(lambda v: v["step3"][0].__setitem__((1, 5), v["step3"][0][1, 5] + 1e-4))
  assert "xpos" in bad(lambda v: v["fields"]["xpos"].__setitem__((0, 4), v["fields"]["xpos"][0, 4] + 1e-4))
  # L' D L rebuilt from a sparse qLD: the oracle's dense factor is not in that layout, so build one from qM
  M = ref["qM"][0]
  t = 6  # the chain of nine hinges
  a, e = int(f["tree_dofadr"][t]), int(f["tree_dofadr"][t + 1])
  qLD = np.zeros(int(mjm.M_rowadr[-1] + mjm.M_rownnz[-1]))
  A = M[a:e, a:e].copy()
  n = e - a
  L, D = np.eye(n), np.zeros(n)
  for k in range(n - 1, -1, -1):  # M = L' D L, from the last dof up
    D[k] = A[k, k]
    L[k, :k] = A[k, :k] / D[k]
    A[:k, :k] -= D[k] * np.outer(L[k, :k], L[k, :k])
  for k in range(a, e):
    adr, nnz = int(mjm.M_rowadr[k]), int(mjm.M_rownnz[k])
    qLD[adr + nnz - 1] = D[k - a]
    for p in range(nnz - 1):
      qLD[adr + p] = L[k - a, int(mjm.M_colind[adr + p]) - a]
  assert np.abs(sp.rebuild_LDL(mjm, f, qLD, t) - M[a:e, a:e]).max() <= 1e-12 * np.abs(M[a:e, a:e]).max()
