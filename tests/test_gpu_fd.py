"""Finite-difference linearisation on the device: the two kernels of csrc/mjw_fd.hip each on their own against
tests/fd_ref.py, transition_fd end to end against a closed form on both Jacobian paths, and the humanoid in ground
contact (finite, `d` untouched, nothing allocated).  Host-side checks are in tests/test_fd.py.
"""

import numpy as np
import pytest

from tests import fd_ref as fr

pytestmark = pytest.mark.gpu

EPS = 2.0**-7
NWORLD = 3
STATE = ("qpos", "qvel", "act", "ctrl")
COPIED = ("time", "qpos", "qvel", "act", "ctrl", "qacc_warmstart", "qfrc_applied", "xfrc_applied", "eq_active", "mocap_pos", "mocap_quat")
# (centered, max_worlds): one pass, and passes of 2 (4) columns with a remainder pass of one column
CONFIGS = [(True, None), (False, None), (True, 3 * 5), (False, 3 * 5)]
IDS = ["centred", "forward", "centred-passes", "forward-passes"]


def _unit(rng, shape):
  q = rng.normal(size=shape + (4,))
  return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _bits(a):
  return np.ascontiguousarray(a).view(np.int32)


def _host(t):
  return t.detach().cpu().numpy()


def _small(centered, max_worlds, seed=0):
  """FD_SMALL on the device: three worlds at a random state with unit quaternions, the motor's ctrl at 0, 1, -1."""
  import torch

  import mujoco_warp_amd as mjw

  mjm = mjw.load_model_from_string(fr.FD_SMALL)
  m = mjw.put_model(mjm, device="cuda")
  d = mjw.make_data(mjm, nworld=NWORLD, device="cuda", m=m)
  rng = np.random.default_rng(seed)
  qpos = rng.normal(0, 0.5, (NWORLD, mjm.nq))
  qpos[:, 3:7] = _unit(rng, (NWORLD,))
  qpos[:, 7:11] = _unit(rng, (NWORLD,))
  ctrl = rng.uniform(-0.5, 0.5, (NWORLD, mjm.nu))
  ctrl[:, 0] = fr.FD_SMALL_CTRL0
  vals = dict(time=rng.uniform(0, 2, NWORLD), qpos=qpos, qvel=rng.normal(0, 0.5, (NWORLD, mjm.nv)), act=rng.normal(0, 0.3, (NWORLD, mjm.na)),
              ctrl=ctrl, qacc_warmstart=rng.normal(size=(NWORLD, mjm.nv)), qfrc_applied=rng.normal(0, 0.1, (NWORLD, mjm.nv)),
              xfrc_applied=rng.normal(0, 0.1, (NWORLD, mjm.nbody, 6)), mocap_pos=rng.normal(size=(NWORLD, 1, 3)), mocap_quat=_unit(rng, (NWORLD, 1)))
  for n, v in vals.items():
    getattr(d, n)[:] = torch.as_tensor(v, dtype=torch.float32, device="cuda")
  d.qfrc_applied[0, 0] = -0.0  # a bit pattern that only a bitwise copy keeps
  d.eq_active[:] = torch.tensor([[1], [0], [1]], dtype=torch.int32, device="cuda")
  ctx = mjw.make_fd_context(mjm, m, NWORLD, centered=centered, max_worlds=max_worlds)
  return mjw, mjm, m, d, ctx


# ---- 3: fd_perturb alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("centered,max_worlds", CONFIGS, ids=IDS)
def test_fd_perturb_fills_every_slot(centered, max_worlds):
  import torch

  mjw, mjm, m, d, ctx = _small(centered, max_worlds)
  assert ctx.npass == (1 if max_worlds is None else (13 if centered else 7))
  before = {n: _host(getattr(d, n)).copy() for n in COPIED}
  ndx, seen, worst = 23, set(), 0.0
  for p in range(ctx.npass):
    for n in COPIED:  # what an earlier pass or a step left must not survive
      getattr(ctx.data, n).fill_(7)
    mjw.fd_perturb(m, d, ctx, EPS, pass_index=p)
    torch.cuda.synchronize()
    got = {n: _host(getattr(ctx.data, n)) for n in COPIED}
    smap = ctx.slot_map(p)
    assert np.array_equal(smap, fr.slot_map(25, ctx.ncp, centered, p))
    for c, (col, sign) in enumerate(smap):
      for w in range(NWORLD):
        sw = c * NWORLD + w
        for n in COPIED:
          if n not in STATE:
            assert np.array_equal(_bits(got[n][sw]), _bits(before[n][w])), (n, p, c, w)
        nominal = {n: before[n][w] for n in STATE}
        want = fr.slot_state(mjm, nominal, int(col), int(sign), EPS, centered)
        quat = set()
        if 0 <= col < mjm.nv:
          isq, adr, _ = fr.dof_target(mjm, int(col))
          quat = set(range(adr, adr + 4)) if isq else set()
        changed = 0
        for n in STATE:
          for i in range(nominal[n].size):
            g, x = got[n][sw, i], want[n][i]
            if n == "qpos" and i in quat:
              worst = max(worst, abs(float(g) - x))
              assert abs(float(g) - x) <= 2.0**-20, (p, c, w, i, g, x)
              changed += 1
            else:  # untouched: the world's bits; nudged: float32(x +- eps)
              assert _bits(np.float32(g)) == _bits(np.float32(x)), (n, p, c, w, i, g, x)
              changed += int(np.float32(x) != nominal[n][i])
        if col < 0:
          assert changed == 0
        elif col >= ndx and c > 0:  # ctrl under the range rule
          plus, minus = fr.ctrl_nudges(mjm, nominal["ctrl"], int(col) - ndx, EPS, centered)
          made = (plus or minus) if not centered else (plus if sign > 0 else minus)
          assert changed == int(made), (p, c, w, plus, minus)
          seen.add((int(col), w, plus, minus))
        else:
          assert changed == (4 if quat else 1), (p, c, w, changed)
  print("fd_perturb: worst quaternion entry error", worst, "bound", 2.0**-20)
  # the three worlds took the three branches of the motor's column, the other actuator is free
  want = {(23, 0, True, centered), (23, 1, False, True), (23, 2, True, False)} | {(24, w, True, centered) for w in range(NWORLD)}
  assert seen == want
  for n in COPIED:  # d is only read
    assert np.array_equal(_bits(_host(getattr(d, n))), _bits(before[n])), n


# ---- 4: fd_difference alone ------------------------------------------------------------------------------------
def _guarded(torch, shape):
  """A NaN-filled (nworld, r, c) output between two guard blocks of the same allocation."""
  big = torch.full((shape[0] + 2,) + tuple(shape[1:]), float("nan"), dtype=torch.float32, device="cuda")
  return big, big[1:-1]


@pytest.mark.parametrize("centered,max_worlds", CONFIGS, ids=IDS)
def test_fd_difference_transposes_the_slots(centered, max_worlds):
  import torch

  mjw, mjm, m, d, ctx = _small(centered, max_worlds, seed=1)
  ndx, nu, ns, K = 23, 2, 7, 25
  bigs, outs = zip(*[_guarded(torch, s) for s in ((NWORLD, ndx, ndx), (NWORLD, ndx, nu), (NWORLD, ns, ndx), (NWORLD, ns, nu))])
  A, B, C, D = outs
  ctrl = _host(d.ctrl)
  h32 = {1: np.float32(EPS), 2: np.float32(2 * EPS)}
  rng = np.random.default_rng(2)
  nsw = ctx.data.nworld
  quat_rows = [v for v in range(mjm.nv) if fr.dof_target(mjm, v)[0]]
  assert quat_rows == [3, 4, 5, 6, 7, 8]
  worst_q = worst_ulp = 0.0
  branches = set()
  for p in range(ctx.npass):
    # random next states and sensordata written by the test itself: no step, so no step's sensitivity
    qpos = rng.normal(0, 0.5, (nsw, mjm.nq))
    qpos[:, 3:7] = _unit(rng, (nsw,))
    qpos[:, 7:11] = _unit(rng, (nsw,))
    y = dict(qpos=qpos, qvel=rng.normal(0, 0.5, (nsw, mjm.nv)), act=rng.normal(0, 0.3, (nsw, mjm.na)), sensordata=rng.normal(size=(nsw, ns)))
    for n, v in y.items():
      getattr(ctx.data, n)[:] = torch.as_tensor(v, dtype=torch.float32, device="cuda")
    y = {n: _host(getattr(ctx.data, n)) for n in y}
    mjw.fd_difference(m, d, ctx, EPS, A, B, C, D, pass_index=p)
    torch.cuda.synchronize()
    M = np.concatenate([np.concatenate([_host(A), _host(B)], axis=2), np.concatenate([_host(C), _host(D)], axis=2)], axis=1)  # (w, ndx + ns, K)
    col0, ncols = ctx.pass_columns(p)
    for j in range(ncols):
      k = col0 + j
      for w in range(NWORLD):
        plan = ("-", "+", 2) if centered else ("0", "+", 1)
        if k >= ndx:
          plan = fr.column_plan(*fr.ctrl_nudges(mjm, ctrl[w], k - ndx, EPS, centered))
          branches.add((k, w, plan))
        got = M[w, :, k]
        if plan is None:
          assert np.array_equal(_bits(got), np.zeros(ndx + ns, dtype=np.int32)), (p, k, w)
          continue
        slot = {"0": 0, "+": 1 + j, "-": 1 + ctx.ncp + j if centered else 1 + j}
        y1, y2 = ({n: y[n][slot[s] * NWORLD + w] for n in y} for s in plan[:2])
        ref = fr.difference(mjm, y1, y2, plan[2] * EPS)
        h = h32[plan[2]]
        exact = np.concatenate([np.zeros(mjm.nv, dtype=np.float32)] + [(y2[n] - y1[n]) / h for n in ("qvel", "act", "sensordata")])
        for v in range(mjm.nv):
          isq, adr, _ = fr.dof_target(mjm, v)
          if not isq:
            exact[v] = (y2["qpos"][adr] - y1["qpos"][adr]) / h
        for r in range(ndx + ns):
          if r in quat_rows:
            worst_q = max(worst_q, abs(float(got[r]) - ref[r]) * float(h))
            assert abs(float(got[r]) - ref[r]) <= 2.0**-20 / float(h), (p, k, w, r, got[r], ref[r])
          else:
            ulp = float(np.spacing(np.abs(exact[r])))
            worst_ulp = max(worst_ulp, abs(float(got[r]) - float(exact[r])) / ulp)
            assert abs(float(got[r]) - float(exact[r])) <= ulp, (p, k, w, r, got[r], exact[r])
  print("fd_difference: worst quaternion row error * h", worst_q, "bound", 2.0**-20, "; worst other row, ulp", worst_ulp)
  for t in outs:  # every element written
    assert not torch.isnan(t).any()
  for big in bigs:  # nothing outside
    assert bool(torch.isnan(big[0]).all()) and bool(torch.isnan(big[-1]).all())
  one = ("0", "+", 1)
  want = {(23, 0, ("-", "+", 2) if centered else one), (23, 1, ("-", "0", 1)), (23, 2, one)} | {(24, w, ("-", "+", 2) if centered else one) for w in range(NWORLD)}
  assert branches == want


def test_fd_difference_without_sensors_leaves_c_and_d_alone():
  import torch

  mjw, mjm, m, d, ctx = _small(True, None, seed=3)
  A = torch.full((NWORLD, 23, 23), float("nan"), device="cuda")
  B = torch.full((NWORLD, 23, 2), float("nan"), device="cuda")
  mjw.fd_perturb(m, d, ctx, EPS)
  mjw.fd_difference(m, d, ctx, EPS, A, B)
  torch.cuda.synchronize()
  # the slots were not stepped: x' = x, so A is the identity up to the rounding of x +- eps (|x| < 4: 2^-22 each, two
  # per entry, over 2 eps; the quaternion rows 2^-20 over 2 eps) and B is zero: exactly in the scalar rows, within the
  # quaternion rows' bound in those (the log of a product that is the identity only up to rounding)
  bound = 2.0**-20 / (2 * EPS)
  err = np.abs(_host(A) - np.eye(23, dtype=np.float32)).max()
  gotB = _host(B)
  print("unstepped A - I:", err, "B:", np.abs(gotB).max(), "bound", bound)
  scalar = [r for r in range(23) if r not in (3, 4, 5, 6, 7, 8)]
  assert err <= bound and not gotB[:, scalar].any() and np.abs(gotB).max() <= bound


# ---- 5: end to end against the closed form, dense and sparse ---------------------------------------------------
@pytest.mark.parametrize("centered", [True, False], ids=["centred", "forward"])
@pytest.mark.parametrize("jacobian", ["dense", "sparse"])
def test_transition_fd_matches_the_slide_closed_form(jacobian, centered):
  import torch

  import mujoco_warp_amd as mjw

  mjm = mjw.load_model_from_string(fr.SLIDE_XML.format(jacobian=f' jacobian="{jacobian}"'))
  m = mjw.put_model(mjm, device="cuda")
  assert bool(m.is_sparse) == (jacobian == "sparse")
  d = mjw.make_data(mjm, nworld=NWORLD, device="cuda", m=m)
  x = np.array([[0.3, -0.2], [-0.7, 0.5], [0.0, 0.9]])
  u = np.array([[0.4], [-1.0], [0.25]])
  d.qpos[:] = torch.as_tensor(x[:, :1], dtype=torch.float32, device="cuda")
  d.qvel[:] = torch.as_tensor(x[:, 1:], dtype=torch.float32, device="cuda")
  d.ctrl[:] = torch.as_tensor(u, dtype=torch.float32, device="cuda")
  ctx = mjw.make_fd_context(mjm, m, NWORLD, centered=centered)
  A = torch.full((NWORLD, 2, 2), float("nan"), device="cuda")
  B = torch.full((NWORLD, 2, 1), float("nan"), device="cuda")
  C, D = torch.zeros((NWORLD, 0, 2), device="cuda"), torch.zeros((NWORLD, 0, 1), device="cuda")
  mjw.transition_fd(m, d, EPS, centered, A, B, C, D, ctx=ctx)
  torch.cuda.synchronize()
  Aw, Bw = fr.slide_closed_form()
  # the final rounding of each q', v' dominates: two per difference of 2^-24 max(1, |y|) / eps each; 4x for the
  # few roundings inside the 1-dof step
  ynext = np.abs(x @ Aw.T + u @ Bw.T).max()
  atol = 8 * 2.0**-24 * max(1.0, ynext) / EPS
  errA, errB = np.abs(_host(A) - Aw).max(), np.abs(_host(B) - Bw).max()
  print(f"transition_fd slide {jacobian} centered={centered}: errA {errA:.3e} errB {errB:.3e} atol {atol:.3e}")
  assert errA <= atol and errB <= atol


# ---- 6: the humanoid in ground contact -------------------------------------------------------------------------
def test_transition_fd_humanoid_in_contact_reads_d_and_allocates_nothing():
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import _lib
  from mujoco_warp_amd.io import _get_data_field
  from tests.common import gpu_from_state, humanoid_model, random_states

  mjm = humanoid_model("CG")
  qpos, qvel, ctrl = random_states(mjm, 2, seed=4, qvel_noise=0.1, ctrl_noise=0.2)  # around key 0, the squat
  m, d = gpu_from_state(mjm, qpos, qvel, ctrl)
  for _ in range(20):
    mjw.step(m, d)
  torch.cuda.synchronize()
  assert int(d.nefc.min()) > 0 and int(d.nacon[0]) > 0  # standing on the floor
  ndx, nu, ns = 2 * mjm.nv + mjm.na, mjm.nu, mjm.nsensordata
  assert (mjm.nv, mjm.na, mjm.nu) == (27, 0, 21)
  ctx = mjw.make_fd_context(mjm, m, 2, nconmax=24, njmax=64)
  assert ctx.data.nworld == 2 * 151
  A, B = torch.empty((2, ndx, ndx), device="cuda"), torch.empty((2, ndx, nu), device="cuda")
  C, D = torch.empty((2, ns, ndx), device="cuda"), torch.empty((2, ns, nu), device="cuda")
  names = [n for n, _ in _lib.DATA_REAL_ARRAYS + _lib.DATA_INT_ARRAYS + _lib.CONTACT_REAL_ARRAYS + _lib.CONTACT_INT_ARRAYS]
  fields = {n: _get_data_field(d, n) for n in names}
  fields.update(nacon=d.nacon, ncollision=d.ncollision, nisland=d.nisland, tree_island=d.tree_island, dof_island=d.dof_island, efc_island=d.efc_island)
  before = {n: t.clone() for n, t in fields.items()}
  torch.cuda.synchronize()
  mem = torch.cuda.memory_allocated()
  mjw.transition_fd(m, d, 2.0**-9, True, A, B, C, D, ctx=ctx)
  torch.cuda.synchronize()
  assert torch.cuda.memory_allocated() == mem
  for t in (A, B, C, D):
    assert bool(torch.isfinite(t).all())
  for n, t in fields.items():
    assert torch.equal(t.view(torch.int32), before[n].view(torch.int32)), n
  assert float(A.abs().max()) > 0 and float(B.abs().max()) > 0
