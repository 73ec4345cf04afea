"""Inverse dynamics, host side: the fp64 yardstick tests/inverse_ref.py pinned on the fp64 oracle's forward
dynamics, the inputs of the device test kept inside the checker's boundary cap, and the public surface
(mjw.inverse, Data.qfrc_inverse, the mjw_inverse entry point).  The kernels are tested in tests/test_gpu_inverse.py.
"""

import numpy as np
import pytest

from tests import inverse_ref as ir
from tests import solver_cases as sc
from tests.common import humanoid_model, oracle_from_state, random_states

TOL64 = 1e-8  # absolute; two orders of magnitude over the fp64 solver's stop tolerance (measured 1.6e-10 worst)
NEWTON = [c for c in sc.CASES if c.solver == "Newton"]
GPU_CASES = ir.gpu_cases()


def _world(od, w, nv, qacc=None):
  a = sc.oracle_world(od, w, nv)
  a.update(qfrc_bias=od.qfrc_bias[w], qfrc_passive=od.qfrc_passive[w])
  if qacc is not None:
    a["qacc"] = qacc
  return a


def _check_forward_consistency(od, nv, njmax):
  od.forward()
  worst = dict(inverse=0.0, force=0.0, qfrc=0.0)
  for w in range(od.nworld):
    out = ir.inverse_world(_world(od, w, nv), njmax)
    n = out["n"]
    worst["inverse"] = max(worst["inverse"], np.abs(out["qfrc_inverse"] - (od.qfrc_applied[w] + od.qfrc_actuator[w])).max())
    worst["qfrc"] = max(worst["qfrc"], np.abs(out["qfrc_constraint"] - od.qfrc_constraint[w]).max())
    if n:
      worst["force"] = max(worst["force"], np.abs(out["force"] - od.efc_force[w, :n]).max())
      assert (out["state"] == od.efc_state[w, :n]).all()
  print("inverse_ref against the fp64 oracle:", worst)
  assert max(worst.values()) <= TOL64, worst


@pytest.mark.parametrize("lower", [0.0, 0.25], ids=["as-is", "root-lowered"])
def test_restatement_matches_oracle_forward_on_the_humanoid(lower):
  mjm = humanoid_model("NEWTON")
  qpos, qvel, ctrl = random_states(mjm, 16, seed=5, qpos_noise=0.1)
  qpos[:, 2] -= lower
  _, od = oracle_from_state(mjm, qpos, qvel, ctrl, njmax=128, nconmax=64)
  od.qfrc_applied[:] = np.random.default_rng(11).normal(0, 1.0, od.qfrc_applied.shape)
  _check_forward_consistency(od, mjm.nv, 128)
  if lower:
    assert od.nefc.max() > 64 > od.nefc.min()  # the row counts cross 64


@pytest.mark.parametrize("case", NEWTON, ids=[c.id for c in NEWTON])
def test_restatement_matches_oracle_forward_on_the_ladder(case):
  mjm = case.model()
  od = case.oracle(mjm, case.states(mjm), 64)
  od.qfrc_applied[:] = np.random.default_rng(case.seed + 3).normal(0, 0.5, od.qfrc_applied.shape)
  _check_forward_consistency(od, mjm.nv, case.njmax)


@pytest.mark.parametrize("case", GPU_CASES, ids=[c.id for c in GPU_CASES])
def test_device_inputs_stay_inside_the_boundary_cap(case):
  """At the perturbed acceleration the device test uses, on both oracle builds: few rows near a branch point,
  and every row state present (cases with friction-loss rows and more than 20 rows)."""
  mjm = case.model()
  states = case.states(mjm)
  for bits in (64, 32):
    od = case.oracle(mjm, states, bits)
    od.forward()
    qacc = ir.perturb_qacc(od.qacc, case.seed + 7)
    rows = boundary = 0
    seen = set()
    for w in range(od.nworld):
      a = _world(od, w, mjm.nv, qacc[w])
      out = ir.inverse_world(a, case.njmax)
      n = out["n"]
      a.update(force=np.concatenate([out["force"], np.zeros(case.njmax - n)]), state=np.concatenate([out["state"], np.zeros(case.njmax - n, int)]),
               qfrc_constraint=out["qfrc_constraint"], Ma=out["Ma"])
      inv = sc.world_invariants(a, case.njmax)
      assert inv["state_bad"] == 0 and max(inv[k] for k in sc.VALUES) <= 1e-12  # the checker and the yardstick agree
      rows += n
      boundary += inv["boundary"]
      seen |= set(out["state"].tolist())
    share = boundary / max(rows, 1)
    print(case.id, bits, "boundary share", share)
    assert share <= sc.BOUNDARY_CAP, (bits, share)
    if not case.bare and min(max(case.targets), case.njmax) > 20:
      assert seen == {0, 1, 2, 3}, (bits, seen)


def test_gpu_cases_span_the_dispatch_edges():
  assert sorted(c.num for c in GPU_CASES) == list(range(1, 14))
  assert {3 * c.nfeet + c.nhinge for c in GPU_CASES} == {16, 17, 28, 29, 32, 33}
  assert {c.njmax for c in GPU_CASES} == {20, 64, 96}
  assert [c.jacobian for c in GPU_CASES if c.num == 13] == ["sparse"]


def test_cone_law_zones():
  D, fr, mu = np.array([2.0, 1.0, 1.0]), np.array([0.5, 0.5, 0.0, 0.0, 0.0]), 0.5
  f, st, zone = ir.cone_law(np.array([1.0, 0.1, 0.0]), D, mu, fr)  # N = 0.5 >= mu T = 0.025
  assert zone == "top" and st == ir.SATISFIED and not f.any()
  f, st, zone = ir.cone_law(np.array([-1.0, 0.1, 0.0]), D, mu, fr)  # mu N + T = -0.25 + 0.05 <= 0
  assert zone == "bottom" and st == ir.QUADRATIC
  np.testing.assert_allclose(f, [2.0, -0.1, 0.0])
  jar = np.array([0.0, 1.0, 0.0])  # N = 0, T = 0.5: the cone's surface
  f, st, zone = ir.cone_law(jar, D, mu, fr)
  assert zone == "middle" and st == ir.CONE
  dm = D[0] / (mu * mu * (1 + mu * mu))
  np.testing.assert_allclose(f, [dm * mu * 0.5 * mu, -dm * mu * 0.5 * mu / 0.5 * 0.5 * 0.5, 0.0])
  assert f[0] > 0 and f[1] < 0  # pushes out along the normal and against the sliding direction


def test_discrete_acc_restatement():
  rng = np.random.default_rng(0)
  A = rng.normal(size=(4, 4))
  M = A @ A.T + 4 * np.eye(4)
  q = rng.normal(size=4)
  np.testing.assert_array_equal(ir.discrete_acc(M, q, 0.01, "Euler", eulerdamp=False), q)
  damp = np.array([0.1, 0.2, 0.0, 0.3])
  got = ir.discrete_acc(M, q, 0.01, "Euler", dof_damping=damp)
  np.testing.assert_allclose(M @ got, M @ q + 0.01 * damp * q, atol=1e-12)
  got = ir.discrete_acc(M, q, 0.01, "implicitfast", qDeriv=-np.diag(damp))
  np.testing.assert_allclose(M @ got, M @ q + 0.01 * damp * q, atol=1e-12)


# ---- surface ----------------------------------------------------------------------------------------
def _small():
  import mujoco_warp_amd as mjw

  case = sc.CASES[0]
  mjm = case.model()
  m = mjw.put_model(mjm, device="cpu")
  d = mjw.make_data(mjm, nworld=3, njmax=case.njmax, nconmax=case.nconmax, device="cpu", m=m)
  return mjw, mjm, m, d


def test_inverse_is_exported_and_data_has_qfrc_inverse():
  import torch

  mjw, mjm, m, d = _small()
  assert callable(mjw.inverse)
  assert tuple(d.qfrc_inverse.shape) == (3, mjm.nv) and d.qfrc_inverse.dtype == torch.float32
  assert not d.qfrc_inverse.any()
  d.qfrc_inverse.fill_(2.0)
  mjw.reset_data(m, d, torch.tensor([True, False, True]))
  assert d.qfrc_inverse[:, 0].tolist() == [0.0, 2.0, 0.0]
  mjw.reset_data(m, d)
  assert not d.qfrc_inverse.any()
  from mujoco_warp_amd import _lib

  assert _lib.ABI_VERSION == 36 and "qfrc_inverse" in [n for n, _ in _lib.DATA_REAL_ARRAYS]


def test_put_data_and_get_data_into_carry_qfrc_inverse():
  import types as pytypes

  import mujoco_warp_amd as mjw

  _, mjm, m, _ = _small()
  mjd = mjw.MjData(mjm)
  mjd.qfrc_inverse = np.arange(mjm.nv, dtype=np.float64)
  d = mjw.put_data(mjm, mjd, nworld=2, device="cpu", m=m)
  np.testing.assert_array_equal(d.qfrc_inverse.numpy(), np.tile(np.arange(mjm.nv, dtype=np.float32), (2, 1)))
  dst = pytypes.SimpleNamespace(qfrc_inverse=np.zeros(mjm.nv))
  mjw.get_data_into(dst, mjm, d, 1)
  np.testing.assert_array_equal(dst.qfrc_inverse, np.arange(mjm.nv))


def test_mjw_inverse_reports_null_arguments_and_takes_no_worlds_as_a_noop():
  """Null pointers come back through mjw_last_error; nworld == 0 returns 0 before any launch (no GPU here)."""
  from mujoco_warp_amd import _lib
  from mujoco_warp_amd.io import cdata, cmodel

  _, _, m, d = _small()
  L = _lib.lib()
  assert L.mjw_inverse(None, cdata(d), None) != 0
  assert b"mjw_inverse" in L.mjw_last_error() and b"null" in L.mjw_last_error()
  assert L.mjw_inverse(cmodel(m), None, None) != 0
  assert b"null" in L.mjw_last_error()
  empty = _lib.CData()  # nworld = 0, every pointer null
  assert L.mjw_inverse(cmodel(m), empty, None) == 0
  some = _lib.CData()
  some.nworld, some.njmax = 2, 8  # worlds, but no arrays
  assert L.mjw_inverse(cmodel(m), some, None) == -1
  assert b"null" in L.mjw_last_error()


def test_rk4_with_invdiscrete_raises_before_any_launch():
  from mujoco_warp_amd.inverse import discrete_acc

  mjw, mjm, _, _ = _small()
  mjm.opt.integrator = int(mjw.IntegratorType.RK4)
  mjm.opt.enableflags |= int(mjw.EnableBit.INVDISCRETE)
  m = mjw.put_model(mjm, device="cpu")
  d = mjw.make_data(mjm, nworld=1, device="cpu", m=m)
  # a launch on this host-only Data would raise RuntimeError instead
  with pytest.raises(NotImplementedError):
    mjw.inverse(m, d)
  with pytest.raises(NotImplementedError):
    discrete_acc(m, d, d.qacc.clone())
