"""Inverse dynamics on the device (mjw.inverse: csrc/mjw_inverse.hip, sp::inverse_kernel in csrc/mjw_sparse.hip).

1. Every dispatch and row-count edge: the ladder cases of tests/solver_cases.CASES at a perturbed acceleration,
   checked with that module's invariants from the arrays on the device.
2. The reference's round trip (inverse_test.py): forward, then inverse, returns the applied forces; Euler and
   implicitfast x dense and sparse x INVDISCRETE off and on, at the reference's own tolerance.
3. Tendon armature with gravity and constraints disabled.
4. Elliptic cones against tests/inverse_ref.cone_law, dense and sparse, one contact cut by njmax.
5. A grid of more than one block's worth of worlds (humanoid, 257 worlds) and the acceleration sensors (apollo).
"""

import os

import numpy as np
import pytest

from tests import inverse_ref as ir
from tests import solver_cases as sc
from tests.common import ROOT, dense_efc_J, gpu_from_state, humanoid_model, np_, random_states

pytestmark = pytest.mark.gpu

GPU_CASES = ir.gpu_cases()
RT_TOL = 5e-3  # atol = rtol of the reference's inverse_test.py


def _bits(t):
  import torch

  return t.view(torch.int32).clone() if t.dtype == torch.float32 else t.clone()


def _dense_M(mjm, m, d, w):
  if m.is_sparse:
    from tests.cloth_common import dense_qM

    return dense_qM(mjm, np_(d.qM[w]))
  return np_(d.qM[w])[: mjm.nv, : mjm.nv]


def _worlds(mjm, m, d):
  """Per-world arrays of the device in the layout of solver_cases.world_invariants / inverse_ref.inverse_world."""
  out = []
  for w in range(d.nworld):
    n = min(int(d.nefc[w]), d.njmax)
    J = np.zeros((d.njmax, mjm.nv))
    J[:n] = dense_efc_J(m, d, w)
    out.append(dict(M=_dense_M(mjm, m, d, w), J=J, D=np_(d.efc.D[w, : d.njmax]), aref=np_(d.efc.aref[w]), fl=np_(d.efc.frictionloss[w]),
                    ne=int(d.ne[w]), nf=int(d.nf[w]), nefc=int(d.nefc[w]), qacc=np_(d.qacc[w]), qfrc_constraint=np_(d.qfrc_constraint[w]),
                    Ma=np_(d.efc.Ma[w]), force=np_(d.efc.force[w]), state=d.efc.state[w, : d.njmax].cpu().numpy(), qfrc_bias=np_(d.qfrc_bias[w]),
                    qfrc_passive=np_(d.qfrc_passive[w]), qfrc_inverse=np_(d.qfrc_inverse[w])))
  return out


def _combine_excess(a):
  """Worst |qfrc_inverse - (bias + M qacc - passive - qfrc_constraint)| over its bar's scale
  |bias| + |M| |qacc| + |passive| + |qfrc_constraint|, per dof, in fp64 from the device's arrays."""
  want = a["qfrc_bias"] + a["M"] @ a["qacc"] - a["qfrc_passive"] - a["qfrc_constraint"]
  scale = np.abs(a["qfrc_bias"]) + np.abs(a["M"]) @ np.abs(a["qacc"]) + np.abs(a["qfrc_passive"]) + np.abs(a["qfrc_constraint"])
  return float((np.abs(a["qfrc_inverse"] - want) / np.maximum(scale, 1e-300)).max())


def _perturbed_inverse(mjm, states, njmax, nconmax, seed):
  """The procedure of the edge test: forward, qacc overwritten with the perturbed one, efc.force filled with NaN,
  the outputs zeroed, inverse.  Returns (m, d, the state's bits before the call)."""
  import torch

  import mujoco_warp_amd as mjw

  m, d = gpu_from_state(mjm, *states, njmax=njmax, nconmax=nconmax)
  mjw.forward(m, d)
  d.qacc[:] = torch.as_tensor(ir.perturb_qacc(np_(d.qacc), seed), device="cuda")
  d.efc.force.fill_(float("nan"))
  for t in (d.qfrc_constraint, d.qfrc_inverse, d.efc.Ma):
    t.zero_()
  before = {k: _bits(getattr(d, k)) for k in ("qacc", "qpos", "qvel", "time")}
  mjw.inverse(m, d)
  torch.cuda.synchronize()
  return m, d, before


def _assert_state_unchanged(d, before):
  import torch

  for k, v in before.items():
    assert torch.equal(_bits(getattr(d, k)), v), k


# ---- 1. every dispatch and row-count edge -------------------------------------------------------------
@pytest.mark.parametrize("case", GPU_CASES, ids=[c.id for c in GPU_CASES])
def test_inverse_at_every_dispatch_and_row_count_edge(case):
  mjm = case.model()
  m, d, before = _perturbed_inverse(mjm, case.states(mjm), case.njmax, case.nconmax, case.seed + 7)
  assert bool(m.is_sparse) == (case.jacobian == "sparse")
  assert [int(x) for x in d.nefc.cpu().ravel()] == list(case.targets)
  worlds = _worlds(mjm, m, d)
  inv = sc.solver_invariants(worlds, case.njmax, sentinel=True)
  combine = max(_combine_excess(a) for a in worlds)
  print(case.id, {k: inv[k] for k in sc.VALUES + ("state_bad", "nonfinite", "touched", "boundary_share", "qfrc_abs")}, "combine", combine)
  for k in sc.VALUES:
    assert inv[k] <= sc.TOL, (k, inv[k])
  assert inv["state_bad"] == 0 and inv["nonfinite"] == 0 and inv["touched"] == 0
  assert inv["boundary_share"] <= sc.BOUNDARY_CAP
  assert inv["qfrc_abs"] == 0.0
  assert combine <= 1e-5
  _assert_state_unchanged(d, before)


# ---- 2. the round trip ----------------------------------------------------------------------------------
ROUND_TRIP_XML = """<mujoco><compiler angle="radian"/>
<option timestep="0.01" gravity="-1 -1 -1" integrator="{integrator}" jacobian="{jacobian}"><flag contact="disable"{flags}/></option>
<worldbody>
 <body><joint name="a" type="hinge" axis="0 1 0" damping="0.1"/><geom type="capsule" size="0.05" fromto="0 0 0 0.6 0 0"/>
  <body pos="0.6 0 0"><joint name="b" type="hinge" axis="0 1 0" damping="0.2"/><geom type="capsule" size="0.08" fromto="0 0 0 0.9 0 0"/></body>
 </body>
</worldbody>
<actuator><motor joint="a"/></actuator>
<equality><joint joint1="a" joint2="b"/></equality>
</mujoco>"""


def _noisy_data(mjm, nworld, seed, key=None):
  """Data with qvel noise 0.01 and ctrl / qfrc_applied / xfrc_applied noise 0.1 around qpos0 (or a keyframe)."""
  import torch

  import mujoco_warp_amd as mjw

  rng = np.random.default_rng(seed)
  m = mjw.put_model(mjm, device="cuda")
  d = mjw.make_data(mjm, nworld=nworld, device="cuda", m=m)
  f32 = lambda x: torch.as_tensor(np.asarray(x, np.float32), device="cuda")  # noqa: E731
  qvel0 = np.zeros(mjm.nv)
  if key is not None:
    d.qpos[:] = f32(mjm.key_qpos[key])
    qvel0 = np.asarray(mjm.key_qvel[key])
  d.qvel[:] = f32(qvel0 + rng.normal(0, 0.01, (nworld, mjm.nv)))
  d.ctrl[:] = f32(rng.normal(0, 0.1, (nworld, mjm.nu)))
  d.qfrc_applied[:] = f32(rng.normal(0, 0.1, (nworld, mjm.nv)))
  xfrc = rng.normal(0, 0.1, (nworld, mjm.nbody, 6))
  xfrc[:, 0] = 0.0
  d.xfrc_applied[:] = f32(xfrc)
  return m, d


def _round_trip(m, d, qacc_in=None):
  """forward, the outputs zeroed, [qacc replaced,] inverse; returns what the assertions compare."""
  import torch

  import mujoco_warp_amd as mjw

  mjw.forward(m, d)
  want_c = np_(d.qfrc_constraint)
  ext = torch.zeros_like(d.qfrc_applied)
  mjw.xfrc_accumulate(m, d, ext)
  want_inv = np_(d.qfrc_applied) + np_(d.qfrc_actuator) + np_(ext)
  if qacc_in is not None:
    d.qacc[:] = qacc_in
  qacc_bits = _bits(d.qacc)
  for t in (d.qfrc_constraint, d.qfrc_inverse):
    t.zero_()
  mjw.inverse(m, d)
  torch.cuda.synchronize()
  assert torch.equal(_bits(d.qacc), qacc_bits)  # restored bitwise
  err = lambda got, want: float((np.abs(got - want) / (RT_TOL + RT_TOL * np.abs(want))).max())  # noqa: E731
  return err(np_(d.qfrc_inverse), want_inv), err(np_(d.qfrc_constraint), want_c), np.abs(want_c).max(), np.abs(want_inv).max()


@pytest.mark.parametrize("invdiscrete", [False, True], ids=["continuous", "invdiscrete"])
@pytest.mark.parametrize("jacobian", ["dense", "sparse"])
@pytest.mark.parametrize("integrator", ["Euler", "implicitfast"])
def test_inverse_round_trip(integrator, jacobian, invdiscrete):
  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf

  flags = ' invdiscrete="enable"' if invdiscrete else ""
  mjm = mjcf.load_model_from_string(ROUND_TRIP_XML.format(integrator=integrator, jacobian=jacobian, flags=flags))
  assert bool(mjm.opt.enableflags & mjw.EnableBit.INVDISCRETE) == invdiscrete
  m, d = _noisy_data(mjm, 32, seed=17)
  assert bool(m.is_sparse) == (jacobian == "sparse")
  qacc_in = None
  if invdiscrete:  # the discrete-time acceleration of one step of a twin
    _, twin = _noisy_data(mjm, 32, seed=17)
    qvel = twin.qvel.clone()
    mjw.step(m, twin)
    qacc_in = (twin.qvel - qvel) / 0.01
  e_inv, e_c, mag_c, mag_inv = _round_trip(m, d, qacc_in)
  print(integrator, jacobian, invdiscrete, "share of the bar: qfrc_inverse", e_inv, "qfrc_constraint", e_c, "magnitudes", mag_c, mag_inv)
  assert int(d.nefc.min()) == 1 and mag_c > 0.0  # the equality row is live
  assert e_inv <= 1.0 and e_c <= 1.0


def test_discrete_acc_without_eulerdamp_is_a_copy():
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf
  from mujoco_warp_amd.inverse import discrete_acc

  mjm = mjcf.load_model_from_string(ROUND_TRIP_XML.format(integrator="Euler", jacobian="dense", flags=' eulerdamp="disable"'))
  m, d = _noisy_data(mjm, 4, seed=3)
  mjw.forward(m, d)
  out = torch.zeros_like(d.qacc)
  discrete_acc(m, d, out)
  assert torch.equal(_bits(out), _bits(d.qacc)) and bool(d.qacc.abs().max() > 0)


# ---- 3. tendon armature -----------------------------------------------------------------------------------
def test_inverse_round_trip_with_tendon_armature():
  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model(os.path.join(ROOT, "tests", "golden", "tendon", "armature.xml"))
  mjm.opt.disableflags |= int(mjw.DisableBit.GRAVITY | mjw.DisableBit.CONSTRAINT)
  m, d = _noisy_data(mjm, 8, seed=5, key=0)
  e_inv, e_c, mag_c, mag_inv = _round_trip(m, d)
  print("tendon armature: share of the bar", e_inv, e_c, "magnitude", mag_inv)
  assert e_inv <= 1.0 and mag_inv > 0.0
  assert not bool(d.qfrc_constraint.any())  # exactly zero


# ---- 4. elliptic cones --------------------------------------------------------------------------------------
ELLIPTIC_XML = """<mujoco><option timestep="0.002" cone="elliptic" solver="Newton" jacobian="{jacobian}"/>
<worldbody><geom type="plane" size="5 5 .1" friction="0.6 0.01 0.001" condim="3"/>
 <body pos="0 0 .1"><freejoint/><geom type="sphere" size=".1" friction="0.6 0.01 0.001" condim="3"/></body>
 <body pos=".5 0 .1"><freejoint/><geom type="sphere" size=".1" friction="0.4 0.02 0.001" condim="4"/></body>
 <body pos="1 0 .1"><freejoint/><geom type="sphere" size=".1" friction="0.8 0.01 0.001" condim="3"/></body>
</worldbody></mujoco>"""
# the seed: on the fp64 and the fp32 oracle build the perturbed state has 15 top, 26 middle and 4 bottom contacts, none
# within BAND of a zone boundary, and 15 contacts cut by njmax
ELL_NWORLD, ELL_NJMAX, ELL_NCONMAX, ELL_SEED = 24, 8, 4, 3


def elliptic_states(mjm, nworld=ELL_NWORLD, seed=ELL_SEED):
  """Three spheres on or just above a plane (each touches in about four worlds of five), sliding, lifting off or
  pressing in: tangential and normal velocities of the same size, so that all three cone zones occur."""
  rng = np.random.default_rng(seed)
  qpos = np.tile(mjm.qpos0, (nworld, 1))
  qvel = np.zeros((nworld, mjm.nv))
  for b in range(3):
    touch = rng.uniform(size=nworld) < 0.8
    qpos[:, 7 * b + 2] = np.where(touch, 0.1 - rng.uniform(0.0005, 0.004, nworld), 0.1 + rng.uniform(0.01, 0.05, nworld))
    qvel[:, 6 * b: 6 * b + 2] = rng.normal(0, 0.4, (nworld, 2))
    qvel[:, 6 * b + 2] = rng.normal(0, 0.4, nworld)
    qvel[:, 6 * b + 3: 6 * b + 6] = rng.normal(0, 2.0, (nworld, 3))
  qpos[0, 2::7] = 0.098  # world 0: all three touch, 3 + 4 + 3 rows > njmax = 8, the last contact is cut
  return qpos, qvel, np.zeros((nworld, mjm.nu))


def cone_check(a, out, cones):
  """Force and state of one world's rows against inverse_ref: (worst error over max D s, worst error over the
  row's own D s, state mismatches, boundary contacts); a contact within BAND of a zone boundary may match any
  zone's law, as long as force and state agree."""
  n = out["n"]
  if n == 0:
    return 0.0, 0.0, 0, 0
  Ds = np.maximum(np.asarray(a["D"][:n], np.float64) * out["s"], 1e-300)
  f, st = np.asarray(a["force"][:n], np.float64), np.asarray(a["state"][:n]).astype(int)
  df = np.abs(np.where(np.isfinite(f), f, np.inf) - out["force"])
  bad = st != out["state"]
  near = 0
  for r0, dim, mu, fr, whole in cones:
    if not whole:
      continue
    rows = slice(r0, r0 + dim)
    if ir.cone_near(out["jar"][rows], out["s"][rows], mu, fr):
      near += 1
      for zone in ir.ZONES:
        wf, ws, _ = ir.cone_law(out["jar"][rows], np.asarray(a["D"], np.float64)[rows], mu, fr, zone=zone)
        if (st[rows] == ws).all():
          df[rows], bad[rows] = np.abs(f[rows] - wf), False
  for r in np.nonzero(out["dist"] < sc.BAND * out["s"])[0]:
    wf, ws = sc._other_side(out["jar"], np.asarray(a["D"], np.float64), np.asarray(a["fl"], np.float64), int(a["ne"]), int(a["nf"]), r)
    if st[r] == ws:
      df[r], bad[r] = abs(f[r] - wf), False
  return float(df.max() / Ds.max()), float((df / Ds).max()), int(bad.sum()), near


@pytest.mark.parametrize("jacobian", ["dense", "sparse"])
def test_inverse_elliptic_cones(jacobian):
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model_from_string(ELLIPTIC_XML.format(jacobian=jacobian))
  assert mjm.nv == 18
  m, d, before = _perturbed_inverse(mjm, elliptic_states(mjm), ELL_NJMAX, ELL_NCONMAX, ELL_SEED + 7)
  assert bool(m.is_sparse) == (jacobian == "sparse")
  worlds = _worlds(mjm, m, d)
  etype, eid = d.efc.type.cpu().numpy(), d.efc.id.cpu().numpy()
  adr0, cdim, cfr = d.contact.efc_address[:, 0].cpu().numpy(), d.contact.dim.cpu().numpy(), np_(d.contact.friction)
  iri = float(m.opt.impratio_invsqrt.reshape(-1)[0])
  worst = dict(force=0.0, force_row=0.0, qfrc=0.0, qfrc_dof=0.0, Ma=0.0, combine=0.0)
  zones, ncone, near, bad, cut, touched, nonfinite = [], 0, 0, 0, 0, 0, 0
  for w, a in enumerate(worlds):
    n = min(a["nefc"], ELL_NJMAX)
    cones = ir.cones_of(etype[w], eid[w], adr0, cdim, cfr, iri, n)
    out = ir.inverse_world(a, ELL_NJMAX, cones)
    fw, fr, b, nr = cone_check(a, out, cones)
    worst["force"], worst["force_row"] = max(worst["force"], fw), max(worst["force_row"], fr)
    bad, near = bad + b, near + nr
    zones += out["zones"]
    ncone += sum(1 for c in cones if c[4])
    cut += sum(1 for c in cones if not c[4])
    inv = sc.world_invariants(a, ELL_NJMAX, sentinel=True)  # its J'f, M qacc and sentinel checks do not depend on the row law
    for k in ("qfrc", "qfrc_dof", "Ma"):
      worst[k] = max(worst[k], inv[k])
    assert inv["qfrc_abs"] == 0.0
    touched, nonfinite = touched + inv["touched"], nonfinite + inv["nonfinite"]
    worst["combine"] = max(worst["combine"], _combine_excess(a))
  print(jacobian, worst, "zones", {z: zones.count(z) for z in ir.ZONES}, "contacts", ncone, "near", near, "cut", cut)
  assert set(zones) == set(ir.ZONES)  # all three zones occur in the fp64 restatement
  assert cut >= 1  # a contact whose rows njmax cuts
  assert near <= sc.BOUNDARY_CAP * ncone
  for k in sc.VALUES:
    assert worst[k] <= sc.TOL, (k, worst[k])
  assert worst["combine"] <= 1e-5
  assert bad == 0 and touched == 0 and nonfinite == 0
  _assert_state_unchanged(d, before)


# ---- 5. grid and sensors ------------------------------------------------------------------------------------
def test_inverse_on_257_humanoid_worlds():
  """More worlds than any multiple of a block: inverse at forward's own qacc against inverse_ref of the device's
  arrays.  The bar is the edge test's, per dof: 1e-5 of |bias| + |M| |qacc| + |passive| + |J|' (D s), the constraint
  term on the scale tests/solver_cases gives a row's force (D s, s = |J| |qacc| + |aref|): the row law is
  continuous in Jaref, whose fp32 rounding is 1e-7 s per term."""
  import torch

  import mujoco_warp_amd as mjw

  mjm = humanoid_model("NEWTON")
  m, d = gpu_from_state(mjm, *random_states(mjm, 257, seed=5, qpos_noise=0.1), njmax=128, nconmax=32)
  mjw.forward(m, d)
  qacc_bits = _bits(d.qacc)
  d.qfrc_inverse.zero_()
  mjw.inverse(m, d)
  torch.cuda.synchronize()
  assert torch.equal(_bits(d.qacc), qacc_bits)
  worst = 0.0
  for a in _worlds(mjm, m, d):
    out = ir.inverse_world(a, d.njmax)
    n = out["n"]
    J, D = np.asarray(a["J"][:n], np.float64), np.asarray(a["D"][:n], np.float64)
    scale = np.abs(a["qfrc_bias"]) + np.abs(a["M"]) @ np.abs(a["qacc"]) + np.abs(a["qfrc_passive"]) + np.abs(J).T @ (D * out["s"])
    worst = max(worst, float((np.abs(a["qfrc_inverse"] - out["qfrc_inverse"]) / scale).max()))
  print("humanoid x 257: worst qfrc_inverse error over its scale", worst, "nefc", int(d.nefc.min()), int(d.nefc.max()))
  assert worst <= 1e-5


def test_acceleration_sensors_after_inverse_match_forward():
  """Accelerometer and gyro depend on the state and qacc only: inverse at forward's own qacc reproduces them."""
  import torch

  import mujoco_warp_amd as mjw
  from tests.parity_models import setup

  mjm, qpos, qvel, ctrl, njmax, nconmax, nworld = setup("apollo")
  keep = [s for s in range(mjm.nsensor) if int(mjm.sensor_type[s]) in (int(mjw.types.SensorType.ACCELEROMETER), int(mjw.types.SensorType.GYRO))]
  assert {int(mjm.sensor_type[s]) for s in keep} == {int(mjw.types.SensorType.ACCELEROMETER), int(mjw.types.SensorType.GYRO)}
  m, d = gpu_from_state(mjm, qpos[:8], qvel[:8], ctrl[:8], njmax=njmax, nconmax=nconmax)
  mjw.forward(m, d)
  want = np_(d.sensordata)
  d.sensordata.zero_()
  mjw.inverse(m, d)
  torch.cuda.synchronize()
  got = np_(d.sensordata)
  for s in keep:
    a, n = int(mjm.sensor_adr[s]), int(mjm.sensor_dim[s])
    assert np.abs(want[:, a: a + n]).max() > 0.0
    np.testing.assert_allclose(got[:, a: a + n], want[:, a: a + n], rtol=1e-5, atol=1e-5)
