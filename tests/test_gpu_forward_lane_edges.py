"""Forward stages at the edges of their lane maps: HIP path vs the fp64 oracle at the strict bar.

The velocity and acceleration stages run their per-component accumulations with one lane per (body,
component) pair -- e = lane, lane + 64, ... with body = e / 6 (cvel, cacc, cfrc_int, the applied-force
subtree sums) -- their tree recursions one level per pass, and copy cacc / cfrc_int to the Data in blocks;
subtree_com and crb walk their subtrees one lane per body.  The models here are the shapes at which
such maps change, not a workload: a single free body; a 31-hinge chain (32 levels, 192 pairs of 6 and
320 words of crb: several strided passes and the deepest subtree walk); a 31-body star (one level, every
subtree of size 1); nbody 11 and 7 (66 and 70 words: one past a wave at 6 and at 10 per body); a dof-less
welded body between two jointed ones and a body with three hinges; a free + ball + hinge + slide mix with
motors on a ball joint (6 moment slots per actuator) and two motors on one hinge (the per-dof actuator
order); and a dense-Jacobian model of nv 60 and nbody 71 that takes the generic kernel (nv 33..64), whose
level passes reach into the second 64-body chunk.  qfrc_actuator switches from the per-dof scan to the
slot push above 12 moment slots: the chain has 12 motors, the star 13, the mixed model 5 x 6 slots.

Every model is contact-free (contype = conaffinity = 0) with joint armature, so that qM is well
conditioned and the step's qpos / qvel hold the same elementwise bar as the smooth fields: rtol 1e-5
with a floor of 1e-6 * max |oracle| per world (test_gpu_parity_strict.py).  nworld 3, random qpos / qvel
/ ctrl, and a non-zero xfrc_applied on the mixed model.

Not covered: a model of the world body alone (nbody 1, nv 0).  forward() on it faults on the GPU, before
and after the lane-map change alike: the dense kernel's stage_fill (mjw_dense.h) loads qM[0] as the
dummy element of every lane outside the nv x nv block, and with nv = 0 qM is an empty tensor.
"""

import numpy as np
import pytest

from tests.common import gpu_from_state, np_, oracle_from_state
from tests.test_gpu_parity_strict import strict_close

pytestmark = pytest.mark.gpu

NWORLD = 3
DEFAULTS = '<default><geom contype="0" conaffinity="0" density="400"/><joint armature="0.05"/></default>'
OPT = '<option timestep="0.002"/>' + DEFAULTS
OPT_DENSE = '<option timestep="0.002" jacobian="dense"/>' + DEFAULTS
FIELDS = ("xpos", "xquat", "xmat", "xipos", "ximat", "xanchor", "xaxis", "geom_xpos", "geom_xmat", "subtree_com", "cinert", "cdof", "crb",
          "cvel", "cdof_dot", "cacc", "cfrc_int", "qfrc_bias", "qfrc_passive", "qfrc_actuator", "qfrc_smooth")
AXES = ("1 0 0", "0 1 0", "0 0 1", "1 1 0", "0 1 1")


def _link(i, pos, joints, inner=""):
  return f'<body name="b{i}" pos="{pos}">{joints}<geom type="capsule" size=".02" fromto="0 0 0 .06 .01 -.03"/>{inner}</body>'


def _hinge(i, extra=""):
  return f'<joint name="j{i}" type="hinge" axis="{AXES[i % len(AXES)]}" {extra}/>'


def _chain(n, first=1, weld_every=0):
  """n nested bodies, each on one hinge; with weld_every = k every k-th body carries no joint."""
  inner = ""
  for i in range(first + n - 1, first - 1, -1):
    jointed = not (weld_every and (i - first) % weld_every == weld_every - 1)
    inner = _link(i, ".06 .01 -.03", _hinge(i) if jointed else "", inner)
  return inner


def _wrap(bodies, actuators="", opt=OPT):
  act = f"<actuator>{actuators}</actuator>" if actuators else ""
  return f"<mujoco>{opt}<worldbody>{bodies}</worldbody>{act}</mujoco>"


def _motors(joints, gear="3"):
  return "".join(f'<motor joint="{j}" gear="{gear}"/>' for j in joints)


def _models():
  star = lambda n: "".join(_link(i, f"{0.1 * (i % 6)} {0.1 * (i // 6)} 0", _hinge(i, 'stiffness="2" damping=".1"')) for i in range(1, n + 1))
  mix = ('<body name="f" pos="0 0 1"><freejoint name="jf"/><geom type="box" size=".05 .04 .03"/>'
         '<body name="ba" pos=".1 0 0"><joint name="jb" type="ball" damping=".05"/><geom type="capsule" size=".02" fromto="0 0 0 .1 0 0"/>'
         '<body name="h" pos=".1 0 0"><joint name="jh" type="hinge" axis="0 1 0" stiffness="1"/><geom type="sphere" size=".03" pos=".05 0 0"/>'
         '<body name="s" pos=".05 0 0"><joint name="js" type="slide" axis="1 0 1"/><geom type="sphere" size=".02" pos="0 .02 0"/></body>'
         "</body></body></body>")
  mix_act = ('<motor joint="jb" gear="1 .5 -.7"/><motor joint="jh" gear="2"/><motor joint="js" gear="1.5"/>'
             '<motor joint="jh" gear="-.8"/><motor joint="jb" gear="0 2 1"/>')
  tri = (_link(1, "0 0 .5", _hinge(1), _link(2, ".06 0 0", "", _link(3, ".06 0 0", _hinge(3) + _hinge(4) + _hinge(5), _link(4, ".06 0 0", "", _link(5, ".06 0 0", _hinge(6)))))))
  return {
    "one_free": _wrap('<body pos="0 0 1"><freejoint/><geom type="box" size=".05 .04 .03"/></body>'),
    "chain31": _wrap(_chain(31), _motors([f"j{i}" for i in range(1, 13)])),
    "star31": _wrap(star(31), _motors([f"j{i}" for i in range(19, 32)])),
    "nbody11": _wrap(_chain(6) + _chain(4, first=7), _motors(["j3", "j9"])),
    "nbody7": _wrap(_chain(4) + _chain(2, first=5), _motors(["j6"])),
    "weld_and_three_hinges": _wrap(tri, _motors(["j4", "j6"])),
    "mixed_joints": _wrap(mix, mix_act),
    "generic_nb71": _wrap(_chain(35, weld_every=7) + _chain(35, first=36, weld_every=7), _motors(["j1", "j40", "j69"]), opt=OPT_DENSE),
  }


def _states(mjm, seed):
  rng = np.random.default_rng(seed)
  qpos = np.tile(np.asarray(mjm.qpos0, np.float64), (NWORLD, 1))
  for j in range(mjm.njnt):
    a, t = int(mjm.jnt_qposadr[j]), int(mjm.jnt_type[j])
    if t == 0:  # free: position jitter and a random unit quaternion
      qpos[:, a : a + 3] += rng.normal(0, 0.1, (NWORLD, 3))
      q = rng.normal(size=(NWORLD, 4))
      qpos[:, a + 3 : a + 7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    elif t == 1:  # ball
      q = rng.normal(size=(NWORLD, 4))
      qpos[:, a : a + 4] = q / np.linalg.norm(q, axis=1, keepdims=True)
    else:
      qpos[:, a] += rng.normal(0, 0.4 if t == 3 else 0.05, NWORLD)
  return qpos, rng.normal(0, 0.5, (NWORLD, mjm.nv)), rng.uniform(-1, 1, (NWORLD, mjm.nu))


def _check(name, got, want):
  got, want = np.asarray(got), np.asarray(want)
  assert got.size == want.size, f"{name}: {got.size} values vs {want.size}"
  if want.size:
    strict_close(name, got.reshape(NWORLD, -1), want.reshape(NWORLD, -1))


@pytest.mark.parametrize("name", list(_models()))
def test_forward_and_step_at_lane_edges(name):
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model_from_string(_models()[name])
  expect = {"one_free": (2, 6), "chain31": (32, 31), "star31": (32, 31), "nbody11": (11, 10), "nbody7": (7, 6),
            "weld_and_three_hinges": (6, 5), "mixed_joints": (5, 11), "generic_nb71": (71, 60)}[name]
  assert (mjm.nbody, mjm.nv) == expect
  qpos, qvel, ctrl = _states(mjm, seed=len(name))
  m, d = gpu_from_state(mjm, qpos, qvel, ctrl)
  om, od = oracle_from_state(mjm, qpos, qvel, ctrl)
  if name == "generic_nb71":
    assert not m.is_sparse and mjm.nv > 32  # the generic kernel, not the dense or the sparse path
  if name == "mixed_joints":
    xfrc = np.random.default_rng(7).normal(0, 5.0, (NWORLD, mjm.nbody, 6))
    xfrc[:, 0] = 0.0
    d.xfrc_applied[:] = torch.as_tensor(xfrc, dtype=torch.float32, device="cuda").reshape(d.xfrc_applied.shape)
    od.xfrc_applied[:] = xfrc.reshape(NWORLD, -1)
  mjw.forward(m, d)
  od.forward()
  torch.cuda.synchronize()
  for f in FIELDS:
    _check(f, np_(getattr(d, f)), getattr(od, f))
  nv = mjm.nv
  if nv:
    _check("qM", np_(d.qM)[:, :nv, :nv], od.qM)
  mjw.step(m, d)
  od.step()
  torch.cuda.synchronize()
  _check("qpos", np_(d.qpos), od.qpos)
  _check("qvel", np_(d.qvel), od.qvel)
