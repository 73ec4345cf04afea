"""Camera and light frames in every tracking mode, on the dense and on the sparse path.

The mode ladder of smooth.py:635-803 is written out twice: `camlight` in mjw_step.hip (the world-per-wave kernel,
opt.jacobian = dense) and `sp::camlight` in mjw_sparse.hip (the workgroup-per-world kernel, sparse).  Elsewhere the
sparse path only ever sees `fixed` items, so this scene carries one camera and one light per mode -- fixed, track,
trackcom, targetbody, targetbodycom, and a target mode without a target (the `tgt < 0` branch) -- on a free body with a
hinged child (its subtree's centre of mass is off the body origin, so trackcom differs from track), aimed at a second
free body.  Bar: the fp64 oracle's fwd_position at rtol 1e-5 with a floor of 1e-6 * scale (strict_close), which these
fields meet on the humanoid.
"""

import functools

import numpy as np
import pytest

from tests.common import gpu_from_state, np_, oracle_from_state
from tests.test_gpu_parity_strict import strict_close

pytestmark = pytest.mark.gpu

MODES = ("fixed", "track", "trackcom", "targetbody", "targetbodycom")
FIELDS = ("cam_xpos", "cam_xmat", "light_xpos", "light_xdir")
NWORLD = 3


def scene_xml(jacobian):
  items = []
  for i, mode in enumerate(MODES + ("targetbody",)):
    target = ' target="tgt"' if mode.startswith("target") and i < len(MODES) else ""
    x = round(0.1 * i - 0.2, 3)
    items.append(f'<camera name="c{i}" mode="{mode}"{target} pos="{x} 0.3 0.2" euler="{round(0.3 + 0.2 * i, 3)} 0.4 -0.2"/>')
    items.append(f'<light name="l{i}" mode="{mode}"{target} pos="{x} -0.3 0.25" dir="0.2 {round(0.1 * i - 0.3, 3)} -0.9"/>')
  return (f'<mujoco><compiler angle="radian"/><option timestep="0.002" jacobian="{jacobian}"/><worldbody>'
          '<body name="a" pos="0 0 1" euler="0.2 -0.3 0.5"><freejoint/><geom type="box" size=".1 .08 .05" contype="0" conaffinity="0"/>'
          + "".join(items) +
          '<body name="a2" pos=".25 .1 -.05"><joint type="hinge" axis="0 1 0"/>'
          '<geom type="capsule" size=".04 .15" pos=".1 0 0" contype="0" conaffinity="0"/></body></body>'
          '<body name="tgt" pos="0.9 0.6 0.4"><freejoint/><geom type="sphere" size=".07" pos=".05 .02 -.1" contype="0" conaffinity="0"/>'
          '<geom type="sphere" size=".03" pos="-.1 .1 .1" contype="0" conaffinity="0"/></body>'
          "</worldbody></mujoco>")


@functools.lru_cache(maxsize=None)
def case(jacobian):
  """(model, states, the oracle's frames): world 0 at qpos0, worlds 1 and 2 at seeded random poses with turned free joints."""
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model_from_string(scene_xml(jacobian))
  assert (mjm.nv, mjm.ncam, mjm.nlight) == (13, 6, 6)
  assert list(mjm.cam_targetbodyid[3:]) == [3, 3, -1] and list(mjm.light_targetbodyid[3:]) == [3, 3, -1]
  rng = np.random.default_rng(9)
  qpos = np.tile(mjm.qpos0, (NWORLD, 1))
  qpos[1:] += rng.normal(0, 0.3, (NWORLD - 1, mjm.nq))
  for adr in (3, 11):  # the two free joints' quaternions
    qpos[1:, adr:adr + 4] = rng.normal(0, 1, (NWORLD - 1, 4))
    qpos[:, adr:adr + 4] /= np.linalg.norm(qpos[:, adr:adr + 4], axis=1, keepdims=True)
  states = (qpos, np.zeros((NWORLD, mjm.nv)), np.zeros((NWORLD, mjm.nu)))
  _, od = oracle_from_state(mjm, *states)
  od.fwd_position()
  ref = {f: np.array(getattr(od, f), np.float64).reshape(NWORLD, -1) for f in FIELDS}
  for f in FIELDS:
    assert np.isfinite(ref[f]).all(), f
    ref[f].setflags(write=False)
  xmat = ref["cam_xmat"][1].reshape(mjm.ncam, 9)
  xdir = ref["light_xdir"][1].reshape(mjm.nlight, 3)
  for i in range(mjm.ncam):
    for j in range(i):  # every mode gives a frame of its own
      assert np.abs(xmat[i] - xmat[j]).max() > 1e-3, (i, j)
      assert np.abs(xdir[i] - xdir[j]).max() > 1e-3, (i, j)
  return mjm, states, ref


@pytest.mark.parametrize("jacobian", ["dense", "sparse"])
def test_camlight_modes(jacobian):
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd.forward import StepTracer
  from tests.sparse_cases import check_kernels

  mjm, states, ref = case(jacobian)
  m, d = gpu_from_state(mjm, *states)
  assert m.is_sparse == (jacobian == "sparse") and int(mjm.opt.jacobian) == (jacobian == "sparse")
  mjw.fwd_position(m, d)
  torch.cuda.synchronize()
  for f in FIELDS:
    strict_close(f"{jacobian} {f}", np_(getattr(d, f)).reshape(NWORLD, -1), ref[f])
  if jacobian == "sparse":
    tracer = StepTracer()
    tracer.step(m, d)
    torch.cuda.synchronize()
    check_kernels([k for k, _ in tracer.durations()[0]])
