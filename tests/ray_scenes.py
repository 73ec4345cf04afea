"""Scenes and seeded rays shared by tests/test_ray.py (CPU) and tests/test_gpu_ray.py (GPU)."""

import numpy as np

# every geom type once, static, plus a free sphere (body 1); geom ids 0-8
ALL_TYPES_XML = """<mujoco model="ray_all_types">
  <asset>
    <mesh name="tet" vertex="0 0 0  1 0 0  0 1 0  0 0 1" face="0 2 1  0 1 3  0 3 2  1 2 3" scale="0.4 0.4 0.4"/>
    <hfield name="hf" nrow="3" ncol="2" elevation="1 2 3 3 2 1" size=".6 .4 .1 .1"/>
  </asset>
  <worldbody>
    <geom name="plane" size="4 4 4" type="plane" rgba="0.1 0.1 0.1 1"/>
    <geom name="sphere" pos="0 0 1" size="0.5" type="sphere"/>
    <geom name="capsule" pos="0 1 1" quat="0 0.3826834 0 0.9238795" size="0.25 0.5" type="capsule"/>
    <geom name="box" pos="1 0 1" quat="0 0.3826834 0 0.9238795" size="0.5 0.25 0.3" type="box"/>
    <geom name="mesh" pos="1 1 1" quat="0 0 0.3826834 0.9238795" type="mesh" mesh="tet"/>
    <geom name="hfield" pos="0 2 1" type="hfield" hfield="hf"/>
    <geom name="cylinder" pos="2 0 1" quat="0 0 .3826834 .9238796" type="cylinder" size=".25 .5"/>
    <geom name="ell" pos="3 0 1" type="ellipsoid" size=".2 .3 .4"/>
    <body name="ball" pos="-1 -1 1"><freejoint/><geom name="ball" size=".2"/></body>
  </worldbody>
</mujoco>"""

SCENE_LO, SCENE_HI = np.array([-2.0, -2.0, 0.05]), np.array([4.0, 3.0, 3.0])


def aimed_rays(centres, n, seed, lo=SCENE_LO, hi=SCENE_HI, jitter=0.3):
  """n seeded rays from the box [lo, hi] aimed at jittered geom centres; every seventh direction is not
  normalised (length 0.3 to 3), the rest are unit vectors."""
  rng = np.random.default_rng(seed)
  centres = np.asarray(centres, dtype=np.float64)
  pnt = rng.uniform(lo, hi, (n, 3))
  tgt = centres[rng.integers(0, len(centres), n)] + rng.normal(0, jitter, (n, 3))
  vec = tgt - pnt
  vec /= np.linalg.norm(vec, axis=1, keepdims=True)
  vec[::7] *= rng.uniform(0.3, 3.0, (len(vec[::7]), 1))
  return pnt, vec


def quat_mat(q):
  w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
  return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def host_frames(mjm):
  """Geom frames at qpos0 of a model whose bodies are unrotated children of the world (the test scenes):
  xpos (ngeom, 3), xmat (ngeom, 3, 3)."""
  xpos = np.asarray(mjm.body_pos, dtype=np.float64)[np.asarray(mjm.geom_bodyid)] + np.asarray(mjm.geom_pos, dtype=np.float64)
  xmat = np.array([quat_mat(q) for q in np.asarray(mjm.geom_quat)]).reshape(-1, 3, 3)
  return xpos, xmat
