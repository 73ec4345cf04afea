"""Scenes and cameras shared by tests/test_render.py (CPU) and tests/test_gpu_render.py (GPU)."""

import numpy as np

from tests.ray_scenes import ALL_TYPES_XML


def look_at(pos, target, up=(0.0, 0.0, 1.0)):
  """The `pos` and `xyaxes` attributes of a camera at pos looking at target (a camera looks along its -z, +y up)."""
  pos, target = np.asarray(pos, dtype=np.float64), np.asarray(target, dtype=np.float64)
  f = (target - pos) / np.linalg.norm(target - pos)
  x = np.cross(f, np.asarray(up, dtype=np.float64))
  x /= np.linalg.norm(x)
  y = np.cross(x, f)
  s = lambda v: " ".join(repr(float(c)) for c in v)
  return f'pos="{s(pos)}" xyaxes="{s(x)} {s(y)}"'


# the view the decisiveness figures were measured at, and a close camera each for the mesh and the heightfield
MAIN_VIEW = ((1.2, -2.6, 2.4), (1.2, 0.7, 0.9))
MESH_VIEW = ((1.9, 0.3, 1.7), (1.12, 1.12, 1.1))
HFIELD_VIEW = ((0.1, 2.9, 1.9), (0.0, 2.0, 1.03))

CAMS = (f'<camera name="main" fovy="60" {look_at(*MAIN_VIEW)}/>'
        f'<camera name="mesh" fovy="40" {look_at(*MESH_VIEW)}/>'
        f'<camera name="hfield" fovy="50" {look_at(*HFIELD_VIEW)}/>')
LIGHTS = ('<light name="sun" directional="true" dir="0.3 0.2 -1" pos="0 0 5"/>'
          '<light name="lamp" pos="1.5 -1 3" dir="0 0 -1"/>')

# ALL_TYPES_XML (geom ids 0-8, the free ball is body 1) with three cameras and two lights in the world body
RENDER_ALL_TYPES_XML = ALL_TYPES_XML.replace("</worldbody>", CAMS + LIGHTS + "</worldbody>")
ALL_TYPES_RES = [(64, 48), (33, 17), (33, 17)]
ALL_TYPES_QPOS = np.array([[-1.0, -1.0, 1.0, 1, 0, 0, 0], [2.0, 2.0, 1.5, 0.8, 0.6, 0, 0], [0.5, -1.0, 2.0, 0.5, 0.5, 0.5, 0.5]])

# a camera pair on a free body (body 2; its own geom is in group 4, which the default groups do not draw): one by
# fovy, one by intrinsics with a 4 : 3 sensor and an off-centre principal point
RIG_XML = ALL_TYPES_XML.replace(
  "</worldbody>",
  LIGHTS + f'<body name="rig" pos="1.2 -2.6 2.4"><freejoint/><geom size=".05" group="4"/>'
  f'<camera name="rigcam" fovy="60" {look_at((0, 0, 0), (0.0, 3.3, -1.5))}/>'
  f'<camera name="intr" sensorsize="0.02 0.015" focal="0.015 0.014" principal="0.001 -0.0005" {look_at((0, 0, 0), (0.0, 3.3, -1.5))}/>'
  "</body></worldbody>")
BALL0 = [-1.0, -1.0, 1.0, 1, 0, 0, 0]
RIG_QPOS = np.array([BALL0 + [1.2, -2.6, 2.4, 1, 0, 0, 0], BALL0 + [0.6, -2.4, 2.2, 0.9914449, 0, 0, -0.1305262],
                     BALL0 + [1.8, -2.2, 2.0, 0.9961947, 0.0610485, 0, 0.0610485]])

_LIGHT_VIEW = ((1.8, -2.4, 2.2), (0.4, 0.1, 0.2))
LIGHTS_XML = f"""<mujoco model="render_lights">
  <asset><material name="red" rgba="0.3 0.1 0.05 1"/></asset>
  <worldbody>
    <geom name="floor" type="plane" size="3 3 1" material="red" rgba="0 1 0 1"/>
    <geom name="sphere" type="sphere" size=".4" pos="0 0 .4" rgba=".2 .6 .9 1"/>
    <geom name="box" type="box" size=".3 .3 .3" pos="1.2 .3 .3" rgba=".9 .9 .2 1"/>
    <camera name="view" fovy="55" {look_at(*_LIGHT_VIEW)}/>
    <light name="sun" type="directional" dir="0.4 0.3 -1" castshadow="false"/>
    <light name="bulb" type="point" pos="-0.8 -1.0 1.6"/>
    <light name="spot" type="spot" pos="0.5 -0.3 2.5" dir="0.05 0 -1"/>
    <light name="off" type="point" pos="1 -1 1" active="false"/>
    <body name="ball" pos="-1.2 0.8 0.3"><freejoint/><geom name="ball" size=".2" rgba=".7 .7 .7 1"/></body>
  </worldbody>
</mujoco>"""


def shadow_xml(castshadow="true"):
  """A sphere over a plane under one point light."""
  return f"""<mujoco model="render_shadow">
  <worldbody>
    <geom name="floor" type="plane" size="3 3 1" rgba=".8 .8 .8 1"/>
    <geom name="sphere" type="sphere" size=".3" pos="0 0 .8" rgba=".2 .6 .9 1"/>
    <camera name="view" fovy="50" {look_at((1.6, -2.0, 2.4), (0.0, 0.0, 0.2))}/>
    <light name="bulb" type="point" pos="0.3 0.2 3" castshadow="{castshadow}"/>
    <body name="ball" pos="-1.5 1.5 0.2"><freejoint/><geom name="ball" size=".2"/></body>
  </worldbody>
</mujoco>"""


# groups and alpha: "hidden" is in group 3, "ghost" has alpha 0 in group 0
GROUPS_XML = f"""<mujoco model="render_groups">
  <worldbody>
    <geom name="floor" type="plane" size="3 3 1" rgba=".5 .5 .5 1"/>
    <geom name="hidden" type="sphere" size=".3" pos="-0.5 0 .5" group="3" rgba="1 0 0 1"/>
    <geom name="ghost" type="sphere" size=".3" pos="0.5 0 .5" rgba="0 0 1 0"/>
    <camera name="view" fovy="50" {look_at((0.0, -2.2, 1.6), (0.0, 0.0, 0.4))}/>
    <light name="sun" type="directional" dir="0 0.2 -1"/>
    <body name="ball" pos="0 1.5 0.2"><freejoint/><geom name="ball" size=".2"/></body>
  </worldbody>
</mujoco>"""

# 129 small spheres in a row (ids 0-128: the last lies in the second 128-geom chunk) and a camera at the row's end
ROW_N = 129
ROW_XML = ('<mujoco model="render_row"><worldbody>'
           + "".join(f'<geom type="sphere" size="0.04" pos="{0.1 * i!r} 0 0.04"/>' for i in range(ROW_N))
           + f'<camera name="view" fovy="32" {look_at((12.55, -0.5, 0.45), (12.55, 0.0, 0.04))}/>'
           + '<light name="sun" type="directional" dir="0 0.2 -1"/>'
           + '<body name="ball" pos="12.5 1 0.2"><freejoint/><geom name="ball" size=".2"/></body></worldbody></mujoco>')


def host_frames_all(mjm, qpos=None):
  """Geom, camera and light frames of a scene whose free bodies are unrotated-at-qpos0 children of the world, at
  qpos (free joints only, in body order; None: qpos0): a dict of float64 arrays like the one the GPU tests read back."""
  from tests.ray_scenes import quat_mat

  nb = int(mjm.nbody)
  bpos = np.asarray(mjm.body_pos, dtype=np.float64).copy()
  bmat = np.tile(np.eye(3), (nb, 1, 1))
  if qpos is not None:
    for b in range(1, nb):
      q = np.asarray(qpos, dtype=np.float64)[7 * (b - 1) : 7 * b]
      bpos[b], bmat[b] = q[:3], quat_mat(q[3:])
  place = lambda body, pos: bpos[body] + np.einsum("nij,nj->ni", bmat[body], np.asarray(pos, dtype=np.float64).reshape(-1, 3))
  rot = lambda body, quat: np.einsum("nij,njk->nik", bmat[body], np.array([quat_mat(q) for q in np.asarray(quat).reshape(-1, 4)]).reshape(-1, 3, 3))
  gb, cb, lb = np.asarray(mjm.geom_bodyid), np.asarray(mjm.cam_bodyid), np.asarray(mjm.light_bodyid)
  return dict(geom_xpos=place(gb, mjm.geom_pos), geom_xmat=rot(gb, mjm.geom_quat), cam_xpos=place(cb, mjm.cam_pos), cam_xmat=rot(cb, mjm.cam_quat),
              light_xpos=place(lb, mjm.light_pos),
              light_xdir=np.einsum("nij,nj->ni", bmat[lb], np.asarray(mjm.light_dir, dtype=np.float64).reshape(-1, 3)))
