"""Scenes, images and meshes shared by tests/test_texture.py (CPU) and tests/test_gpu_texture.py (GPU).

Every drawn geom, camera and light hangs on the world body, so the frames are known on the host
(render_scenes.host_frames_all at qpos0).  Like every render scene the models have one free body, a small ball in
group 4, which the default groups do not draw.  Images and OBJ files are written by the tests into a directory of
their own; the scenes name them by absolute path.
"""

import struct
import zlib

import numpy as np

from tests.render_scenes import look_at

BALL = '<body name="ball" pos="0 0 -5"><freejoint/><geom name="ball" size=".1" group="4"/></body>'
SUN = '<light name="sun" type="directional" dir="0.3 0.2 -1" castshadow="false"/>'

# eight distinct, high-contrast texels, 2 rows of 4 (row 0 first)
TEX8 = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0]],
                 [[0, 255, 255], [255, 0, 255], [255, 255, 255], [16, 16, 16]]], dtype=np.uint8)


def write_png(path, px, depth=8):
  """px (H, W) or (H, W, C) with C in 1 (grey), 2 (grey + alpha), 3 (RGB), 4 (RGBA), as an 8- or 16-bit PNG (filter 0)."""
  px = np.asarray(px)
  if px.ndim == 2:
    px = px[:, :, None]
  h, w, c = px.shape
  ctype = {1: 0, 2: 4, 3: 2, 4: 6}[c]
  rows = px.astype(">u2" if depth == 16 else np.uint8).reshape(h, -1)
  raw = b"".join(b"\x00" + rows[r].tobytes() for r in range(h))
  chunk = lambda kind, body: struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
  with open(path, "wb") as f:
    f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw))
            + chunk(b"IEND", b""))
  return str(path)


def uv_sphere_obj(path, nseg=8, nring=6, radius=0.5, vt=True):
  """A latitude / longitude sphere as an OBJ of 2 nseg (nring - 1) triangles (80) with one `vt` per grid point."""
  lines, vid = [], {}
  for r in range(nring + 1):
    th = np.pi * r / nring
    for s in range(nseg + 1):
      ph = 2 * np.pi * s / nseg
      x, y, z = (float(c) for c in (radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), radius * np.cos(th)))
      lines.append(f"v {x!r} {y!r} {z!r}")
      vid[r, s] = len(vid) + 1
  if vt:
    for r in range(nring + 1):
      for s in range(nseg + 1):
        lines.append(f"vt {s / nseg!r} {1.0 - r / nring!r}")
  c = (lambda i: f"{i}/{i}") if vt else (lambda i: f"{i}")
  for r in range(nring):
    for s in range(nseg):
      a, b, cc, d = vid[r, s], vid[r + 1, s], vid[r + 1, s + 1], vid[r, s + 1]
      if r > 0:
        lines.append(f"f {c(a)} {c(b)} {c(d)}")
      if r < nring - 1:
        lines.append(f"f {c(b)} {c(cc)} {c(d)}")
  with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
  return str(path)


TETRA = ('vertex="0 0 0  1 0 0  0 1 0  0 0 1" face="0 2 1  0 1 3  1 2 3  0 3 2"')
TETRA_UV = 'texcoord="0.1 0.1  0.9 0.2  0.2 0.9  0.6 0.6"'

PLANE_VIEW = ((1.9, -2.3, 2.2), (0.3, -0.2, 0.1))


def _asset(png, extra=""):
  return (f'<asset><texture name="t8" type="2d" file="{png}"/>'
          '<texture name="chk" type="2d" builtin="checker" width="6" height="4" rgb1="1 0.9 0.2" rgb2="0.1 0.2 0.9" mark="edge" markrgb="1 1 1"/>'
          '<texture name="sky" type="skybox" builtin="gradient" rgb1="1 1 1" rgb2="0 0 0" width="8" height="48"/>'
          '<material name="m8" texture="t8" texrepeat="1.5 0.75" rgba="0.9 0.8 1 1"/>'
          '<material name="plain" rgba="0.4 0.7 0.3 1"/>'
          f'{extra}</asset>')


def plane_xml(png, extra_world="", lights=SUN):
  """Scene 1: a rotated, offset, finite plane with the 4 x 2 texture; local coordinates of both signs are in view."""
  return (f'<mujoco model="tex_plane">{_asset(png)}<worldbody>'
          '<geom name="floor" type="plane" size="1.6 1.3 1" pos="0.3 -0.2 0.1" euler="10 -15 30" material="m8"/>'
          f'<camera name="view" fovy="42" {look_at(*PLANE_VIEW)}/>{lights}{extra_world}{BALL}</worldbody></mujoco>')


def shadow_xml(png):
  """Scene 5: scene 1 with an occluder and a shadow-casting spot light."""
  return plane_xml(png, '<geom name="occluder" type="sphere" size=".3" pos="0.4 -0.3 0.9" rgba=".9 .9 .9 1"/>',
                   lights='<light name="spot" type="spot" pos="0.2 -0.1 3.0" dir="0.05 -0.05 -1" castshadow="true"/>' + SUN)


def mesh_xml(png, obj):
  """Scene 2: an inline tetrahedron with per-vertex uv (the face loop) and an OBJ sphere with vt (the walk)."""
  extra = (f'<mesh name="tetra" {TETRA} {TETRA_UV}/><mesh name="ball" file="{obj}"/>')
  return (f'<mujoco model="tex_mesh">{_asset(png, extra)}<worldbody>'
          '<geom name="tetra" type="mesh" mesh="tetra" pos="-0.9 0 0" euler="20 30 40" material="m8"/>'
          '<geom name="ball" type="mesh" mesh="ball" pos="0.5 0.1 0.5" euler="15 25 35" material="m8"/>'
          f'<camera name="view" fovy="27" {look_at((0.6, -2.6, 1.9), (-0.1, 0.0, 0.35))}/>{SUN}{BALL}</worldbody></mujoco>')


def untextured_xml(png):
  """Scene 3: a sphere, a box and a mesh without texcoords, all with the textured material, over an untextured plane."""
  extra = f'<mesh name="bare" {TETRA}/>'
  return (f'<mujoco model="tex_untextured">{_asset(png, extra)}<worldbody>'
          '<geom name="floor" type="plane" size="3 3 1" material="plain"/>'
          '<geom name="sphere" type="sphere" size=".4" pos="-0.9 0 .4" material="m8"/>'
          '<geom name="box" type="box" size=".3 .3 .3" pos="0.1 .3 .3" euler="0 0 25" material="m8"/>'
          '<geom name="bare" type="mesh" mesh="bare" pos="0.9 -0.4 0" euler="0 0 40" material="m8"/>'
          f'<camera name="view" fovy="50" {look_at((0.2, -2.6, 1.8), (0.1, 0.0, 0.3))}/>{SUN}{BALL}</worldbody></mujoco>')


def flex_xml(png):
  """Scene 6: a textured floor under a 3 x 3 cloth, seen from above."""
  cloth = ('<flexcomp type="grid" name="sheet" dim="2" count="3 3 1" spacing=".5 .5 .1" pos="0.2 0.1 0" radius="0.02" mass="1" rgba=".8 .3 .2 1">'
           '<contact contype="0" conaffinity="0"/></flexcomp>')
  return (f'<mujoco model="tex_flex"><option gravity="0 0 0"/>{_asset(png)}<worldbody><camera name="top" pos="0 0 3" fovy="45"/>{SUN}'
          f'<geom name="floor" type="plane" size="1.9 1.1 .1" pos="0 0 -0.6" material="m8"/>{cloth}</worldbody></mujoco>')


# the resolutions of the GPU tests: tiles with edges, and the one-wave path
RES_TILES, RES_WAVE = (40, 24), (8, 8)
