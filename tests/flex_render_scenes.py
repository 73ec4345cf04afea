"""Small flex scenes for tests/test_flex_render.py and tests/test_gpu_flex_render.py, and the deformations the tests
write into d.flexvert_xpos.

Unless said otherwise a scene is seen from a camera 3 m above the origin looking down (fovy 45): at 33 x 17 pixels the picture spans
about 4.8 m x 2.5 m of the plane z = 0, so a sheet of 1.2 m x 1.2 m or more covers over 10 % of it.  The sheets are
coarse on purpose: few silhouette and crease pixels, so nearly every pixel is decisive (see flex_render_ref).
"""

import numpy as np

CAM = '<camera name="top" pos="0 0 3" fovy="45"/>'
SUN = '<light name="sun" type="directional" dir="0.25 0.15 -1" castshadow="true"/>'
SPOT = '<light name="spot" type="spot" pos="0.4 -0.2 2.8" dir="-0.1 0.05 -1" castshadow="true"/>'
FLOOR = '<geom name="floor" type="plane" size="1.9 1.1 .1" pos="0 0 -0.6" rgba=".3 .5 .3 1"/>'
_NOCOL = '<contact contype="0" conaffinity="0"/>'


def flexcomp(name, dim, count, spacing, pos="0 0 0", radius=0.02, rgba=None, mass=1.0):
  col = f' rgba="{rgba}"' if rgba else ""
  return (f'<flexcomp type="grid" name="{name}" dim="{dim}" count="{count}" spacing="{spacing}" pos="{pos}" radius="{radius}" mass="{mass}"{col}>'
          f'{_NOCOL}</flexcomp>')


def scene(*parts, lights=SUN, floor=True, cam=CAM):
  return f'<mujoco><option gravity="0 0 0"/><worldbody>{cam}{lights}{FLOOR if floor else ""}{"".join(parts)}</worldbody></mujoco>'


SHEET3 = flexcomp("sheet", 2, "3 3 1", ".7 .7 .1", radius=0.02, rgba=".8 .3 .2 1")  # 8 elements, 8 fragments: 32 faces
SHEET76 = flexcomp("sheet", 2, "7 6 1", ".3 .3 .1", radius=0.02, rgba=".2 .4 .9 1")  # 60 elements, 22 fragments: 164 faces
ROPE = flexcomp("rope", 1, "4 1 1", ".5 .1 .1", pos="0 -0.8 0.3", radius=0.08, rgba=".9 .8 .1 1")  # 3 edges
BLOCK = flexcomp("block", 3, "2 2 2", ".6 .6 .6", pos="-1.4 0.5 0.2", radius=0.0, rgba=".6 .2 .7 1")  # 12 shell faces
DEFAULT_COLOUR = flexcomp("plain", 2, "2 2 1", ".2 .2 .1")

SHEET3_XML = scene(SHEET3)
SHEET76_XML = scene(SHEET76)
# alone, the rope and the block are seen from close above, so that they too cover a tenth of the picture
ROPE_XML = scene(ROPE, cam='<camera name="top" pos="0 -0.8 1.5" fovy="45"/>')
BLOCK_XML = scene(BLOCK, cam='<camera name="top" pos="-1.4 0.5 1.7" fovy="45"/>')
# a sheet, a rope and a soft body in one model: flex ids 0, 1, 2
MIXED_XML = scene(flexcomp("sheet", 2, "3 3 1", ".6 .6 .1", pos="0.6 0.3 0", radius=0.02, rgba=".8 .3 .2 1"), ROPE, BLOCK)
# a sphere in front of the sheet and a box behind it, over the plane; an 8 x 8 camera for the one-wave path
OCCLUSION_XML = scene(SHEET3, '<geom name="ball" type="sphere" size=".25" pos="0.3 0.2 0.6" rgba=".9 .9 .2 1"/>',
                      '<geom name="slab" type="box" size=".5 .3 .05" pos="-1.1 0 -0.3" rgba=".2 .8 .8 1"/>')
# a sheet for the collapsed element, a sheet without thickness, and a rope for the zero-length edge (the sheets lie off
# the picture's middle row, whose rays would otherwise run along a row of element edges)
DEGENERATE_XML = scene(flexcomp("sheet", 2, "3 3 1", ".6 .6 .1", pos="0.5 0.07 0", radius=0.02, rgba=".8 .3 .2 1"),
                       flexcomp("thin", 2, "3 3 1", ".5 .5 .1", pos="-1.2 -0.06 0", radius=0.0, rgba=".2 .4 .9 1"), ROPE)
# no flex at all (the ball is a free body: like every scene of tests/render_scenes.py the model has dofs)
PLAIN_XML = scene('<body name="ball" pos="0 0 0.2"><freejoint/><geom name="ball" type="sphere" size=".4" rgba=".9 .2 .2 1"/></body>',
                  '<geom name="cap" type="capsule" size=".1 .4" pos="1 0.3 0" euler="0 70 20" rgba=".2 .2 .9 1"/>')
EXPLICIT_RGBA_XML = scene(SHEET3, DEFAULT_COLOUR)


def saddle(x0, amp, shift=(0.0, 0.0, 0.0), tilt=0.0):
  """Rest positions x0 (n, 3) bent into z += amp (x^2 - y^2) + tilt x, then moved by shift."""
  x = np.array(x0, dtype=np.float64)
  c = x[:, :2] - x[:, :2].mean(axis=0)
  x[:, 2] += amp * (c[:, 0] ** 2 - c[:, 1] ** 2) + tilt * c[:, 0]
  return x + np.asarray(shift, dtype=np.float64)


# shadows: the sheet shadows the plane and a sphere shadows the sheet, under one directional and one spot light.  The
# sun is slanted: the camera looks straight down, so under a sun from above the sheet would hide its own shadow.
SLANTED_SUN = '<light name="sun" type="directional" dir="0.8 0.3 -1" castshadow="true"/>'
SHADOW_XML = scene(SHEET3, '<geom name="ball" type="sphere" size=".3" pos="-0.5 -0.1 0.9" rgba=".9 .9 .2 1"/>', lights=SLANTED_SUN + SPOT)
# two sheets without thickness in the same place, in two colours, and the first of them alone: every flex pixel is a tie
_TIE_A = flexcomp("a", 2, "2 2 1", "1.4 1.4 .1", radius=0.0, rgba=".9 .1 .1 1")
TIE_XML = scene(_TIE_A, flexcomp("b", 2, "2 2 1", "1.4 1.4 .1", radius=0.0, rgba=".1 .9 .1 1"), floor=False)
TIE_FIRST_XML = scene(_TIE_A, floor=False)


def sheet3_worlds(rest):
  """Three deformations of the 3 x 3 sheet; the last lies wholly outside the boxes of the other two."""
  return np.stack([saddle(rest, 0.5), saddle(rest, -0.4, tilt=0.3), saddle(rest, 0.3, shift=(0.5, 0.2, 0.9))])


def wavy(rest, amp=0.15):
  """A smooth deformation for ropes and soft bodies: z += amp sin(3 x) + amp / 2 cos(2 y), x += amp / 3 z."""
  x = np.array(rest, dtype=np.float64)
  x[:, 2] += amp * np.sin(3.0 * x[:, 0]) + 0.5 * amp * np.cos(2.0 * x[:, 1])
  x[:, 0] += amp / 3.0 * x[:, 2]
  return x


def degenerate(mjm, rest):
  """The DEGENERATE_XML scene bent, with one collapsed element in the thick sheet (vertex 1 on vertex 0) and a
  zero-length first edge in the rope."""
  x = wavy(rest, 0.1)
  va = [int(v) for v in mjm.flex_vertadr]
  x[va[0] + 1] = x[va[0]]
  x[va[2] + 1] = x[va[2]]
  return x
