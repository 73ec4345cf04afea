"""Meshes, scenes and seeded rays shared by tests/test_bvh.py (CPU) and tests/test_gpu_bvh.py (GPU).

The meshes are generated here and written inline (`<mesh vertex= face=>`): closed shapes, so the compiler's hull
step works, with the face count set by the resolution, and variants with a block of duplicated triangles (which
also gives the odd counts a closed surface cannot have).  Face counts: BVH_LEAF (a root that is a leaf),
BVH_LEAF + 1 (the first split), 37 (no power of two) and 260 + 8.
"""

import numpy as np

from tests.render_scenes import look_at


def tetrahedron():
  v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64) * 0.5
  return v, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])


def uv_sphere(nseg, nstack, radius=0.3):
  """2 nseg (nstack - 1) faces: two fans and nstack - 2 bands."""
  v = [[0.0, 0.0, radius]]
  for i in range(1, nstack):
    th = np.pi * i / nstack
    v += [[radius * np.sin(th) * np.cos(2 * np.pi * (j + 0.37) / nseg), radius * np.sin(th) * np.sin(2 * np.pi * (j + 0.37) / nseg), radius * np.cos(th)]
          for j in range(nseg)]
  v.append([0.0, 0.0, -radius])
  ring = lambda i, j: 1 + (i - 1) * nseg + j % nseg
  f = [[0, ring(1, j), ring(1, j + 1)] for j in range(nseg)]
  for i in range(1, nstack - 1):
    for j in range(nseg):
      f += [[ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)], [ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)]]
  last = len(v) - 1
  f += [[last, ring(nstack - 1, j + 1), ring(nstack - 1, j)] for j in range(nseg)]
  return np.array(v), np.array(f)


def torus(nu, nv, R=0.35, r=0.12):
  """2 nu nv faces."""
  u, w = np.meshgrid(2 * np.pi * (np.arange(nu) + 0.21) / nu, 2 * np.pi * (np.arange(nv) + 0.13) / nv, indexing="ij")
  v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], axis=-1).reshape(-1, 3)
  idx = lambda i, j: (i % nu) * nv + j % nv
  f = []
  for i in range(nu):
    for j in range(nv):
      f += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
  return v, np.array(f)


def with_duplicates(vf, faces, at):
  """The mesh with copies of `faces` (face ids) inserted at position `at` of its face list."""
  v, f = vf
  return v, np.concatenate([f[:at], f[list(faces)], f[at:]])


def mesh_xml(name, vf):
  v, f = vf
  return (f'<mesh name="{name}" vertex="{" ".join(repr(float(round(x, 6))) for x in np.asarray(v).ravel())}" '
          f'face="{" ".join(str(int(i)) for i in np.asarray(f).ravel())}"/>')


# name -> (vertices, faces); the face counts the tests name
MESHES = {
  "tet4": tetrahedron(),
  "tet5": with_duplicates(tetrahedron(), [2], 1),
  "ball37": with_duplicates(uv_sphere(6, 4), [10], 30),
  "torus268": with_duplicates(torus(13, 10), [5, 6, 7, 8, 100, 101, 5, 5], 50),
}
NFACE = {"tet4": 4, "tet5": 5, "ball37": 37, "torus268": 268}

_ASSETS = "".join(mesh_xml(k, vf) for k, vf in MESHES.items())
_VIEW = ((1.6, -3.2, 2.6), (1.6, 0.6, 0.6))
_CLOSE = ((3.4, -0.9, 1.5), (3.0, 0.0, 0.8))

# Geoms 0-4 primitives and a heightfield, 5-8 one geom per mesh, 9 a second torus in another frame, 10 a ball in
# group 3, 11 a transparent torus, 12 (body 1, free) a third torus, 13 (body 2, free) a ball mesh.
SCENE_XML = f"""<mujoco model="bvh_scene">
  <asset>{_ASSETS}<hfield name="hf" nrow="3" ncol="2" elevation="1 2 3 3 2 1" size=".6 .4 .1 .1"/></asset>
  <worldbody>
    <geom name="plane" type="plane" size="6 6 1" rgba=".4 .4 .4 1"/>
    <geom name="box" type="box" size=".3 .2 .25" pos="-1 1.2 .5" quat="0.9238795 0 0.3826834 0"/>
    <geom name="sphere" type="sphere" size=".3" pos="-1 0 .6"/>
    <geom name="capsule" type="capsule" size=".15 .3" pos="4.2 1.2 .6" quat="0.9238795 0.3826834 0 0"/>
    <geom name="hfield" type="hfield" hfield="hf" pos="4.2 0 .4"/>
    <geom name="tet4" type="mesh" mesh="tet4" pos="0 0 .5" quat="0.9238795 0 0 0.3826834" rgba=".9 .3 .3 1"/>
    <geom name="tet5" type="mesh" mesh="tet5" pos="1 0 .5" quat="0.8 0.6 0 0" rgba=".3 .9 .3 1"/>
    <geom name="ball37" type="mesh" mesh="ball37" pos="2 0 .6" quat="0.5 0.5 0.5 0.5" rgba=".3 .3 .9 1"/>
    <geom name="torus" type="mesh" mesh="torus268" pos="3 0 .8" quat="0.9238795 0.3826834 0 0" rgba=".9 .9 .3 1"/>
    <geom name="torus2" type="mesh" mesh="torus268" pos="3.3 0.15 .8" quat="0.7071068 0 0.7071068 0" rgba=".3 .9 .9 1"/>
    <geom name="hidden" type="mesh" mesh="ball37" pos="0.5 1.2 .6" group="3"/>
    <geom name="ghost" type="mesh" mesh="torus268" pos="0.5 2.0 .8" rgba="1 1 1 0"/>
    <camera name="view" fovy="55" {look_at(*_VIEW)}/>
    <camera name="close" fovy="45" {look_at(*_CLOSE)}/>
    <light name="sun" type="directional" dir="0.3 0.2 -1"/>
    <light name="lamp" type="point" pos="2.5 -1.5 3"/>
    <body name="free" pos="2.2 1.3 1.0"><freejoint/><geom name="torus3" type="mesh" mesh="torus268" rgba=".9 .5 .2 1"/></body>
    <body name="free2" pos="3.0 1.4 1.6"><freejoint/><geom name="ball2" type="mesh" mesh="ball37" rgba=".6 .2 .8 1"/></body>
  </worldbody>
</mujoco>"""
MESH_GEOMS = (5, 6, 7, 8, 9, 12, 13)
FREE_BODY = 1
SCENE_QPOS = np.array([[2.2, 1.3, 1.0, 1, 0, 0, 0, 3.0, 1.4, 1.6, 1, 0, 0, 0],
                       [1.5, -0.9, 1.2, 0.8, 0.6, 0, 0, 0.1, 0.1, 1.4, 0.5, 0.5, 0.5, 0.5],
                       [3.1, 0.1, 1.5, 0.5, -0.5, 0.5, 0.5, 2.0, 0.05, 1.3, 0.9238795, 0, 0.3826834, 0]])
LO, HI = np.array([-2.0, -2.0, 0.05]), np.array([5.0, 2.5, 3.0])


def scene_rays(xpos, xmat, aabb, nray, seed):
  """nray seeded rays for the scene at the geom frames xpos (ngeom, 3), xmat (ngeom, 3, 3); aabb = geom_aabb
  (ngeom, 6).  A mix, by ray index mod 8: 0-3 aimed from the scene's box at a jittered mesh centre; 4 aimed at any
  geom; 5 parallel to a world axis through a jittered mesh centre; 6 starting inside a mesh geom's bounding box;
  7 parallel to an axis of the mesh's own frame (components that are exactly zero in the geom frame of an
  unrotated mesh).  Neighbouring rays aim at different meshes, so a wave straddles several."""
  rng = np.random.default_rng(seed)
  xpos, xmat, aabb = np.asarray(xpos, dtype=np.float64), np.asarray(xmat, dtype=np.float64), np.asarray(aabb, dtype=np.float64)
  centre = lambda g: xpos[g] + xmat[g] @ aabb[g, :3]
  pnt, vec = np.zeros((nray, 3)), np.zeros((nray, 3))
  for i in range(nray):
    g = MESH_GEOMS[int(rng.integers(0, len(MESH_GEOMS)))]
    kind = i % 8
    tgt = centre(g) + rng.normal(0, 0.12, 3)
    if kind <= 4:
      if kind == 4:
        tgt = xpos[int(rng.integers(0, len(xpos)))] + rng.normal(0, 0.2, 3)
      p = rng.uniform(LO, HI)
      v = tgt - p
      v /= np.linalg.norm(v)
      if i % 3 == 0:
        v *= rng.uniform(0.3, 3.0)
    elif kind == 5:
      k, s = int(rng.integers(0, 3)), float(rng.choice([-1.0, 1.0]))
      v = np.zeros(3)
      v[k] = s
      p = tgt - v * rng.uniform(1.0, 2.0)
    elif kind == 6:
      p = centre(g) + xmat[g] @ (rng.uniform(-0.9, 0.9, 3) * aabb[g, 3:])
      v = rng.normal(0, 1, 3)
      v /= np.linalg.norm(v)
    else:
      k, s = int(rng.integers(0, 3)), float(rng.choice([-1.0, 1.0]))
      v = xmat[g][:, k] * s
      p = tgt - v * rng.uniform(1.0, 2.0)
    pnt[i], vec[i] = p, v
  return pnt, vec


def walk(node, tri, adr, mesh, vert, face, lp, lv, triangle):
  """A plain walk of mesh `mesh`'s tree for one ray (lp, lv in the mesh frame) with exact slabs grown by 1e-9:
  (distance, face) of the nearest triangle, the lowest face id among equal distances, (-1, -1) for a miss.
  `triangle` is ray_ref.triangle; vert / face are the mesh's own (float64 vertices, local indices)."""
  ints = node.view(np.int32)
  n0, nn, t0, _ = (int(v) for v in adr[mesh])
  best, bf = np.inf, -1
  stack = [0]
  while stack:
    k = stack.pop()
    lo, hi = node[n0 + k, 0:3].astype(np.float64) - 1e-9, node[n0 + k, 3:6].astype(np.float64) + 1e-9
    tmin, tmax = 0.0, np.inf
    for i in range(3):
      if lv[i] == 0.0:
        if not (lo[i] <= lp[i] <= hi[i]):
          tmin, tmax = 1.0, 0.0
      else:
        a, b = (lo[i] - lp[i]) / lv[i], (hi[i] - lp[i]) / lv[i]
        tmin, tmax = max(tmin, min(a, b)), min(tmax, max(a, b))
    if tmin > tmax or tmin > best:
      continue
    a, b = int(ints[n0 + k, 6]), int(ints[n0 + k, 7])
    if b <= 0:
      for f in tri[t0 + a : t0 + a - b]:
        x = float(triangle(lp[None], lv[None], *vert[face[f]])[0][0])
        if x >= 0 and (x < best or (x == best and f < bf)):
          best, bf = x, int(f)
    else:
      assert a > k and (b & ((1 << 29) - 1)) > k
      stack += [b & ((1 << 29) - 1), a]
  return (best, bf) if bf >= 0 else (-1.0, -1)
