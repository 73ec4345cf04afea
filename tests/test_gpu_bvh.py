"""The mesh BVH on the device (csrc/mjw_ray.h `mesh_bvh`): `rays(rc=rc)` and `render` walk each mesh's tree in place
of the loop over every face and must give that loop's result bit for bit, on every ray and pixel.

The face loop is the same build's: `rays(rc=None)`, and for `render` a call with a per-world batched `mesh_vert` of
identical rows, which takes the fallback.  The same rays and images are also held against the float64 yardsticks
(tests/ray_ref.py, tests/render_ref.py) at the bars of tests/test_gpu_ray.py and tests/test_gpu_render.py: on
decisive rays the geom id exact, distance and normal to atol = rtol = 5e-4; tests/test_bvh.py checks on the CPU
that at least 90 % of the rays are decisive.  The scene (tests/bvh_scenes.py) holds meshes of 4, 5, 37 and 268 faces
with duplicated triangles, two geoms sharing a mesh in different frames, primitives and a heightfield.  A context
walks the meshes of at least `bvh_min_faces` faces (default 64) and loops over the smaller ones; the tests set it to
0, so that every mesh is walked, and the first also to each face count's edge and to the default.
"""

import numpy as np
import pytest

from tests import bvh_scenes as scenes
from tests import ray_ref

pytestmark = pytest.mark.gpu

TOL = 5e-4
MIN_DECISIVE = 0.9
NRAYS = (1, 64, 65, 300)  # a lane, a wave, over a wave, over the 256-ray tile


@pytest.fixture(scope="module")
def scene():
  """The scene on the device in three worlds with different qpos, after one forward: mjm, m, d, frames, aabb."""
  from mujoco_warp_amd import mjcf
  from tests.test_gpu_ray import _device

  mjm = mjcf.load_model_from_string(scenes.SCENE_XML)
  m, d, (xpos, xmat) = _device(mjm, 3, scenes.SCENE_QPOS)
  return mjm, m, d, xpos, xmat, np.asarray(mjm.geom_aabb, dtype=np.float64).reshape(-1, 6)


def _ctx(mjm, nworld, min_faces=0):
  """A render context whose trees are walked for the meshes of at least min_faces faces (None: the default)."""
  import mujoco_warp_amd as mjw

  rc = mjw.create_render_context(mjm, nworld=nworld, cam_res=(4, 3), device="cuda")
  if min_faces is not None:
    rc.bvh_min_faces = min_faces
  return rc


def _cast(m, d, pnt, vec, rc, geomgroup=None, flg_static=True, bodyexclude=None):
  """mjw.rays from numpy inputs (pnt / vec: (nb, nray, 3)); geomid, dist, normal as numpy (dist / normal float32)."""
  import torch

  import mujoco_warp_amd as mjw

  nray = pnt.shape[1]
  t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
  excl = t(np.full(nray, -1) if bodyexclude is None else bodyexclude, torch.int32)
  dist = torch.full((d.nworld, nray), 7.0, dtype=torch.float32, device="cuda")
  geomid = torch.full((d.nworld, nray), 7, dtype=torch.int32, device="cuda")
  normal = torch.full((d.nworld, nray, 3), 7.0, dtype=torch.float32, device="cuda")
  mjw.rays(m, d, t(pnt, torch.float32), t(vec, torch.float32), geomgroup, flg_static, excl, dist, geomid, normal, rc=rc)
  torch.cuda.synchronize()
  return geomid.cpu().numpy(), dist.cpu().numpy(), normal.cpu().numpy()


def _same(a, b, label):
  np.testing.assert_array_equal(a[0], b[0], err_msg=f"{label}: geomid")
  assert a[1].tobytes() == b[1].tobytes(), f"{label}: dist differs at rays {np.nonzero(a[1] != b[1])}"
  assert a[2].tobytes() == b[2].tobytes(), f"{label}: normal differs at rays {np.nonzero((a[2] != b[2]).any(-1))}"


def _world_rays(scene, nray, worlds):
  mjm, m, d, xpos, xmat, aabb = scene
  pv = [scenes.scene_rays(xpos[w], xmat[w], aabb, nray, seed=1000 * w + nray) for w in worlds]
  return np.stack([p for p, _ in pv]), np.stack([v for _, v in pv])


@pytest.mark.parametrize("min_faces", [0, 5, 38, 268, 269, None])
def test_gpu_rays_bvh_bitwise_as_the_face_loop(scene, min_faces):
  """Every ray, decisive or not: nray 1 / 64 / 65 / 300, three worlds with their own qpos and rays (aimed, parallel to
  an axis, starting inside a mesh's box, neighbours aimed at different meshes), and one set of rays for all worlds.
  min_faces 0 walks every mesh; 5 / 38 / 268 / 269 put the 4- / 37- / 268-face meshes on either side of the
  threshold; None is the context's default."""
  import mujoco_warp_amd as mjw

  mjm, m, d, xpos, xmat, aabb = scene
  rc = _ctx(mjm, 3, min_faces)
  first = np.zeros(mjm.ngeom, dtype=int)
  for nray in NRAYS:
    pnt, vec = _world_rays(scene, nray, range(3))
    for p, v, label in ((pnt, vec, "per world"), (pnt[:1], vec[:1], "broadcast")):
      loop, walk = _cast(m, d, p, v, None), _cast(m, d, p, v, rc)
      _same(walk, loop, f"nray {nray} {label}")
      first += np.bincount(loop[0][loop[0] >= 0], minlength=mjm.ngeom)
  print("first hits per geom", first)
  assert all(first[g] >= 20 for g in scenes.MESH_GEOMS), first  # every mesh size, both frames of the shared mesh
  assert first[[0, 1, 2, 3, 4]].min() >= 3  # the primitives and the heightfield are met beside them
  # ray() takes the context too
  import torch

  p1, v1 = pnt[:, :1], vec[:, :1]
  t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda")
  d1, g1, n1 = mjw.ray(m, d, t(p1), t(v1), rc=rc)
  d0, g0, n0 = mjw.ray(m, d, t(p1), t(v1))
  assert torch.equal(d1, d0) and torch.equal(g1, g0) and torch.equal(n1, n0)


def test_gpu_rays_bvh_one_world(scene):
  """nworld 1 (its own Data and context) at every ray count."""
  import mujoco_warp_amd as mjw
  from tests.test_gpu_ray import _device

  mjm = scene[0]
  m, d, (xpos, xmat) = _device(mjm, 1, scenes.SCENE_QPOS[1:2])
  rc = _ctx(mjm, 1)
  for nray in NRAYS:
    pnt, vec = scenes.scene_rays(xpos[0], xmat[0], scene[5], nray, seed=77 + nray)
    _same(_cast(m, d, pnt[None], vec[None], rc), _cast(m, d, pnt[None], vec[None], None), f"nray {nray}")


def test_gpu_rays_bvh_filters(scene):
  """A mesh geom removed by bodyexclude, by group and by alpha 0 is removed from the walk as from the loop."""
  import mujoco_warp_amd as mjw

  mjm, m, d, xpos, xmat, aabb = scene
  rc = _ctx(mjm, 3)
  names = list(mjm.geom_names)
  hidden, ghost, torus3 = names.index("hidden"), names.index("ghost"), names.index("torus3")
  assert mjm.geom_group[hidden] == 3 and mjm.geom_rgba[ghost][3] == 0.0 and mjm.geom_bodyid[torus3] == scenes.FREE_BODY
  # straight down through the hidden ball, the ghost torus' tube and the free torus' tube (world 0's pose), and aimed rays
  centre = lambda g: xpos[0][g] + xmat[0][g] @ aabb[g, :3]
  down = np.array([centre(hidden) + [0.01, 0.02, 2.0], centre(ghost) + [0.35, 0.01, 2.0], centre(torus3) + [0.35, 0.01, 2.0]])
  pnt, vec = _world_rays(scene, 125, [0])
  pnt, vec = np.concatenate([down, pnt[0]])[None], np.concatenate([np.tile([0.0, 0.0, -1.0], (3, 1)), vec[0]])[None]
  nray = pnt.shape[1]
  excl_free = np.full(nray, scenes.FREE_BODY)
  cases = {
    "no filter": dict(),
    "groups 0-2": dict(geomgroup=(1, 1, 1, 0, 0, 0)),
    "group 3 only": dict(geomgroup=(0, 0, 0, 1, 0, 0)),
    "not static": dict(flg_static=False),
    "bodyexclude free": dict(bodyexclude=excl_free),
    "bodyexclude mix": dict(bodyexclude=np.where(np.arange(nray) % 2 == 0, scenes.FREE_BODY, -1)),
  }
  got = {}
  for label, kw in cases.items():
    got[label] = _cast(m, d, pnt, vec, rc, **kw)
    _same(got[label], _cast(m, d, pnt, vec, None, **kw), label)
  gid = got["no filter"][0][0]
  assert gid[0] == hidden and gid[1] == 0 and gid[2] == torus3  # alpha 0: the ray goes through the ghost to the plane
  assert ghost not in set(gid.tolist())
  assert got["groups 0-2"][0][0][0] == 0 and hidden not in set(got["groups 0-2"][0][0].tolist())
  assert set(got["group 3 only"][0][0].tolist()) == {-1, hidden}
  assert set(got["not static"][0][0].tolist()) <= {-1, torus3, names.index("ball2")}
  assert torus3 not in set(got["bodyexclude free"][0][0].tolist()) and got["bodyexclude free"][0][0][2] == 0
  assert got["bodyexclude mix"][0][0][2] == 0 and torus3 in set(got["bodyexclude mix"][0][0].tolist())


def test_gpu_rays_bvh_against_yardstick(scene):
  """The same rays against tests/ray_ref.py at the bar of tests/test_gpu_ray.py, on decisive rays."""
  import mujoco_warp_amd as mjw

  mjm, m, d, xpos, xmat, aabb = scene
  rc = _ctx(mjm, 3)
  total = decisive = mesh_first = 0
  for nray in NRAYS:
    pnt, vec = _world_rays(scene, nray, range(3))
    gid, dist, nrm = _cast(m, d, pnt, vec, rc)
    for w in range(3):
      p, v = pnt[w].astype(np.float32).astype(np.float64), vec[w].astype(np.float32).astype(np.float64)
      g, x, n, ok = ray_ref.cast(mjm, xpos[w], xmat[w], p, v)
      label = f"nray {nray} world {w}"
      bad = np.nonzero(ok & (gid[w] != g))[0]
      assert len(bad) == 0, f"{label}: geom id of ray {bad[0]}: device {gid[w][bad[0]]} (dist {dist[w][bad[0]]}), yardstick {g[bad[0]]} (dist {x[bad[0]]})"
      np.testing.assert_allclose(dist[w][ok], x[ok], rtol=TOL, atol=TOL, err_msg=f"{label}: dist")
      np.testing.assert_allclose(nrm[w][ok], n[ok], rtol=TOL, atol=TOL, err_msg=f"{label}: normal")
      miss = gid[w] < 0
      assert np.all(dist[w][miss] == -1.0) and not nrm[w][miss].any()
      total, decisive = total + nray, decisive + int(ok.sum())
      hit = ok & (g >= 0)
      mesh_first += int((np.asarray(mjm.geom_type)[g[hit]] == ray_ref.MESH).sum())
  print(f"decisive {decisive} of {total} rays ({decisive / total:.4f}); {mesh_first} decisive first hits on a mesh")
  assert decisive / total >= MIN_DECISIVE and mesh_first >= total // 4


def _images(m, d, rc):
  from tests.test_gpu_render import _render

  return [a.copy() for a in _render(m, d, rc)]


@pytest.mark.parametrize("shadows", [False, True])
def test_gpu_render_bvh(scene, shadows):
  """`render` on the mesh scene, with and without shadows (the any-hit walk), at tile shapes 1 x 1, 16 x 16 and
  33 x 17: against tests/render_ref.py at the bar of tests/test_gpu_render.py, and bitwise against the face loop,
  which a per-world batched mesh_vert of identical rows forces."""
  from tests.test_gpu_render import _Tally, _context

  mjm, m, d, xpos, xmat, aabb = scene
  nworld = 3
  tally = _Tally()
  keep = m.mesh_vert
  assert keep.shape[0] == 1
  batched = keep.repeat(nworld, *([1] * (keep.dim() - 1))).contiguous()
  try:
    for W, H in ((1, 1), (16, 16), (33, 17)):
      kw = dict(cam_res=(W, H), render_rgb=True, render_depth=True, render_seg=True, use_shadows=shadows)
      rc, rc_loop = _context(mjm, nworld, **kw), _context(mjm, nworld, **kw)
      part = _images(m, d, rc)  # the default: only the 268-face mesh is walked
      rc.bvh_min_faces = 0
      walk = _images(m, d, rc)
      for a, b in zip(walk, part):
        assert a.tobytes() == b.tobytes()
      m.mesh_vert = batched
      loop = _images(m, d, rc_loop)
      m.mesh_vert = keep
      for a, b, name in zip(walk, loop, ("rgb", "depth", "seg")):
        assert a.tobytes() == b.tobytes(), f"{W} x {H}: {name} differs from the face loop's at {np.nonzero(a != b)}"
      tally.context(mjm, m, d, rc, walk, f"{W} x {H} shadows {shadows}", worlds=[0, 2] if (W, H) == (33, 17) else None)
      if (W, H) == (33, 17):
        seen = set(walk[2].ravel().tolist())
        assert set(scenes.MESH_GEOMS) <= seen, seen  # every mesh is in some picture
  finally:
    m.mesh_vert = keep
  tally.check_skipped()
  assert tally.hits[ray_ref.MESH] >= 100


def test_gpu_rays_bvh_batched_mesh_vert_falls_back(scene):
  """With a per-world mesh_vert whose rows differ the trees (built from the host model's vertices) would be wrong:
  `rays(rc=rc)` runs the face loop, so it follows each world's vertices as `rays(rc=None)` does."""
  import mujoco_warp_amd as mjw

  mjm, m, d, xpos, xmat, aabb = scene
  rc = _ctx(mjm, 3)
  keep = m.mesh_vert
  batched = keep.repeat(3, *([1] * (keep.dim() - 1))).contiguous()
  batched[1] *= 1.5  # world 1's meshes are half as large again
  pnt, vec = _world_rays(scene, 300, [0])
  base = _cast(m, d, pnt, vec, None)
  try:
    m.mesh_vert = batched
    loop, walk = _cast(m, d, pnt, vec, None), _cast(m, d, pnt, vec, rc)
  finally:
    m.mesh_vert = keep
  _same(walk, loop, "batched mesh_vert")
  _same([a[0] for a in walk], [a[0] for a in base], "world 0 keeps its vertices")
  assert (walk[1][1] != base[1][1]).mean() > 0.2  # world 1 does see larger meshes


def test_gpu_bvh_graph_capture(scene):
  """forward + render with the BVH captured in a graph and replayed at two states."""
  import torch

  import mujoco_warp_amd as mjw
  from tests.test_gpu_render import SENTINEL, _context, _device

  mjm = scene[0]
  nworld = 3
  m, d = _device(mjm, nworld, scenes.SCENE_QPOS)
  kw = dict(cam_res=(33, 17), render_rgb=True, render_depth=True, render_seg=True, use_shadows=True)
  eager, graphed = _context(mjm, nworld, **kw), _context(mjm, nworld, **kw)
  eager.bvh_min_faces = graphed.bvh_min_faces = 0
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g, stream=s):
    mjw.forward(m, d)
    mjw.render(m, d, graphed)
  torch.cuda.synchronize()
  assert bool((graphed.seg_data == SENTINEL).all())  # capture records, it does not run
  moved = torch.as_tensor(scenes.SCENE_QPOS[::-1].copy(), dtype=torch.float32, device="cuda")
  first = None
  for qpos in (d.qpos.clone(), moved):
    d.qpos[:] = qpos
    g.replay()
    torch.cuda.synchronize()
    mjw.forward(m, d)
    mjw.render(m, d, eager)
    torch.cuda.synchronize()
    for name in ("rgb_data", "depth_data", "seg_data"):
      assert torch.equal(getattr(eager, name), getattr(graphed, name)), name
    if first is None:
      first = eager.seg_data.clone()
  assert not torch.equal(first, eager.seg_data)  # the free meshes moved between the replays
  seen = set(eager.seg_data.unique().tolist())
  assert len(seen & set(scenes.MESH_GEOMS)) >= 4
