"""The mesh BVH, host side: the builder's invariants (mujoco_warp_amd/bvh.py), a numpy walk of the built trees
against the brute-force yardstick tests/ray_ref.py, the render context's tensors, the refusals of `rays(rc=...)`,
and the share of decisive rays of the ray sets tests/test_gpu_bvh.py casts (on the yardstick alone, from host-side
frames).  The kernel's walk is tested in tests/test_gpu_bvh.py."""

import numpy as np
import pytest

from tests import bvh_scenes as scenes
from tests import ray_ref

MIN_DECISIVE = 0.9


def _load(xml):
  from mujoco_warp_amd import mjcf

  return mjcf.load_model_from_string(xml)


@pytest.fixture(scope="module")
def mjm():
  return _load(scenes.SCENE_XML)


@pytest.fixture(scope="module")
def built(mjm):
  from mujoco_warp_amd import bvh

  return bvh.build_mesh_bvh(mjm.mesh_vert, mjm.mesh_vertadr, mjm.mesh_face, mjm.mesh_faceadr, mjm.mesh_facenum)


def _mesh(mjm, i):
  va, fa = int(mjm.mesh_vertadr[i]), int(mjm.mesh_faceadr[i])
  vert = np.asarray(mjm.mesh_vert, dtype=np.float32).reshape(-1, 3)[va : va + int(mjm.mesh_vertnum[i])]
  face = np.asarray(mjm.mesh_face).reshape(-1, 3)[fa : fa + int(mjm.mesh_facenum[i])]
  return vert, face


def test_scene_meshes_have_the_face_counts(mjm):
  from mujoco_warp_amd.bvh import BVH_LEAF

  assert [int(n) for n in mjm.mesh_facenum] == [scenes.NFACE[k] for k in scenes.MESHES] == [BVH_LEAF, BVH_LEAF + 1, 37, 268]
  assert [int(mjm.geom_type[g]) for g in scenes.MESH_GEOMS] == [ray_ref.MESH] * len(scenes.MESH_GEOMS)
  # the duplicated triangles are kept, in place
  _, face = _mesh(mjm, 1)
  assert np.array_equal(face[1], face[3])


def test_builder_invariants(mjm, built):
  from mujoco_warp_amd import bvh

  node, tri, adr, max_depth = built
  nmesh = int(mjm.nmesh)
  assert node.dtype == np.float32 and node.shape[1] == 8 and tri.dtype == np.int32 and adr.dtype == np.int32 and adr.shape == (nmesh, 4)
  assert tri.shape == (int(mjm.nmeshface),) and int(adr[:, 1].sum()) == len(node)
  ints = node.view(np.int32)
  for i in range(nmesh):
    vert, face = _mesh(mjm, i)
    nface = len(face)
    n0, nn, t0, depth = (int(v) for v in adr[i])
    assert t0 == int(mjm.mesh_faceadr[i]) and n0 == int(adr[:i, 1].sum())
    # every face exactly once
    assert sorted(tri[t0 : t0 + nface].tolist()) == list(range(nface))
    if nface <= bvh.BVH_LEAF:
      assert nn == 1 and ints[n0, 7] == -nface  # the root is a leaf
    if nface == bvh.BVH_LEAF + 1:
      assert nn == 3 and sorted([-ints[n0 + 1, 7], -ints[n0 + 2, 7]]) == [2, 3]  # the first split
    seen, leaves, deepest = np.zeros(nn, dtype=int), [], 0
    todo = [(0, 1)]
    while todo:
      k, level = todo.pop()
      seen[k] += 1
      deepest = max(deepest, level)
      lo, hi, a, b = node[n0 + k, 0:3], node[n0 + k, 3:6], int(ints[n0 + k, 6]), int(ints[n0 + k, 7])
      if b <= 0:
        cnt = -b
        assert 1 <= cnt <= bvh.BVH_LEAF and 0 <= a and a + cnt <= nface
        leaves.append((a, cnt))
        tv = vert[face[tri[t0 + a : t0 + a + cnt]]].reshape(-1, 3)
        assert np.array_equal(lo, tv.min(0)) and np.array_equal(hi, tv.max(0))  # exact float32 bounds, so every vertex is inside
      else:
        l, r, axis = a, b & ((1 << bvh.AXIS_SHIFT) - 1), b >> bvh.AXIS_SHIFT
        assert k < l < nn and r == l + 1 and r < nn and 0 <= axis <= 2
        for c in (l, r):
          assert np.all(node[n0 + c, 0:3] >= lo) and np.all(node[n0 + c, 3:6] <= hi)  # a child's box lies in its parent's
        assert np.array_equal(lo, np.minimum(node[n0 + l, 0:3], node[n0 + r, 0:3])) and np.array_equal(hi, np.maximum(node[n0 + l, 3:6], node[n0 + r, 3:6]))
        todo += [(l, level + 1), (r, level + 1)]
    assert np.all(seen == 1)  # a tree: every node reached once
    leaves.sort()
    assert leaves[0][0] == 0 and all(a + c == nxt for (a, c), (nxt, _) in zip(leaves, leaves[1:])) and sum(c for _, c in leaves) == nface
    assert deepest == depth <= bvh.depth_bound(nface) <= bvh.BVH_MAX_DEPTH
    assert bvh.depth_bound(nface) == max(int(np.ceil(np.log2(nface / bvh.BVH_LEAF))), 0) + 1
  assert max_depth == int(adr[:, 3].max())


def test_builder_ends_on_coincident_triangles():
  """64 copies of one triangle, and triangles whose centroids coincide: ties split by face id."""
  from mujoco_warp_amd import bvh

  vert = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 1]], dtype=np.float32)
  face = np.array([[0, 1, 2]] * 64 + [[0, 3, 4], [1, 2, 4]] * 5)  # the last two kinds share the centroid (0.5, 0.5, 1 / 3)
  node, tri, adr, depth = bvh.build_mesh_bvh(vert, [0], face, [0], [len(face)])
  assert sorted(tri.tolist()) == list(range(len(face))) and depth <= bvh.depth_bound(len(face))
  ints = node.view(np.int32)
  leaf = ints[:, 7] <= 0
  assert int(-ints[leaf, 7].sum()) == len(face) and int(-ints[leaf, 7].min()) >= 1 and int(-ints[leaf, 7].max()) <= bvh.BVH_LEAF
  # no mesh, and a mesh without faces
  node, tri, adr, depth = bvh.build_mesh_bvh(np.zeros((0, 3)), [], np.zeros((0, 3)), [], [])
  assert node.shape == (0, 8) and tri.shape == (0,) and adr.shape == (0, 4) and depth == 0
  node, tri, adr, depth = bvh.build_mesh_bvh(vert, [0, 0], face[:3], [0, 0], [0, 3])
  assert adr.tolist() == [[0, 1, 0, 1], [1, 1, 0, 1]] and node.view(np.int32)[:, 7].tolist() == [0, -3]


def test_walk_matches_brute_force(mjm, built):
  """The built trees walked in numpy (exact slabs, ray_ref.triangle in the leaves) give the distance and the face of
  ray_ref.mesh's brute force: on aimed rays, rays parallel to an axis, and origins inside the box."""
  node, tri, adr, _ = built
  rng = np.random.default_rng(5)
  for i in range(int(mjm.nmesh)):
    vert, face = _mesh(mjm, i)
    vert = vert.astype(np.float64)
    lo, hi = vert.min(0), vert.max(0)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    n = 60
    pnt = c + rng.uniform(-4, 4, (n, 3)) * h
    vec = c + rng.uniform(-0.8, 0.8, (n, 3)) * h - pnt
    vec[::3] = np.eye(3)[rng.integers(0, 3, len(vec[::3]))] * rng.choice([-1.0, 1.0], (len(vec[::3]), 1))  # parallel to an axis
    pnt[::3] = c + rng.uniform(-0.7, 0.7, (len(pnt[::3]), 3)) * h - 3 * vec[::3] * h.max()
    pnt[1::6] = c + rng.uniform(-0.9, 0.9, (len(pnt[1::6]), 3)) * h  # inside the box
    pnt[0] = [c[0], c[1], hi[2]]  # on a face of the box, pointing in
    vec[0] = [0.0, 0.0, -1.0]
    aabb = np.concatenate([c, h])
    want_x, want_n = ray_ref.mesh(pnt, vec, vert, face, aabb)
    hits = 0
    for r in range(n):
      x, f = scenes.walk(node, tri, adr, i, vert, face, pnt[r], vec[r], ray_ref.triangle)
      if want_x[r] < 0:
        assert f == -1, (i, r)
        continue
      hits += 1
      every = np.array([ray_ref.triangle(pnt[r : r + 1], vec[r : r + 1], *vert[fc])[0][0] for fc in face])
      every = np.where(every < 0, np.inf, every)
      assert f == int(every.argmin()) and x == every.min(), (i, r)  # the first face of the least distance
      assert abs(x - want_x[r]) <= 1e-12 * max(1.0, x)
      np.testing.assert_allclose(ray_ref.triangle(pnt[r : r + 1], vec[r : r + 1], *vert[face[f]])[1][0], want_n[r], atol=1e-12)
    assert hits >= n // 3, (i, hits)


def test_render_context_carries_the_bvh(mjm, built):
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import bvh

  node, tri, adr, depth = built
  rc = mjw.create_render_context(mjm, nworld=2, cam_res=(4, 3), device="cpu")
  assert rc.mesh_bvh_node.dtype == torch.float32 and rc.mesh_bvh_tri.dtype == torch.int32 and rc.mesh_bvh_adr.dtype == torch.int32
  assert rc.mesh_bvh_node.numpy().tobytes() == node.tobytes()
  assert np.array_equal(rc.mesh_bvh_tri.numpy(), tri) and np.array_equal(rc.mesh_bvh_adr.numpy(), adr)
  assert rc.bvh_leaf_size == bvh.BVH_LEAF == 4 and rc.bvh_max_depth == depth == 8 and rc.bvh_min_faces == bvh.BVH_MIN_FACES == 64
  # a model without meshes gets empty tensors
  bare = _load('<mujoco><worldbody><geom size=".1"/><camera/></worldbody></mujoco>')
  rc = mjw.create_render_context(bare, nworld=1, device="cpu")
  assert tuple(rc.mesh_bvh_node.shape) == (0, 8) and tuple(rc.mesh_bvh_tri.shape) == (0,) and tuple(rc.mesh_bvh_adr.shape) == (0, 4)
  assert rc.bvh_max_depth == 0


def test_rays_rc_refusals(mjm):
  import torch

  import mujoco_warp_amd as mjw
  from tests.ray_scenes import ALL_TYPES_XML

  m = mjw.put_model(mjm, device="cpu")
  d = mjw.make_data(mjm, nworld=2, device="cpu", m=m)
  out = (torch.zeros(2, 1), torch.zeros(2, 1, dtype=torch.int32), torch.zeros(2, 1, 3))
  pnt, vec, excl = torch.zeros(1, 1, 3), torch.ones(1, 1, 3), torch.zeros(1, dtype=torch.int32)
  with pytest.raises(NotImplementedError):
    mjw.rays(m, d, pnt, vec, None, True, excl, *out, rc=object())
  with pytest.raises(NotImplementedError):
    mjw.ray(m, d, pnt, vec, rc=object())
  other = mjw.create_render_context(_load(ALL_TYPES_XML), nworld=2, device="cpu")  # another model: 1 mesh, 4 faces
  with pytest.raises(ValueError, match="meshes"):
    mjw.rays(m, d, pnt, vec, None, True, excl, *out, rc=other)
  with pytest.raises(ValueError, match="meshes"):
    mjw.ray(m, d, pnt, vec, rc=other)
  three = mjw.create_render_context(mjm, nworld=3, device="cpu")
  with pytest.raises(ValueError, match="nworld"):
    mjw.rays(m, d, pnt, vec, None, True, excl, *out, rc=three)
  assert mjw.refit_bvh(m, d, three) is None and "rigid" in mjw.refit_bvh.__doc__


def test_gpu_ray_sets_are_decisive(mjm):
  """The rays tests/test_gpu_bvh.py casts, on the yardstick alone at the host-side frames of each world."""
  from tests.render_scenes import host_frames_all

  aabb = np.asarray(mjm.geom_aabb, dtype=np.float64).reshape(-1, 6)
  total = ok_total = 0
  mesh_first = 0
  for w, qpos in enumerate(scenes.SCENE_QPOS):
    fr = host_frames_all(mjm, qpos)
    for nray in (1, 64, 65, 300):
      pnt, vec = scenes.scene_rays(fr["geom_xpos"], fr["geom_xmat"], aabb, nray, seed=1000 * w + nray)
      pnt, vec = pnt.astype(np.float32).astype(np.float64), vec.astype(np.float32).astype(np.float64)
      g, x, n, ok = ray_ref.cast(mjm, fr["geom_xpos"], fr["geom_xmat"], pnt, vec)
      total, ok_total = total + nray, ok_total + int(ok.sum())
      hit = ok & (g >= 0)
      mesh_first += int((np.asarray(mjm.geom_type)[g[hit]] == ray_ref.MESH).sum())
  print(f"decisive {ok_total} of {total} rays ({ok_total / total:.4f}); {mesh_first} decisive first hits on a mesh")
  assert ok_total / total >= MIN_DECISIVE
  assert mesh_first >= total // 4
