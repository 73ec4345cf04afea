"""Flex rendering on the host: the tables create_render_context(render_flex=True) builds (mujoco_warp_amd/bvh.py
build_flex_tables), the library's host face builder against the yardstick tests/flex_render_ref.py, and the refusals.
No GPU is needed: contexts are made on the CPU and nothing is launched."""

import numpy as np
import pytest

from tests import flex_render_ref as ref
from tests import flex_render_scenes as scenes


def _load(xml):
  from mujoco_warp_amd import mjcf

  return mjcf.load_model_from_string(xml)


def _context(mjm, **kw):
  import mujoco_warp_amd as mjw

  return mjw.create_render_context(mjm, cam_res=(8, 4), device="cpu", render_flex=True, **kw)


def _np(t):
  return t.cpu().numpy()


def test_flex_rgba_is_parsed():
  mjm = _load(scenes.EXPLICIT_RGBA_XML)
  assert mjm.flex_rgba.shape == (2, 4)
  np.testing.assert_allclose(mjm.flex_rgba[0], [0.8, 0.3, 0.2, 1.0], rtol=1e-6)
  np.testing.assert_allclose(mjm.flex_rgba[1], [0.5, 0.5, 0.5, 1.0])  # the default
  # an explicit <flex> keeps its rgba too
  bodies = "".join(f'<body name="b{i}" pos="{i % 2} {i // 2} 0"><joint type="slide" axis="0 0 1"/><geom size=".01" mass=".1"/></body>' for i in range(4))
  mjm = _load(f'<mujoco><worldbody>{bodies}</worldbody><deformable><flex name="f" dim="2" body="b0 b1 b2 b3" element="0 1 3 0 3 2" '
              f'rgba=".1 .2 .3 .4"/></deformable></mujoco>')
  np.testing.assert_allclose(mjm.flex_rgba, [[0.1, 0.2, 0.3, 0.4]], rtol=1e-6)


@pytest.mark.parametrize("name, nfaces", [("SHEET3_XML", [32]), ("SHEET76_XML", [164]), ("ROPE_XML", [0]), ("BLOCK_XML", [12]), ("MIXED_XML", [32, 0, 12])])
def test_flex_context_tables(name, nfaces):
  from mujoco_warp_amd import bvh

  mjm = _load(getattr(scenes, name))
  rc = _context(mjm, nworld=2)
  info, corner = _np(rc.flex_info), _np(rc.flex_corner)
  node, tri, level = _np(rc.flex_bvh_node), _np(rc.flex_bvh_tri), _np(rc.flex_bvh_level)
  ints = node.view(np.int32)[:, 6:8]
  inc_adr, inc = _np(rc.flex_inc_adr), _np(rc.flex_inc)
  assert info.shape == (mjm.nflex, 12) and rc.flex_bvh_min_faces == bvh.FLEX_BVH_MIN_FACES
  assert tuple(rc.flex_node_box.shape) == (2, len(node) + mjm.nflex, 6) and tuple(rc.flexvert_norm.shape) == (2, mjm.nflexvert, 3)
  assert corner.shape == (sum(nfaces), 3, 3) and len(tri) == sum(nfaces)
  for f in range(mjm.nflex):
    dim, vertadr, vertnum, faceadr, nface, nodeadr, nnode, depth, leveladr, edgeadr, edgenum = (int(v) for v in info[f, :11])
    assert (dim, vertadr, vertnum) == (mjm.flex_dim[f], mjm.flex_vertadr[f], mjm.flex_vertnum[f])
    assert (edgeadr, edgenum) == (mjm.flex_edgeadr[f], mjm.flex_edgenum[f])
    # face counts by the formulas
    frag = ref.fragments(mjm, f) if dim == 2 else []
    want = {1: 0, 2: 2 * int(mjm.flex_elemnum[f]) + 2 * len(frag), 3: int(mjm.flex_shellnum[f])}[dim]
    assert nface == want == nfaces[f]
    # the fragments are the edges used by exactly one element, in edge order
    got = rc._flex_frag[f] - vertadr
    assert got.tolist() == [list(e) for e in frag]
    if dim == 2:
      assert len(frag) > 0
      c = corner[faceadr : faceadr + nface]
      assert set(np.unique(c[..., 1])) == {-1, 1} and (c[..., 2] == -1).all()  # smooth: vertex normals everywhere
      assert c[..., 0].min() >= vertadr and c[..., 0].max() < vertadr + vertnum
    if dim == 3:
      assert (corner[faceadr : faceadr + nface, :, 1] == 0).all()
    # every face once in the tree's tri
    assert sorted(tri[faceadr : faceadr + nface].tolist()) == list(range(nface))
    # children after parents, leaves of at most BVH_LEAF faces covering tri, depth within the bound
    assert depth <= bvh.depth_bound(nface) and nnode >= 1
    covered = np.zeros(nface, dtype=int)
    for i in range(nnode):
      a, b = int(ints[nodeadr + i, 0]), int(ints[nodeadr + i, 1])
      if b > 0:
        r = b & ((1 << bvh.AXIS_SHIFT) - 1)
        assert i < a < nnode and i < r < nnode
      else:
        assert 0 <= -b <= bvh.BVH_LEAF and 0 <= a <= nface + b
        covered[a : a - b] += 1
    assert (covered == 1).all()
    # level offsets: increasing, from the root to the node count, every child one level below its parent
    lv = level[leveladr : leveladr + depth + 1]
    assert lv[0] == 0 and lv[1] == 1 and lv[-1] == nnode and np.all(np.diff(lv) > 0)
    of = lambda i: int(np.searchsorted(lv, i, side="right")) - 1
    for i in range(nnode):
      a, b = int(ints[nodeadr + i, 0]), int(ints[nodeadr + i, 1])
      if b > 0:
        assert of(a) == of(i) + 1 == of(b & ((1 << bvh.AXIS_SHIFT) - 1))
  # incidence CSR: ascending, and exactly the elements that hold the vertex
  assert len(inc_adr) == mjm.nflexvert + 1 and inc_adr[0] == 0 and inc_adr[-1] == len(inc)
  ev = _np(rc.flex_elem_vert)
  for v in range(mjm.nflexvert):
    mine = inc[inc_adr[v] : inc_adr[v + 1]]
    assert np.all(np.diff(mine) > 0)
    f = int(mjm.flex_vertflexid[v])
    want = [e for e in range(mjm.nflexelem) if mjm.flex_dim[f] == 2 and mjm.flex_elemadr[f] <= e < mjm.flex_elemadr[f] + mjm.flex_elemnum[f] and v in ev[e]]
    assert mine.tolist() == want
  assert sum(nfaces) == 0 or max(int(info[f, 7]) for f in range(mjm.nflex)) == rc.flex_bvh_max_depth


def test_sheet76_tree_is_deep_and_uneven():
  rc = _context(_load(scenes.SHEET76_XML))
  info = _np(rc.flex_info)
  assert int(info[0, 4]) == 164 and int(info[0, 7]) >= 6
  ints = _np(rc.flex_bvh_node).view(np.int32)[:, 6:8]
  counts = sorted({-int(b) for a, b in ints if b <= 0})
  assert len(counts) > 1  # 164 = 82 + 82 = (41 + 41) ...: the halves of 41 are 21 and 20


@pytest.mark.parametrize("smooth", [True, False])
def test_host_face_builder_matches_the_yardstick(smooth):
  from mujoco_warp_amd import bvh

  mjm = _load(scenes.MIXED_XML)
  rest = bvh.flex_rest_xpos(mjm)
  # the rest positions are the flexcomp's grid
  assert np.ptp(rest[:9, 2]) == 0 and abs(np.ptp(rest[:9, 0]) - 1.2) < 1e-12
  rng = np.random.default_rng(3)
  x = scenes.saddle(rest, 0.4, tilt=0.2) + 0.03 * rng.normal(size=rest.shape)
  t = bvh.build_flex_tables(mjm, smooth=smooth)
  vn, en = bvh.flex_vertex_normals(x, t["elem_vert"], t["inc_adr"], t["inc"])
  got = bvh.flex_face_points(t["corner"], t["face_radius"], x, vn, en)
  want = np.concatenate([ref.faces(mjm, f, x, smooth) for f in range(mjm.nflex)], axis=0)
  assert got.shape == want.shape == (44, 3, 3)
  np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)
  np.testing.assert_allclose(vn[:9], ref.vertex_normals(mjm, 0, x[:9]), rtol=0, atol=1e-13)
  if not smooth:
    assert np.abs(got - np.concatenate([ref.faces(mjm, f, x, True) for f in range(mjm.nflex)], axis=0)).max() > 1e-4
    c = t["corner"].reshape(-1, 3, 3)
    assert (c[:16, :, 2] >= 0).all() and (c[16:32, :, 2] == -1).all()  # the fragment faces keep the vertex normals


def test_flat_sheet_faces():
  from mujoco_warp_amd import bvh

  mjm = _load(scenes.SHEET3_XML)
  x = bvh.flex_rest_xpos(mjm)
  assert np.all(x[:, 2] == 0)
  r = float(mjm.flex_radius[0])
  for smooth in (True, False):
    tri = ref.faces(mjm, 0, x, smooth)
    np.testing.assert_allclose(tri[0:16:2, :, 2], r)  # the upper element faces
    np.testing.assert_allclose(tri[1:16:2, :, 2], -r)
    n = np.cross(tri[16:, 1] - tri[16:, 0], tri[16:, 2] - tri[16:, 0])
    assert np.abs(n[:, 2]).max() < 1e-15 and np.linalg.norm(n, axis=1).min() > 0  # the fragment faces are vertical
    t = bvh.build_flex_tables(mjm, smooth=smooth)
    vn, en = bvh.flex_vertex_normals(x, t["elem_vert"], t["inc_adr"], t["inc"])
    np.testing.assert_allclose(bvh.flex_face_points(t["corner"], t["face_radius"], x, vn, en), tri, atol=1e-15)
  # a collapsed element and a vertex whose normals cancel give zero normals, not NaN
  y = x.copy()
  y[1] = y[0]
  vn = ref.vertex_normals(mjm, 0, y)
  assert np.isfinite(vn).all() and np.isfinite(ref.faces(mjm, 0, y)).all()
  t = bvh.build_flex_tables(mjm)
  vn2, en2 = bvh.flex_vertex_normals(y, t["elem_vert"], t["inc_adr"], t["inc"])
  assert np.isfinite(vn2).all() and np.isfinite(en2).all() and (np.linalg.norm(en2, axis=1) == 0).any()
  np.testing.assert_allclose(vn2, vn, atol=1e-15)


def test_render_refuses_a_context_never_refit():
  import mujoco_warp_amd as mjw

  mjm = _load(scenes.SHEET3_XML)
  m = mjw.put_model(mjm, device="cpu")
  d = mjw.make_data(mjm, nworld=2, device="cpu", m=m)
  rc = _context(mjm, nworld=2)
  assert rc.render_flex and rc._flex_refit is False
  with pytest.raises(ValueError, match="refit_bvh"):
    mjw.render(m, d, rc)
  other = _context(_load(scenes.SHEET76_XML), nworld=2)
  with pytest.raises(ValueError, match="flex"):
    mjw.refit_bvh(m, d, other)  # made for another model
  with pytest.raises(ValueError, match="nworld"):
    mjw.refit_bvh(m, d, _context(mjm, nworld=3))


def test_render_flex_changes_nothing_without_flexes():
  import torch

  import mujoco_warp_amd as mjw

  mjm = _load(scenes.PLAIN_XML)
  kw = dict(nworld=2, cam_res=(9, 5), render_depth=True, render_seg=True, use_shadows=True, device="cpu")
  a, b = mjw.create_render_context(mjm, **kw), mjw.create_render_context(mjm, render_flex=True, flex_render_smooth=False, **kw)
  assert a.fields() == b.fields()
  for name in a.fields():
    x, y = getattr(a, name), getattr(b, name)
    assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y, name
  m = mjw.put_model(mjm, device="cpu")
  d = mjw.make_data(mjm, nworld=2, device="cpu", m=m)
  assert mjw.refit_bvh(m, d, b) is None


def test_default_call_still_refuses_a_flex_model():
  import mujoco_warp_amd as mjw

  with pytest.raises(NotImplementedError, match="flex"):
    mjw.create_render_context(_load(scenes.SHEET3_XML), device="cpu")
  with pytest.raises(NotImplementedError, match="render_flex"):
    mjw.create_render_context(_load(scenes.SHEET3_XML), device="cpu", render_flex=False)
