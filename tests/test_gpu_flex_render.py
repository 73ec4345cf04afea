"""Flex rendering on the device (mjw.refit_bvh + mjw.render of a render_flex context; csrc/mjw_flexrender.hip,
mjw_render.hip) against the float64 yardstick tests/flex_render_ref.py.

The vertex positions are written straight into d.flexvert_xpos after one mjw.forward, and the yardstick renders from
what the device holds (those float32 positions, the geom / camera / light frames, the float32 colours), so only the
render code is under test.  The bars are those of tests/test_gpu_render.py: only decisive pixels are compared, at most
2 % of a test's pixels may be non-decisive (each test prints its share), and on decisive pixels the segmentation is
exact, the depth within rtol = atol = 5e-4 and each RGB byte within one level.  Every parity scene has the flex on at
least 10 % of its pixels.  Walk (flex_bvh_min_faces = 0) and face loop (a value above every face count) must agree
bit for bit.
"""

import ctypes

import numpy as np
import pytest

from tests import flex_render_ref as ref
from tests import flex_render_scenes as scenes
from tests import render_ref
from tests.common import np_

pytestmark = pytest.mark.gpu

TOL = 5e-4
MAX_SKIPPED = 0.02
MIN_FLEX = 0.10
SENTINEL = 7
LOOP = 1 << 30  # flex_bvh_min_faces above every face count: the face loop
RES = (33, 17)


def _load(xml):
  from mujoco_warp_amd import mjcf

  return mjcf.load_model_from_string(xml)


def _device(mjm, nworld):
  import torch

  import mujoco_warp_amd as mjw

  m = mjw.put_model(mjm, device="cuda")
  d = mjw.make_data(mjm, nworld=nworld, device="cuda", m=m)
  mjw.forward(m, d)
  torch.cuda.synchronize()
  return m, d


def _rest(mjm):
  from mujoco_warp_amd import bvh

  return bvh.flex_rest_xpos(mjm)


def _set_xpos(d, xs):
  import torch

  xs = np.asarray(xs, dtype=np.float32)
  d.flexvert_xpos[:] = torch.as_tensor(xs.reshape(d.flexvert_xpos.shape), device="cuda")


def _context(mjm, nworld, **kw):
  import mujoco_warp_amd as mjw

  kw.setdefault("cam_res", RES)
  rc = mjw.create_render_context(mjm, nworld=nworld, device="cuda", render_flex=True, render_rgb=True, render_depth=True, render_seg=True, **kw)
  for t in (rc.rgb_data, rc.depth_data, rc.seg_data):
    t.fill_(SENTINEL)
  return rc


def _render(m, d, rc, min_faces=None, refit=True):
  import torch

  import mujoco_warp_amd as mjw

  if min_faces is not None:
    rc.flex_bvh_min_faces = min_faces
  if refit:
    assert mjw.refit_bvh(m, d, rc) is None
  mjw.render(m, d, rc)
  torch.cuda.synchronize()
  return rc.rgb_data.cpu().numpy().copy(), rc.depth_data.cpu().numpy().copy(), rc.seg_data.cpu().numpy().copy()


def _same(a, b, what):
  for x, y, name in zip(a, b, ("rgb", "depth", "seg")):
    assert x.tobytes() == y.tobytes(), f"{what}: {name} differs"


class _Tally:
  def __init__(self):
    self.total = self.skipped = self.flex = 0

  def context(self, mjm, m, d, rc, images, label, smooth=True):
    """Camera 0 of the context in every world against the yardstick; returns {w: (seg, flexid, depth, rgb, ok)}."""
    nw = d.nworld
    gx, gm = np_(d.geom_xpos).reshape(nw, mjm.ngeom, 3), np_(d.geom_xmat).reshape(nw, mjm.ngeom, 3, 3)
    cx, cm = np_(d.cam_xpos).reshape(nw, mjm.ncam, 3), np_(d.cam_xmat).reshape(nw, mjm.ncam, 3, 3)
    lx, ld = np_(d.light_xpos).reshape(nw, mjm.nlight, 3), np_(d.light_xdir).reshape(nw, mjm.nlight, 3)
    fx = np_(d.flexvert_xpos).reshape(nw, mjm.nflexvert, 3)
    rgb_d, depth_d, seg_d = images
    W, H = (int(v) for v in rc.cam_res.cpu().numpy()[0])
    n, out = W * H, {}
    assert rc.rgb_adr.tolist()[0] == 0 and rc.depth_adr.tolist()[0] == 0 and rc.seg_adr.tolist()[0] == 0
    for w in range(nw):
      lab = f"{label}: world {w}"
      seg, fid, depth, rgb, ok = ref.render(
        mjm, gx[w], gm[w], fx[w], cx[w, 0], cm[w, 0], np_(m.cam_fovy).reshape(-1)[0], np_(m.cam_sensorsize).reshape(-1, 2)[0],
        np_(m.cam_intrinsic).reshape(-1, 4)[0], W, H, lx[w], ld[w], rc.light_type.cpu().numpy(), rc.light_active.cpu().numpy(),
        rc.light_castshadow.cpu().numpy(), groups=rc.enabled_geom_groups, use_shadows=rc.use_shadows, smooth=smooth,
        geom_rgba=np_(m.geom_rgba).reshape(-1, 4)[: mjm.ngeom], mat_rgba=np_(m.mat_rgba).reshape(-1, 4), flex_rgba=np_(rc.flex_rgba))
      out[w] = (seg, fid, depth, rgb, ok)
      self.total += n
      self.skipped += int((~ok).sum())
      self.flex += int((seg == -2).sum())
      got = seg_d[w, :n]
      assert np.all((got >= -2) & (got < mjm.ngeom)), f"{lab}: a pixel was not written"
      bad = np.nonzero(ok & (got != seg))[0]
      assert len(bad) == 0, f"{lab}: seg of pixel {bad[0]}: device {got[bad[0]]}, yardstick {seg[bad[0]]}"
      background = got == -1
      gd = depth_d[w, :n].astype(np.float64)
      assert np.isfinite(gd).all()
      np.testing.assert_allclose(gd[ok], depth[ok], rtol=TOL, atol=TOL, err_msg=f"{lab}: depth")
      assert np.all(gd[background] == 0.0) and np.all(gd[ok & (seg != -1)] > 0.0)
      packed = rgb_d[w, :n]
      px = render_ref.unpack(packed)
      assert np.all(px[:, 3] == 255), f"{lab}: alpha must be 255 (or a pixel was not written)"
      diff = np.abs(px[ok, :3] - rgb[ok])
      assert diff.size == 0 or diff.max() <= 1, f"{lab}: an RGB byte is {diff.max()} levels off"
      assert np.all((packed[background].astype(np.int64) & 0xFFFFFFFF) == render_ref.BACKGROUND_PACKED), f"{lab}: background colour"
    return out

  def check(self):
    share, flex = self.skipped / max(self.total, 1), self.flex / max(self.total, 1)
    print(f"skipped {self.skipped} of {self.total} pixels ({share:.4f}); flex on {flex:.3f} of them")
    assert share <= MAX_SKIPPED, f"{self.skipped} of {self.total} pixels are non-decisive"
    assert flex >= MIN_FLEX, f"the flexes cover only {flex:.3f} of the pixels"


# ---- 1. a small sheet, loop and walk, three worlds -----------------------------------------------------------
def test_gpu_flex_sheet_loop_and_walk_per_world():
  from mujoco_warp_amd import bvh

  mjm = _load(scenes.SHEET3_XML)
  nworld = 3
  m, d = _device(mjm, nworld)
  xs = scenes.sheet3_worlds(_rest(mjm))
  assert xs[2, :, 2].min() > xs[:2, :, 2].max() + 0.1  # world 2 lies outside the others' boxes
  _set_xpos(d, xs)
  rc = _context(mjm, nworld)
  assert rc.flex_bvh_min_faces == bvh.FLEX_BVH_MIN_FACES > 32  # 32 faces: the default takes the face loop
  tally = _Tally()
  loop = _render(m, d, rc)
  want = tally.context(mjm, m, d, rc, loop, "loop")
  walk = _render(m, d, rc, min_faces=0)
  tally.context(mjm, m, d, rc, walk, "walk")
  _same(loop, walk, "walk against loop")
  tally.check()
  # the refit is per world: whole-flex boxes and normals differ between the worlds and hold the vertices
  box = rc.flex_node_box.cpu().numpy()[:, -1]
  got = d.flexvert_xpos.cpu().numpy().reshape(nworld, -1, 3)
  r = np.float32(mjm.flex_radius[0])
  np.testing.assert_array_equal(box[:, :3], got.min(axis=1) - r)
  np.testing.assert_array_equal(box[:, 3:], got.max(axis=1) + r)
  assert box[2, 2] > box[:2, 5].max()
  nrm = rc.flexvert_norm.cpu().numpy()
  assert np.abs(nrm[0] - nrm[1]).max() > 0.1 and np.allclose(np.linalg.norm(nrm, axis=2), 1.0, atol=1e-5)
  seen = set(np.concatenate([w[0] for w in want.values()]).tolist())
  assert seen == {-2, -1, 0}, seen


# ---- 2. a deeper tree of unequal halves ----------------------------------------------------------------------
def test_gpu_flex_sheet76_walk_against_yardstick_and_loop():
  mjm = _load(scenes.SHEET76_XML)
  m, d = _device(mjm, 1)
  _set_xpos(d, scenes.saddle(_rest(mjm), 0.35, tilt=0.15)[None])
  rc = _context(mjm, 1)
  info = rc.flex_info.cpu().numpy()
  assert int(info[0, 4]) == 164 and int(info[0, 7]) >= 6
  tally = _Tally()
  walk = _render(m, d, rc, min_faces=0)
  tally.context(mjm, m, d, rc, walk, "walk")
  _same(_render(m, d, rc, min_faces=LOOP), walk, "loop against walk")
  _same(_render(m, d, rc, min_faces=164), walk, "min_faces = the face count walks")
  _same(_render(m, d, rc, min_faces=165), walk, "min_faces = the face count + 1 loops")
  tally.check()
  # every node's box is the exact float32 hull of its faces' points, which lie within radius of the vertices
  box = rc.flex_node_box.cpu().numpy()[0]
  assert np.isfinite(box).all() and np.all(box[:, :3] <= box[:, 3:])
  assert np.all(box[0, :3] >= box[-1, :3] - 1e-6) and np.all(box[0, 3:] <= box[-1, 3:] + 1e-6)  # the root inside the whole-flex box
  ints = rc.flex_bvh_node.cpu().numpy().view(np.int32)[:, 6:8]
  for i, (a, b) in enumerate(ints):
    if b > 0:
      l, r = int(a), int(b) & ((1 << 29) - 1)
      np.testing.assert_array_equal(box[i, :3], np.minimum(box[l, :3], box[r, :3]))
      np.testing.assert_array_equal(box[i, 3:], np.maximum(box[l, 3:], box[r, 3:]))


# ---- 3. smooth and flat normals ------------------------------------------------------------------------------
def test_gpu_flex_render_smooth_and_flat():
  mjm = _load(scenes.SHEET3_XML)
  m, d = _device(mjm, 1)
  _set_xpos(d, scenes.saddle(_rest(mjm), 0.6, tilt=0.2)[None])
  tally, images = _Tally(), {}
  for smooth in (True, False):
    rc = _context(mjm, 1, flex_render_smooth=smooth)
    assert rc.flex_render_smooth is smooth
    images[smooth] = _render(m, d, rc, min_faces=0)
    tally.context(mjm, m, d, rc, images[smooth], f"smooth {smooth}", smooth=smooth)
    _same(_render(m, d, rc, min_faces=LOOP), images[smooth], f"smooth {smooth}: loop against walk")
  tally.check()
  assert (images[True][1] != images[False][1]).mean() > 0.05  # the depth images differ where the sheet is


# ---- 4. ropes, soft bodies, and all three together -----------------------------------------------------------
@pytest.mark.parametrize("name", ["rope", "block", "mixed"])
def test_gpu_flex_rope_block_and_mixed(name):
  mjm = _load({"rope": scenes.ROPE_XML, "block": scenes.BLOCK_XML, "mixed": scenes.MIXED_XML}[name])
  m, d = _device(mjm, 2)
  rest = _rest(mjm)
  _set_xpos(d, np.stack([scenes.wavy(rest), scenes.wavy(rest, -0.1)]))
  rc = _context(mjm, 2)
  tally = _Tally()
  walk = _render(m, d, rc, min_faces=0)
  want = tally.context(mjm, m, d, rc, walk, name)
  _same(_render(m, d, rc, min_faces=LOOP), walk, "loop against walk")
  tally.check()
  if name == "mixed":
    seg, fid, _, _, ok = want[0]
    for f in range(3):  # every flex is the first hit of decisive pixels, in its own colour
      sel = ok & (fid == f)
      assert sel.sum() >= 5, (f, sel.sum())
    px = render_ref.unpack(walk[0][0])[:, :3]
    assert np.all(px[ok & (fid == 0), 0] > px[ok & (fid == 0), 2])  # the sheet is red
    assert np.all(px[ok & (fid == 1), 1] > px[ok & (fid == 1), 2])  # the rope is yellow
    assert np.all(px[ok & (fid == 2), 2] > px[ok & (fid == 2), 1])  # the block is purple


def test_gpu_flex_tie_goes_to_the_lower_flex_id():
  images = []
  for xml in (scenes.TIE_XML, scenes.TIE_FIRST_XML):
    mjm = _load(xml)
    m, d = _device(mjm, 1)
    x = scenes.saddle(_rest(mjm)[:4], 0.3)
    _set_xpos(d, np.concatenate([x] * mjm.nflex)[None])
    rc = _context(mjm, 1)
    images.append(_render(m, d, rc, min_faces=0))
    _same(_render(m, d, rc, min_faces=LOOP), images[-1], "loop against walk")
  _same(images[0], images[1], "two coincident sheets against the first alone")
  assert (images[0][2] == -2).mean() > 0.1


# ---- 5. occlusion both ways ----------------------------------------------------------------------------------
def test_gpu_flex_occlusion_and_one_wave_camera():
  mjm = _load(scenes.OCCLUSION_XML)
  m, d = _device(mjm, 1)
  _set_xpos(d, scenes.saddle(_rest(mjm), 0.3)[None])
  tally = _Tally()
  rc = _context(mjm, 1)
  assert rc.tile_threads == 256
  images = _render(m, d, rc, min_faces=0)
  want = tally.context(mjm, m, d, rc, images, "occlusion")
  seg, _, _, _, ok = want[0]
  ball, slab = mjm.geom_names.index("ball"), mjm.geom_names.index("slab")
  assert set(seg[ok].tolist()) == {-2, -1, 0, ball, slab}
  rc8 = _context(mjm, 1, cam_res=(8, 8))
  assert rc8.tile_threads == 64
  small = _render(m, d, rc8, min_faces=0)
  tally.context(mjm, m, d, rc8, small, "8 x 8")
  _same(_render(m, d, rc8, min_faces=LOOP), small, "8 x 8: loop against walk")
  assert -2 in small[2] and ball in small[2]
  tally.check()


# ---- 6. shadows ----------------------------------------------------------------------------------------------
def test_gpu_flex_shadows():
  mjm = _load(scenes.SHADOW_XML)
  assert list(mjm.light_type) == [1, 0] and all(mjm.light_castshadow)
  m, d = _device(mjm, 1)
  _set_xpos(d, scenes.saddle(_rest(mjm), 0.2)[None])
  tally = _Tally()
  rc_off, rc_on = _context(mjm, 1), _context(mjm, 1, use_shadows=True)
  off, on = _render(m, d, rc_off, min_faces=0), _render(m, d, rc_on, min_faces=0)
  w_off = tally.context(mjm, m, d, rc_off, off, "shadows off")[0]
  w_on = tally.context(mjm, m, d, rc_on, on, "shadows on")[0]
  _same(_render(m, d, rc_on, min_faces=LOOP), on, "shadows: loop against walk")
  tally.check()
  darker = w_on[4] & w_off[4] & (w_on[3].sum(axis=1) < w_off[3].sum(axis=1) - 6)
  on_floor, on_sheet = darker & (w_on[0] == 0), darker & (w_on[0] == -2)
  print("shadowed decisive pixels: floor", on_floor.sum(), "sheet", on_sheet.sum())
  assert on_floor.sum() >= 5 and on_sheet.sum() >= 5  # the sheet shadows the plane, the ball shadows the sheet
  a, b = render_ref.unpack(on[0][0])[:, :3].sum(axis=1), render_ref.unpack(off[0][0])[:, :3].sum(axis=1)
  assert np.all(a[on_floor | on_sheet] < b[on_floor | on_sheet]) and np.all(a <= b)
  np.testing.assert_array_equal(on[2], off[2])


# ---- 7. the refit follows the data ---------------------------------------------------------------------------
def test_gpu_flex_refit_follows_the_data():
  import torch

  import mujoco_warp_amd as mjw

  mjm = _load(scenes.SHEET3_XML)
  m, d = _device(mjm, 1)
  rc = _context(mjm, 1)
  with pytest.raises(ValueError, match="refit_bvh"):
    mjw.render(m, d, rc)
  assert bool((rc.seg_data == SENTINEL).all())
  rest = _rest(mjm)
  tally = _Tally()
  _set_xpos(d, scenes.saddle(rest, 0.4)[None])
  first = _render(m, d, rc, min_faces=0)
  tally.context(mjm, m, d, rc, first, "first")
  _set_xpos(d, scenes.saddle(rest, -0.5, shift=(0.4, -0.1, 0.5), tilt=-0.3)[None])
  stale = _render(m, d, rc, refit=False)  # render does not refit: the old boxes cull the moved sheet
  second = _render(m, d, rc)
  tally.context(mjm, m, d, rc, second, "second")
  tally.check()
  assert (first[2] != second[2]).mean() > 0.03 and stale[2].tobytes() != second[2].tobytes()
  torch.cuda.synchronize()


# ---- 8. degenerate input -------------------------------------------------------------------------------------
def test_gpu_flex_degenerate_input():
  mjm = _load(scenes.DEGENERATE_XML)
  assert [int(x) for x in mjm.flex_dim] == [2, 2, 1] and float(mjm.flex_radius[1]) == 0.0
  m, d = _device(mjm, 1)
  x = scenes.degenerate(mjm, _rest(mjm))
  _set_xpos(d, x[None])
  rc = _context(mjm, 1)
  tally = _Tally()
  walk = _render(m, d, rc, min_faces=0)
  want = tally.context(mjm, m, d, rc, walk, "degenerate")
  _same(_render(m, d, rc, min_faces=LOOP), walk, "loop against walk")
  tally.check()
  assert np.isfinite(rc.flex_node_box.cpu().numpy()).all() and np.isfinite(rc.flexvert_norm.cpu().numpy()).all()
  assert np.isfinite(walk[1]).all()
  fid, ok = want[0][1], want[0][4]
  for f in range(3):
    assert (ok & (fid == f)).sum() >= 5, f


# ---- 9. the towel scene --------------------------------------------------------------------------------------
def test_gpu_flex_aloha_cloth():
  import torch

  import mujoco_warp_amd as mjw
  from tests.cloth_common import aloha_model, aloha_states
  from tests.common import gpu_from_state

  mjm = aloha_model()
  nworld = 2
  m, d = gpu_from_state(mjm, *aloha_states(mjm, nworld, seed=1), njmax=16384, nconmax=4096)
  for _ in range(3):
    mjw.step(m, d)
  torch.cuda.synchronize()
  active = [n == "overhead_cam" for n in mjm.cam_names]
  assert sum(active) == 1
  # groups 0 and 2: the floor, the table and the arms' visual meshes (the camera's own housing, group 1, hides the scene)
  rc = _context(mjm, nworld, cam_active=active, enabled_geom_groups=[0, 2])
  assert int(rc.flex_info.cpu().numpy()[0, 4]) >= rc.flex_bvh_min_faces
  walk = _render(m, d, rc, min_faces=0)
  _same(_render(m, d, rc, min_faces=LOOP), walk, "loop against walk")
  seg = walk[2]
  assert np.all((seg >= -2) & (seg < mjm.ngeom)) and (seg == -2).sum() >= 5 and (seg >= 0).sum() >= 50
  assert np.isfinite(walk[1]).all() and np.all(render_ref.unpack(walk[0])[..., 3] == 255)
  assert walk[1][seg == -2].min() > 0.0


# ---- 10. no flexes: the flag changes nothing -----------------------------------------------------------------
def test_gpu_flex_flag_without_flexes_is_bitwise_the_plain_context():
  import mujoco_warp_amd as mjw

  mjm = _load(scenes.PLAIN_XML)
  m, d = _device(mjm, 2)
  kw = dict(nworld=2, cam_res=RES, render_rgb=True, render_depth=True, render_seg=True, use_shadows=True, device="cuda")
  plain, flagged = mjw.create_render_context(mjm, **kw), mjw.create_render_context(mjm, render_flex=True, **kw)
  a = _render(m, d, plain)
  b = _render(m, d, flagged)
  _same(a, b, "render_flex on a model without flexes")
  assert (a[2] >= 0).sum() > 50


# ---- 11. C ABI refusals --------------------------------------------------------------------------------------
def test_gpu_flex_abi_refusals():
  import torch

  import importlib

  from mujoco_warp_amd import _lib
  from mujoco_warp_amd.forward import _stream
  from mujoco_warp_amd.io import cdata, cmodel
  from mujoco_warp_amd.ray import _ray_model

  render = importlib.import_module("mujoco_warp_amd.render")  # (the package's `render` is the function)
  mjm = _load(scenes.SHEET3_XML)
  m, d = _device(mjm, 1)
  rc = _context(mjm, 1)
  L = _lib.lib()
  assert L.mjw_abi_version() == 36
  fr = render._cflex(rc, m, d, "test")
  cr, bvh, rm = render._crender(rc), render._cbvh(rc, m, d, "test"), _ray_model(m)
  rc.flex_node_box.fill_(SENTINEL)
  assert L.mjw_flex_refit(cmodel(m), cdata(d), None, _stream(d)) == -1 and b"null" in L.mjw_last_error()
  assert L.mjw_render_flex(cmodel(m), cdata(d), ctypes.byref(rm), ctypes.byref(cr), ctypes.byref(bvh), None, _stream(d)) == -1
  for field, value in (("nflexvert", 10), ("nflex", 2), ("nflexelem", 7), ("nflexedge", 3), ("max_depth", 33), ("leaf_size", 5)):
    other = _lib.CFlexRender.from_buffer_copy(fr)
    setattr(other, field, value)
    assert L.mjw_flex_refit(cmodel(m), cdata(d), ctypes.byref(other), _stream(d)) == -4, field
    assert L.mjw_render_flex(cmodel(m), cdata(d), ctypes.byref(rm), ctypes.byref(cr), ctypes.byref(bvh), ctypes.byref(other), _stream(d)) == -4, field
  other = _lib.CFlexRender.from_buffer_copy(fr)
  other.corner = None
  assert L.mjw_flex_refit(cmodel(m), cdata(d), ctypes.byref(other), _stream(d)) == -1
  torch.cuda.synchronize()
  assert bool((rc.flex_node_box == SENTINEL).all()) and bool((rc.seg_data == SENTINEL).all())  # nothing was launched
  # a null bvh is the face loop for the meshes, not an error
  assert L.mjw_flex_refit(cmodel(m), cdata(d), ctypes.byref(fr), _stream(d)) == 0
  assert L.mjw_render_flex(cmodel(m), cdata(d), ctypes.byref(rm), ctypes.byref(cr), None, ctypes.byref(fr), _stream(d)) == 0
  torch.cuda.synchronize()
  assert bool((rc.seg_data != SENTINEL).all())
