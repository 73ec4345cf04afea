"""mjw.render on the device (csrc/mjw_render.hip) against the float64 yardstick tests/render_ref.py.

The yardstick renders from the frames the device itself computed (geom, camera and light frames read back after
one mjw.forward) and from the float32 camera parameters and colours of the device model, so only the render
code is under test.  Only decisive pixels are compared (render_ref: the primary ray decisive by ray_ref's
rule and, with shadows, no shadow ray's occlusion changing under the 1e-4 perturbations); every test asserts
that at most 2 % of its pixels are skipped that way.  On decisive pixels the segmentation must match exactly,
the depth to atol = rtol = 5e-4 (the bar of test_gpu_ray.py), and each RGB byte within one level (truncating a
float32 colour can flip at most one level against float64).  Separately, every pixel the device calls
background must be exactly seg -1, depth 0 and the packed background colour.
"""

import os

import numpy as np
import pytest

from tests import render_ref
from tests.common import ROOT, np_
from tests import render_scenes as scenes

pytestmark = pytest.mark.gpu

TOL = 5e-4
MAX_SKIPPED = 0.02
SENTINEL = 7


def _device(mjm, nworld, qpos=None):
  """Model and Data on the device after one forward."""
  import torch

  import mujoco_warp_amd as mjw

  m = mjw.put_model(mjm, device="cuda")
  d = mjw.make_data(mjm, nworld=nworld, device="cuda", m=m)
  if qpos is not None:
    d.qpos[:] = torch.as_tensor(np.asarray(qpos), dtype=torch.float32, device="cuda")
  mjw.forward(m, d)
  torch.cuda.synchronize()
  return m, d


def _frames(mjm, d):
  """The frames the device computed, float64 numpy."""
  nw = d.nworld
  return dict(geom_xpos=np_(d.geom_xpos).reshape(nw, mjm.ngeom, 3), geom_xmat=np_(d.geom_xmat).reshape(nw, mjm.ngeom, 3, 3),
              cam_xpos=np_(d.cam_xpos).reshape(nw, mjm.ncam, 3), cam_xmat=np_(d.cam_xmat).reshape(nw, mjm.ncam, 3, 3),
              light_xpos=np_(d.light_xpos).reshape(nw, mjm.nlight, 3), light_xdir=np_(d.light_xdir).reshape(nw, mjm.nlight, 3))


def _context(mjm, nworld, **kw):
  import mujoco_warp_amd as mjw

  rc = mjw.create_render_context(mjm, nworld=nworld, device="cuda", **kw)
  rc.rgb_data.fill_(SENTINEL)
  rc.depth_data.fill_(SENTINEL)
  rc.seg_data.fill_(SENTINEL)
  return rc


def _render(m, d, rc):
  import torch

  import mujoco_warp_amd as mjw

  mjw.render(m, d, rc)
  torch.cuda.synchronize()
  return rc.rgb_data.cpu().numpy(), rc.depth_data.cpu().numpy().astype(np.float64), rc.seg_data.cpu().numpy()


def _world_row(t, w):
  a = np_(t)
  return a[w % a.shape[0]]


class _Tally:
  """Compares the device's images with the yardstick on decisive pixels and counts the skipped ones."""

  def __init__(self):
    self.total = self.skipped = 0
    self.hits = np.zeros(8, dtype=int)  # decisive first hits per geom type

  def context(self, mjm, m, d, rc, images, label, worlds=None):
    """Every rendered camera of the context in every world; returns {(ci, w): (seg, depth, rgb, ok)} of the yardstick."""
    fr = _frames(mjm, d)
    rgb_d, depth_d, seg_d = images
    res, cams = rc.cam_res.cpu().numpy(), rc.cam_id_map.cpu().numpy()
    adr = [rc.rgb_adr.cpu().numpy(), rc.depth_adr.cpu().numpy(), rc.seg_adr.cpu().numpy()]
    lights = dict(light_type=rc.light_type.cpu().numpy(), light_active=rc.light_active.cpu().numpy(),
                  light_castshadow=rc.light_castshadow.cpu().numpy())
    out = {}
    for ci in range(rc.nrender):
      cadr, dadr, sadr = (int(a[ci]) for a in adr)
      if cadr < 0 and dadr < 0 and sadr < 0:
        continue
      (W, H), cam = (int(v) for v in res[ci]), int(cams[ci])
      n = W * H
      for w in range(d.nworld) if worlds is None else worlds:
        lab = f"{label}: camera {ci} ({W} x {H}) world {w}"
        seg, depth, rgb, ok = render_ref.render(
          mjm, fr["geom_xpos"][w], fr["geom_xmat"][w], fr["cam_xpos"][w, cam], fr["cam_xmat"][w, cam], _world_row(m.cam_fovy, w)[cam],
          _world_row(m.cam_sensorsize, w).reshape(-1, 2)[cam], _world_row(m.cam_intrinsic, w).reshape(-1, 4)[cam], W, H,
          fr["light_xpos"][w], fr["light_xdir"][w], groups=rc.enabled_geom_groups, use_shadows=rc.use_shadows,
          geom_rgba=_world_row(m.geom_rgba, w), mat_rgba=_world_row(m.mat_rgba, w), **lights)
        out[ci, w] = (seg, depth, rgb, ok)
        self.total += n
        self.skipped += int((~ok).sum())
        background = ok & (seg < 0)  # where no device segmentation says so, the yardstick's decisive misses
        if sadr >= 0:
          got = seg_d[w, sadr : sadr + n]
          bad = np.nonzero(ok & (got != seg))[0]
          assert len(bad) == 0, f"{lab}: seg of pixel {bad[0]}: device {got[bad[0]]}, yardstick {seg[bad[0]]}"
          background = got == -1
          assert np.all((got >= -1) & (got < mjm.ngeom)), f"{lab}: a pixel was not written"
        if dadr >= 0:
          got = depth_d[w, dadr : dadr + n]
          np.testing.assert_allclose(got[ok], depth[ok], rtol=TOL, atol=TOL, err_msg=f"{lab}: depth")
          assert np.all(got[background] == 0.0), f"{lab}: background depth must be 0"
          assert np.all(got[ok & (seg >= 0)] > 0.0)
        if cadr >= 0:
          packed = rgb_d[w, cadr : cadr + n]
          got = render_ref.unpack(packed)
          assert np.all(got[:, 3] == 255), f"{lab}: alpha must be 255 (or a pixel was not written)"
          diff = np.abs(got[ok, :3] - rgb[ok])
          assert diff.size == 0 or diff.max() <= 1, f"{lab}: an RGB byte is {diff.max()} levels off"
          assert np.all((packed[background].astype(np.int64) & 0xFFFFFFFF) == render_ref.BACKGROUND_PACKED), f"{lab}: background colour"
        hit = ok & (seg >= 0)
        self.hits += np.bincount(np.asarray(mjm.geom_type)[seg[hit]], minlength=8)
    return out

  def check_skipped(self):
    share = self.skipped / max(self.total, 1)
    print(f"skipped {self.skipped} of {self.total} pixels ({share:.4f})")
    assert share <= MAX_SKIPPED, f"{self.skipped} of {self.total} pixels are non-decisive"


def _load(xml):
  from mujoco_warp_amd import mjcf

  return mjcf.load_model_from_string(xml)


# ---- 1. all geom types -------------------------------------------------------------------------------------
def test_gpu_render_all_types_against_yardstick():
  mjm = _load(scenes.RENDER_ALL_TYPES_XML)
  nworld = 3
  m, d = _device(mjm, nworld, scenes.ALL_TYPES_QPOS)
  rc = _context(mjm, nworld, cam_res=scenes.ALL_TYPES_RES, render_rgb=True, render_depth=True, render_seg=True)
  assert rc.tile_threads == 256 and rc.tile.shape[0] == 4 * 3 + 2 * 3 * 2
  tally = _Tally()
  tally.context(mjm, m, d, rc, _render(m, d, rc), "all types")
  tally.check_skipped()
  print("decisive first hits per geom type", tally.hits)
  assert (tally.hits >= 10).all(), f"a geom type is the first hit of fewer than 10 decisive pixels: {tally.hits}"


# ---- 2. tile edges -----------------------------------------------------------------------------------------
def test_gpu_render_tile_edges():
  mjm = _load(scenes.RENDER_ALL_TYPES_XML)
  nworld = 2
  m, d = _device(mjm, nworld, scenes.ALL_TYPES_QPOS[:nworld])
  tally = _Tally()
  for W, H in ((1, 1), (7, 5), (8, 8), (13, 5), (16, 16), (17, 16), (33, 17)):
    rc = _context(mjm, nworld, cam_res=(W, H), cam_active=[True, False, False], render_rgb=True, render_depth=True, render_seg=True)
    assert rc.tile_threads == (64 if W * H <= 64 else 256)
    assert rc.tile.shape[0] == (1 if W * H <= 64 else -(-W // 16) * -(-H // 16))
    assert tuple(rc.seg_data.shape) == (nworld, W * H)
    tally.context(mjm, m, d, rc, _render(m, d, rc), f"{W} x {H}")
  tally.check_skipped()


# ---- 3. several cameras, flags and offsets -----------------------------------------------------------------
def test_gpu_render_cameras_flags_and_readers():
  import torch

  import mujoco_warp_amd as mjw

  mjm = _load(scenes.RENDER_ALL_TYPES_XML)
  nworld = 2
  m, d = _device(mjm, nworld, scenes.ALL_TYPES_QPOS[:nworld])
  tally = _Tally()
  # a cam_active subset: model cameras 0 and 2 at different resolutions with different outputs
  rc = _context(mjm, nworld, cam_res=[(20, 12), (9, 14)], cam_active=[True, False, True], render_rgb=[True, False], render_depth=[False, True],
                render_seg=[True, True])
  assert rc.cam_id_map.tolist() == [0, 2] and rc.nrender == 2 and rc.total_rays == 240 + 126
  assert rc.rgb_adr.tolist() == [0, -1] and rc.depth_adr.tolist() == [-1, 0] and rc.seg_adr.tolist() == [0, 240]
  assert tuple(rc.rgb_data.shape) == (nworld, 240) and tuple(rc.depth_data.shape) == (nworld, 126) and tuple(rc.seg_data.shape) == (nworld, 366)
  want = tally.context(mjm, m, d, rc, _render(m, d, rc), "subset")
  seg = torch.zeros(nworld, 14, 9, dtype=torch.int32, device="cuda")
  mjw.get_segmentation(rc, 1, seg)
  depth = torch.zeros(nworld, 14, 9, device="cuda")
  mjw.get_depth(rc, 1, 4.0, depth)
  rgb = torch.zeros(nworld, 12, 20, 3, device="cuda")
  mjw.get_rgb(rc, 0, rgb)
  for w in range(nworld):
    s2, d2, _, ok2 = want[1, w]  # model camera 2, not camera 1
    got = seg[w].cpu().numpy().ravel()
    np.testing.assert_array_equal(got[ok2], s2[ok2])
    np.testing.assert_allclose(np_(depth[w]).ravel()[ok2], np.clip(d2[ok2] / 4.0, 0, 1), atol=TOL)
    _, _, c0, ok0 = want[0, w]
    assert np.abs(np_(rgb[w]).reshape(-1, 3)[ok0] * 255.0 - c0[ok0]).max() <= 1.0 + 1e-4
  assert float(rgb.min()) >= 0.0 and float(rgb.max()) <= 1.0
  with pytest.raises(ValueError):
    mjw.get_rgb(rc, 1, torch.zeros(nworld, 14, 9, 3, device="cuda"))  # camera 1 renders no RGB
  with pytest.raises(ValueError):
    mjw.get_depth(rc, 0, 1.0, torch.zeros(nworld, 12, 20, device="cuda"))
  with pytest.raises(ValueError):
    mjw.get_segmentation(rc, 1, torch.zeros(nworld, 9, 14, dtype=torch.int32, device="cuda"))  # H and W swapped
  with pytest.raises(ValueError):
    mjw.get_segmentation(rc, 1, torch.zeros(nworld, 14, 9, device="cuda"))  # dtype
  with pytest.raises(ValueError):
    mjw.get_segmentation(rc, 1, torch.zeros(nworld, 14, 9, dtype=torch.int32))  # device

  # all three cameras, the middle one with every output off: it gets no tiles and nothing of it is written
  rc = _context(mjm, nworld, cam_res=[(18, 10), (300, 200), (10, 6)], render_rgb=[True, False, False], render_depth=[False, False, True],
                render_seg=False)
  assert rc.tile.shape[0] == 2 + 1 and set(rc.tile[:, 0].tolist()) == {0, 2}
  assert rc.rgb_adr.tolist() == [0, -1, -1] and rc.depth_adr.tolist() == [-1, -1, 0] and rc.seg_adr.tolist() == [-1, -1, -1]
  assert tuple(rc.seg_data.shape) == (nworld, 1) and rc.total_rays == 180 + 60000 + 60
  images = _render(m, d, rc)
  assert np.all(images[2] == SENTINEL)  # no segmentation output: its one-element buffer is left alone
  tally.context(mjm, m, d, rc, images, "middle camera off")
  tally.check_skipped()
  # a context without any output renders nothing and is not an error
  rc = _context(mjm, nworld, cam_res=(8, 8), render_rgb=False, render_depth=False, render_seg=False)
  assert rc.tile.shape[0] == 0
  mjw.render(m, d, rc)
  mjw.refit_bvh(m, d, rc)


# ---- 4. a camera on a moving body, and intrinsics ----------------------------------------------------------
def test_gpu_render_body_camera_and_intrinsics():
  mjm = _load(scenes.RIG_XML)
  nworld = 3
  m, d = _device(mjm, nworld, scenes.RIG_QPOS)
  assert float(mjm.cam_sensorsize[1][1]) != 0.0 and float(mjm.cam_sensorsize[0][1]) == 0.0
  fr = _frames(mjm, d)
  assert np.abs(fr["cam_xpos"][1, 0] - scenes.RIG_QPOS[1, 7:10]).max() < 1e-6 and np.abs(fr["cam_xmat"][1, 0] - fr["cam_xmat"][0, 0]).max() > 0.1
  tally = _Tally()
  # the sensor is 4 : 3; 24 x 12 is wider (the sensor's height is cut), 12 x 16 narrower (its width is cut)
  for res in ([(32, 24), (24, 12)], [(17, 9), (12, 16)]):
    rc = _context(mjm, nworld, cam_res=res, render_rgb=True, render_depth=True, render_seg=True)
    tally.context(mjm, m, d, rc, _render(m, d, rc), f"rig {res}")
  tally.check_skipped()
  assert tally.hits[[0, 2, 3, 6]].min() >= 10


# ---- 5. per-world fovy -------------------------------------------------------------------------------------
def test_gpu_render_batched_fovy():
  import torch

  mjm = _load(scenes.RENDER_ALL_TYPES_XML)
  nworld = 3
  m, d = _device(mjm, nworld, scenes.ALL_TYPES_QPOS)
  rc = _context(mjm, nworld, cam_res=(33, 17), cam_active=[True, False, False], render_rgb=False, render_depth=True, render_seg=True)
  same = [a.copy() for a in _render(m, d, rc)]
  fovy = m.cam_fovy.repeat(nworld, 1).contiguous()
  assert tuple(fovy.shape) == (nworld, mjm.ncam)
  fovy[:, 0] = torch.tensor([60.0, 35.0, 80.0], device="cuda")
  m.cam_fovy = fovy
  images = _render(m, d, rc)
  tally = _Tally()
  tally.context(mjm, m, d, rc, images, "batched fovy")
  tally.check_skipped()
  np.testing.assert_array_equal(images[2][0], same[2][0])  # world 0 keeps 60 degrees
  assert (images[2][1] != same[2][1]).mean() > 0.1 and (images[2][2] != same[2][2]).mean() > 0.1


# ---- 6. lights, materials, per-world colours ---------------------------------------------------------------
def test_gpu_render_lights_and_colours():
  mjm = _load(scenes.LIGHTS_XML)
  assert list(mjm.light_type) == [1, 2, 0, 2] and list(mjm.light_active) == [True, True, True, False]
  nworld = 2
  m, d = _device(mjm, nworld)
  rgba = m.geom_rgba.repeat(nworld, 1, 1).contiguous()
  rgba[1, 1, :3] = rgba.new_tensor([0.9, 0.3, 0.6])  # the sphere is another colour in world 1
  m.geom_rgba = rgba
  rc = _context(mjm, nworld, cam_res=(48, 32), render_rgb=True, render_depth=False, render_seg=True)
  images = _render(m, d, rc)
  tally = _Tally()
  want = tally.context(mjm, m, d, rc, images, "lights")
  tally.check_skipped()
  seg, _, rgb, ok = want[0, 0]
  got = render_ref.unpack(images[0][0])[:, :3]
  floor = ok & (seg == 0)
  assert floor.sum() > 100 and np.all(got[floor, 1] < got[floor, 0])  # the material's red, not the geom's own green
  assert len(np.unique(got[floor, 0])) > 20  # the spot's cone and the point light's fall-off shade the floor
  # the spot's cone edge lies inside the image: floor pixels in full cone, on the ramp and outside it
  fr = _frames(mjm, d)
  local = render_ref.pixel_rays(float(mjm.cam_fovy[0]), mjm.cam_sensorsize[0], mjm.cam_intrinsic[0], 48, 32)
  vec = local @ fr["cam_xmat"][0, 0].T
  hitp = fr["cam_xpos"][0, 0] + vec * (want[0, 0][1] / -local[:, 2])[:, None]
  L = fr["light_xpos"][0, 2] - hitp
  cs = -(L / np.linalg.norm(L, axis=1, keepdims=True)) @ (fr["light_xdir"][0, 2] / np.linalg.norm(fr["light_xdir"][0, 2]))
  assert (floor & (cs > 0.95)).sum() >= 10 and (floor & (cs > 0.85) & (cs < 0.95)).sum() >= 10 and (floor & (cs < 0.85)).sum() >= 10
  # world 1's sphere differs, everything else is the same picture
  sphere = images[2][0] == 1
  assert np.array_equal(images[2][1], images[2][0])
  g1 = render_ref.unpack(images[0][1])[:, :3]
  assert np.array_equal(g1[~sphere], got[~sphere]) and (g1[sphere & ok] != got[sphere & ok]).any(axis=1).all()
  # switching the inactive light on changes the picture; switching every light off leaves the ambient term
  rc.light_active[3] = 1
  lit = _render(m, d, rc)
  tally.context(mjm, m, d, rc, lit, "fourth light on")
  assert (lit[0] != images[0]).mean() > 0.2
  rc.light_active[:] = 0
  dark = _render(m, d, rc)
  tally.context(mjm, m, d, rc, dark, "ambient only")
  up = floor  # the floor faces up: 0.5 base amb_hi
  np.testing.assert_array_equal(render_ref.unpack(dark[0][0])[up, :3], np.tile(np.floor(0.5 * np.array([0.3, 0.1, 0.05]) * render_ref.AMB_HI * 255), (up.sum(), 1)))


# ---- 7. shadows --------------------------------------------------------------------------------------------
def test_gpu_render_shadows():
  mjm = _load(scenes.shadow_xml())
  nworld = 2
  m, d = _device(mjm, nworld)
  kw = dict(cam_res=(40, 30), render_rgb=True, render_depth=False, render_seg=True)
  tally = _Tally()
  rc_off, rc_on = _context(mjm, nworld, **kw), _context(mjm, nworld, use_shadows=True, **kw)
  off, on = _render(m, d, rc_off), _render(m, d, rc_on)
  w_off = tally.context(mjm, m, d, rc_off, off, "shadows off")
  w_on = tally.context(mjm, m, d, rc_on, on, "shadows on")
  tally.check_skipped()
  # the yardstick's shadow: decisive floor pixels that are darker with shadows than without (by more than the
  # two levels the byte tolerance of both pictures allows)
  shadowed = w_on[0, 0][3] & w_off[0, 0][3] & (w_on[0, 0][0] == 0) & (w_on[0, 0][2][:, 0] < w_off[0, 0][2][:, 0] - 2)
  assert shadowed.sum() >= 10
  a, b = render_ref.unpack(on[0][0])[:, 0], render_ref.unpack(off[0][0])[:, 0]
  assert np.all(a[shadowed] < b[shadowed]) and np.all(a <= b)
  np.testing.assert_array_equal(on[2], off[2])
  # a light with castshadow="false" throws none, whatever the context says
  mjm2 = _load(scenes.shadow_xml("false"))
  assert list(mjm2.light_castshadow) == [False]
  m2, d2 = _device(mjm2, nworld)
  rc2 = _context(mjm2, nworld, use_shadows=True, **kw)
  no = _render(m2, d2, rc2)
  np.testing.assert_array_equal(no[0], off[0])


# ---- 8. groups and alpha -----------------------------------------------------------------------------------
def test_gpu_render_groups_and_alpha():
  mjm = _load(scenes.GROUPS_XML)
  hidden, ghost = mjm.geom_names.index("hidden"), mjm.geom_names.index("ghost")
  assert mjm.geom_group[hidden] == 3 and mjm.geom_rgba[ghost][3] == 0.0
  nworld = 1
  m, d = _device(mjm, nworld)
  kw = dict(cam_res=(32, 20), render_rgb=True, render_depth=True, render_seg=True)
  tally = _Tally()
  rc = _context(mjm, nworld, **kw)
  images = _render(m, d, rc)
  tally.context(mjm, m, d, rc, images, "default groups")
  ids = set(images[2][0].tolist())
  assert hidden not in ids and ghost in ids and 0 in ids  # group 3 is absent, alpha 0 is drawn all the same
  assert (images[2][0] == ghost).sum() >= 10
  rc = _context(mjm, nworld, enabled_geom_groups=[3], **kw)
  images = _render(m, d, rc)
  tally.context(mjm, m, d, rc, images, "group 3 only")
  assert set(images[2][0].tolist()) == {-1, hidden} and (images[2][0] == hidden).sum() >= 10
  tally.check_skipped()


# ---- 9. more geoms than one LDS chunk ----------------------------------------------------------------------
def test_gpu_render_geom_chunk_edge():
  mjm = _load(scenes.ROW_XML)
  assert mjm.ngeom == scenes.ROW_N + 1 == 130
  nworld = 2
  m, d = _device(mjm, nworld)
  tally = _Tally()
  for shadows in (False, True):  # with shadows the any-hit pass stages both chunks again
    rc = _context(mjm, nworld, cam_res=(40, 24), render_rgb=True, render_depth=True, render_seg=True, use_shadows=shadows)
    images = _render(m, d, rc)
    want = tally.context(mjm, m, d, rc, images, f"row, shadows {shadows}")
    seg, _, _, ok = want[0, 0]
    seen = set(seg[ok & (seg >= 0)].tolist())
    assert 128 in seen and min(seen) < 128, seen  # the last sphere is in the second chunk
    assert (ok & (seg == 128)).sum() >= 10
  tally.check_skipped()


# ---- 10. sparse-path models --------------------------------------------------------------------------------
def test_gpu_render_sparse_models():
  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import types
  from tests.cloth_common import aloha_model

  with pytest.raises(NotImplementedError):
    mjw.create_render_context(aloha_model(), nworld=1, device="cuda")  # flexes would be silently invisible
  # the same scene on the sparse path renders what the dense path renders
  nworld = 2
  kw = dict(cam_res=(33, 17), cam_active=[True, False, False], render_rgb=True, render_depth=True, render_seg=True)
  images = []
  for sparse in (False, True):
    mjm = _load(scenes.RENDER_ALL_TYPES_XML)
    if sparse:
      mjm.opt.jacobian = types.JacobianType.SPARSE
    m, d = _device(mjm, nworld, scenes.ALL_TYPES_QPOS[:nworld])
    assert bool(m.is_sparse) == sparse
    rc = _context(mjm, nworld, **kw)
    images.append(_render(m, d, rc))
    if sparse:
      tally = _Tally()
      tally.context(mjm, m, d, rc, images[-1], "sparse path")
      tally.check_skipped()
  np.testing.assert_array_equal(images[0][2], images[1][2])
  np.testing.assert_allclose(images[0][1], images[1][1], rtol=1e-5, atol=1e-5)


# ---- 11. graph capture -------------------------------------------------------------------------------------
def test_gpu_render_graph_capture():
  import torch

  import mujoco_warp_amd as mjw

  mjm = _load(scenes.RENDER_ALL_TYPES_XML)
  nworld = 3
  m, d = _device(mjm, nworld, scenes.ALL_TYPES_QPOS)
  kw = dict(cam_res=scenes.ALL_TYPES_RES, render_rgb=True, render_depth=True, render_seg=True, use_shadows=True)
  eager, graphed = _context(mjm, nworld, **kw), _context(mjm, nworld, **kw)
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g, stream=s):
    mjw.forward(m, d)
    mjw.render(m, d, graphed)
  torch.cuda.synchronize()
  assert bool((graphed.seg_data == SENTINEL).all())  # capture records, it does not run
  moved = torch.as_tensor(scenes.ALL_TYPES_QPOS[::-1].copy(), dtype=torch.float32, device="cuda")
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
  assert not torch.equal(first, eager.seg_data)  # the ball moved between the replays
  assert int((eager.seg_data >= 0).sum()) > 1000


# ---- 12. mjw.rays after the shared loop was factored out ---------------------------------------------------
def test_gpu_rays_bitwise_as_before_the_shared_loop():
  """tests/golden/render/rays_all_types.npz: mjw.rays on this scene, recorded at the commit before geom_loop
  was factored out of rays_kernel (inputs and outputs)."""
  import torch

  import mujoco_warp_amd as mjw

  gold = np.load(os.path.join(ROOT, "tests", "golden", "render", "rays_all_types.npz"))
  mjm = _load(scenes.RENDER_ALL_TYPES_XML)
  nworld = 3
  m, d = _device(mjm, nworld, scenes.ALL_TYPES_QPOS)
  for nray in (1, 63, 64, 65, 300):
    excl = torch.full((nray,), -1, dtype=torch.int32, device="cuda")
    dist = torch.zeros(nworld, nray, device="cuda")
    gid = torch.zeros(nworld, nray, dtype=torch.int32, device="cuda")
    nrm = torch.zeros(nworld, nray, 3, device="cuda")
    mjw.rays(m, d, torch.as_tensor(gold[f"pnt{nray}"], device="cuda"), torch.as_tensor(gold[f"vec{nray}"], device="cuda"), None, True, excl,
             dist, gid, nrm)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(gid.cpu().numpy(), gold[f"geomid{nray}"])
    assert dist.cpu().numpy().tobytes() == gold[f"dist{nray}"].tobytes()
    assert nrm.cpu().numpy().tobytes() == gold[f"normal{nray}"].tobytes()
  assert sum(int((gold[f"geomid{n}"] >= 0).sum()) for n in (1, 63, 64, 65, 300)) > 1000
