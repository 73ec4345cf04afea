"""CPU tests of the render feature: exports, the <light> attributes, the render context's layout, the refusals,
self-checks of the float64 yardstick tests/render_ref.py, and the share of non-decisive pixels of the scenes and
cameras that tests/test_gpu_render.py renders (on the yardstick alone, from host-side frames)."""

import numpy as np
import pytest

from tests import render_ref
from tests import render_scenes as scenes

MAX_SKIPPED = 0.02


def _load(xml):
  from mujoco_warp_amd import mjcf

  return mjcf.load_model_from_string(xml)


def test_render_names_are_exported():
  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import _lib, types

  for name in ("create_render_context", "render", "get_rgb", "get_depth", "get_segmentation", "refit_bvh", "RenderContext"):
    assert hasattr(mjw, name), name
  assert mjw.RenderContext is types.RenderContext
  assert "mjw_render" in _lib.ENTRY_POINTS and "mjw_render_t" in _lib._H
  import ctypes

  assert ctypes.sizeof(_lib.CRender) == 6 * 4 + 12 * 8 + 3 * 8


def test_light_attributes_and_defaults():
  mjm = _load("""<mujoco><worldbody>
    <light name="a"/>
    <light name="b" directional="true"/>
    <light name="c" type="point" active="false"/>
    <light name="d" type="directional" castshadow="false"/>
    <light name="e" type="spot" directional="true"/>
    <body><freejoint/><geom size=".1"/></body>
  </worldbody></mujoco>""")
  assert list(mjm.light_type) == [0, 1, 2, 1, 0]  # spot 0 (default), directional 1, point 2; `type` wins over `directional`
  assert list(mjm.light_active) == [True, True, False, True, True]
  assert list(mjm.light_castshadow) == [True, True, True, False, True]
  with pytest.raises(NotImplementedError):
    _load('<mujoco><worldbody><light type="image"/><body><freejoint/><geom size=".1"/></body></worldbody></mujoco>')
  import torch

  import mujoco_warp_amd as mjw

  m = mjw.put_model(mjm, device="cpu")
  assert m.light_type.tolist() == [0, 1, 2, 1, 0] and m.light_type.dtype == torch.int32
  assert m.light_active.tolist() == [1, 1, 0, 1, 1] and m.light_castshadow.tolist() == [1, 1, 1, 0, 1]
  rc = mjw.create_render_context(mjm, nworld=2, device="cpu")
  assert rc.nrender == 0 and rc.light_type.tolist() == [0, 1, 2, 1, 0] and rc.light_active.tolist() == [1, 1, 0, 1, 1]


def test_render_context_layout():
  import torch

  import mujoco_warp_amd as mjw

  mjm = _load(scenes.RENDER_ALL_TYPES_XML)
  # defaults: the model's resolutions (1 x 1 here), RGB only (the host model carries no cam_output), groups 0-2
  rc = mjw.create_render_context(mjm, nworld=4, device="cpu")
  assert isinstance(rc, mjw.RenderContext) and rc.nrender == 3 and rc.total_rays == 3
  assert rc.cam_res.tolist() == [[1, 1]] * 3 and rc.cam_id_map.tolist() == [0, 1, 2]
  assert rc.rgb_adr.tolist() == [0, 1, 2] and rc.depth_adr.tolist() == [-1] * 3 and rc.seg_adr.tolist() == [-1] * 3
  assert rc.render_rgb.tolist() == [True] * 3 and rc.render_depth.tolist() == [False] * 3 and rc.render_seg.tolist() == [False] * 3
  assert tuple(rc.rgb_data.shape) == (4, 3) and rc.rgb_data.dtype == torch.int32
  assert tuple(rc.depth_data.shape) == (4, 0) and rc.depth_data.dtype == torch.float32
  assert tuple(rc.seg_data.shape) == (4, 1) and rc.seg_data.dtype == torch.int32
  assert rc.use_shadows is False and rc.enabled_geom_groups == [0, 1, 2] and rc.group_mask == 7
  assert rc.tile_threads == 64 and rc.tile.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0]]
  # a tuple serves every active camera, a list names each; the adr offsets run over the cameras that have the output
  for cam_res in ((20, 10), [(20, 10), (20, 10)]):
    rc = mjw.create_render_context(mjm, nworld=2, cam_res=cam_res, cam_active=[False, True, True], render_rgb=[False, True], render_depth=True,
                                   render_seg=[True, False], use_shadows=True, enabled_geom_groups=[0, 3], device="cpu")
    assert rc.cam_id_map.tolist() == [1, 2] and rc.cam_res.tolist() == [[20, 10], [20, 10]] and rc.total_rays == 400
    assert rc.rgb_adr.tolist() == [-1, 0] and rc.depth_adr.tolist() == [0, 200] and rc.seg_adr.tolist() == [0, -1]
    assert tuple(rc.rgb_data.shape) == (2, 200) and tuple(rc.depth_data.shape) == (2, 400) and tuple(rc.seg_data.shape) == (2, 200)
    assert rc.use_shadows is True and rc.group_mask == 9
    assert rc.tile_threads == 256 and rc.tile.tolist() == [[0, 0, 0, 0], [0, 16, 0, 0], [1, 0, 0, 0], [1, 16, 0, 0]]
  # ignored arguments are accepted
  mjw.create_render_context(mjm, use_textures=False, flex_render_smooth=False, use_precomputed_rays=False, device="cpu")
  # the reference's length assertions
  with pytest.raises(AssertionError):
    mjw.create_render_context(mjm, cam_active=[True, False], device="cpu")
  with pytest.raises(AssertionError):
    mjw.create_render_context(mjm, cam_res=[(4, 4), (4, 4)], device="cpu")
  with pytest.raises(AssertionError):
    mjw.create_render_context(mjm, cam_active=[True, False, True], cam_res=[(4, 4)] * 3, device="cpu")
  with pytest.raises(AssertionError):
    mjw.create_render_context(mjm, render_depth=[True, False], device="cpu")
  with pytest.raises(ValueError):
    mjw.create_render_context(mjm, enabled_geom_groups=[0, 40], device="cpu")
  with pytest.raises(ValueError):
    mjw.create_render_context(mjm, cam_res=(0, 4), device="cpu")


def test_render_refusals():
  import torch

  import mujoco_warp_amd as mjw
  from tests.cloth_common import aloha_model

  with pytest.raises(NotImplementedError, match="flex"):
    mjw.create_render_context(aloha_model(), device="cpu")
  mjm = _load(scenes.RENDER_ALL_TYPES_XML)
  m = mjw.put_model(mjm, device="cpu")
  d = mjw.make_data(mjm, nworld=2, device="cpu", m=m)
  rc = mjw.create_render_context(mjm, nworld=3, cam_res=(4, 3), render_depth=[True, False, False], device="cpu")
  with pytest.raises(ValueError, match="nworld"):
    mjw.render(m, d, rc)  # made for another nworld
  with pytest.raises(ValueError):
    mjw.render(m, d, None)
  other = mjw.create_render_context(_load(scenes.GROUPS_XML), nworld=2, cam_res=(4, 3), device="cpu")
  with pytest.raises(ValueError, match="cameras"):
    mjw.render(m, d, other)  # made for another model
  assert mjw.refit_bvh(m, d, rc) is None
  # readers: an output that is off, a wrong shape, a wrong dtype, a camera that is not there
  with pytest.raises(ValueError, match="does not render seg"):
    mjw.get_segmentation(rc, 0, torch.zeros(3, 3, 4, dtype=torch.int32))
  with pytest.raises(ValueError, match="does not render depth"):
    mjw.get_depth(rc, 1, 1.0, torch.zeros(3, 3, 4))
  with pytest.raises(ValueError):
    mjw.get_depth(rc, 0, 1.0, torch.zeros(3, 4, 3))
  with pytest.raises(ValueError):
    mjw.get_rgb(rc, 0, torch.zeros(3, 3, 4, 3, dtype=torch.float64))
  with pytest.raises(ValueError):
    mjw.get_rgb(rc, 3, torch.zeros(3, 3, 4, 3))
  # and what they compute, on hand-made buffers
  rc.rgb_data[:, 12:24] = (255 << 24 | 255 << 16 | 51 << 8 | 0) - (1 << 32)
  rgb = torch.zeros(3, 3, 4, 3)
  mjw.get_rgb(rc, 1, rgb)
  assert torch.equal(rgb, torch.tensor([1.0, 0.2, 0.0]).expand(3, 3, 4, 3))
  rc.depth_data[:] = torch.arange(12, dtype=torch.float32)
  depth = torch.zeros(3, 3, 4)
  mjw.get_depth(rc, 0, 8.0, depth)
  np.testing.assert_allclose(depth[1].numpy(), np.clip(np.arange(12).reshape(3, 4) / 8.0, 0, 1))


# ---- the yardstick's own checks ------------------------------------------------------------------------------
def test_yardstick_centre_pixel_looks_along_minus_z():
  for W, H in ((1, 1), (5, 3), (33, 17)):
    local = render_ref.pixel_rays(60.0, [0.0, 0.0], [0.01, 0.01, 0, 0], W, H)
    np.testing.assert_allclose(local[(H // 2) * W + W // 2], [0, 0, -1], atol=1e-15)
    np.testing.assert_allclose(np.linalg.norm(local, axis=1), 1.0)
  # the corners of a 2 x 2 image sit at half the half-extents: fovy 90 -> y = +-0.5, x = +-0.5 W / H
  local = render_ref.pixel_rays(90.0, [0.0, 0.0], [0, 0, 0, 0], 2, 2)
  np.testing.assert_allclose(local[0] / -local[0, 2], [-0.5, 0.5, -1.0])  # pixel (0, 0) is up and to the left
  # intrinsics: a centred principal point and a sensor of the image's aspect give x in +-sw / 2 fx
  local = render_ref.pixel_rays(0.0, [0.02, 0.01], [0.01, 0.01, 0, 0], 2, 1)
  np.testing.assert_allclose(local[:, 0] / -local[:, 2], [-0.5, 0.5])
  # a wider image than the sensor cuts the sensor's height, a narrower one its width
  wide = render_ref.pixel_rays(0.0, [0.02, 0.02], [0.01, 0.01, 0, 0], 4, 2)
  assert abs(wide[0, 0] / -wide[0, 2] + 0.75) < 1e-12 and abs(wide[0, 1] / -wide[0, 2] - 0.25) < 1e-12
  tall = render_ref.pixel_rays(0.0, [0.02, 0.02], [0.01, 0.01, 0, 0], 2, 4)
  assert abs(tall[0, 0] / -tall[0, 2] + 0.25) < 1e-12 and abs(tall[0, 1] / -tall[0, 2] - 0.75) < 1e-12


_SIMPLE = """<mujoco><worldbody>
  <geom type="plane" size="5 5 1" rgba="0.6 0.4 0.2 1"/>
  <geom type="sphere" size="0.5" pos="0 0 3" rgba="1 1 1 1"/>
  <camera name="down" pos="0 0 6" fovy="40"/>
  <camera name="floor" pos="2 2 4" fovy="20"/>
  <light type="point" pos="2 2 5" dir="0 0 -1" castshadow="false"/>
  <body pos="4 4 1"><freejoint/><geom size=".1"/></body>
</worldbody></mujoco>"""


def test_yardstick_depth_and_shading():
  mjm = _load(_SIMPLE)
  fr = scenes.host_frames_all(mjm)
  args = lambda cam: (mjm, fr["geom_xpos"], fr["geom_xmat"], fr["cam_xpos"][cam], fr["cam_xmat"][cam], 40.0 if cam == 0 else 20.0, [0, 0], [0, 0, 0, 0], 3, 3,
                      fr["light_xpos"], fr["light_xdir"])
  # the sphere straight ahead of the centre pixel: depth = distance - radius
  seg, depth, rgb, ok = render_ref.render(*args(0))
  assert seg[4] == 1 and abs(depth[4] - 2.5) < 1e-12 and ok[4]
  # the up-facing plane with the light off: 0.5 base amb_hi
  seg, depth, rgb, ok = render_ref.render(*args(1), light_active=[False])
  assert seg[4] == 0 and abs(depth[4] - 4.0) < 1e-12
  base = np.array([0.6, 0.4, 0.2])
  np.testing.assert_array_equal(rgb[4], np.floor(0.5 * base * render_ref.AMB_HI * 255))
  # the point light straight above the pixel's hit (r = 5) adds base / (1 + 0.02 r^2)
  seg, depth, rgb, ok = render_ref.render(*args(1))
  np.testing.assert_array_equal(rgb[4], np.floor((0.5 * base * render_ref.AMB_HI + base / 1.5) * 255))
  # a miss is background
  mjm.geom_group[:] = 5
  seg, depth, rgb, ok = render_ref.render(*args(0))
  assert np.all(seg == -1) and np.all(depth == 0) and np.all(rgb == render_ref.BACKGROUND) and ok.all()
  assert render_ref.unpack(np.array([render_ref.BACKGROUND_PACKED - (1 << 32)], dtype=np.int64).astype(np.int32)).tolist() == [[25, 25, 51, 255]]


# ---- the non-decisive share of what the GPU tests render --------------------------------------------------------
def _share(mjm, qpos, views, **kw):
  """views: (camera, W, H) list; qpos: (nworld, nq) or None.  Returns total, skipped and the decisive hits per geom type."""
  total = skipped = 0
  hits = np.zeros(8, dtype=int)
  for q in [None] if qpos is None else qpos:
    fr = scenes.host_frames_all(mjm, q)
    for cam, W, H in views:
      seg, _, _, ok = render_ref.render(mjm, fr["geom_xpos"], fr["geom_xmat"], fr["cam_xpos"][cam], fr["cam_xmat"][cam], mjm.cam_fovy[cam],
                                        mjm.cam_sensorsize[cam], mjm.cam_intrinsic[cam], W, H, fr["light_xpos"], fr["light_xdir"], **kw)
      total += W * H
      skipped += int((~ok).sum())
      hit = ok & (seg >= 0)
      hits += np.bincount(np.asarray(mjm.geom_type)[seg[hit]], minlength=8)
  return total, skipped, hits


GPU_VIEWS = {
  "all types": (scenes.RENDER_ALL_TYPES_XML, scenes.ALL_TYPES_QPOS, [(c, w, h) for c, (w, h) in enumerate(scenes.ALL_TYPES_RES)], {}),
  "tile edges": (scenes.RENDER_ALL_TYPES_XML, scenes.ALL_TYPES_QPOS[:2], [(0, w, h) for w, h in ((1, 1), (7, 5), (8, 8), (13, 5), (16, 16), (17, 16), (33, 17))], {}),
  "rig": (scenes.RIG_XML, scenes.RIG_QPOS, [(0, 32, 24), (1, 24, 12), (0, 17, 9), (1, 12, 16)], {}),
  "lights": (scenes.LIGHTS_XML, None, [(0, 48, 32)], {}),
  "shadows": (scenes.shadow_xml(), None, [(0, 40, 30)], dict(use_shadows=True)),
  "groups": (scenes.GROUPS_XML, None, [(0, 32, 20)], {}),
  "row": (scenes.ROW_XML, None, [(0, 40, 24)], dict(use_shadows=True)),
}


@pytest.mark.parametrize("name", list(GPU_VIEWS))
def test_gpu_scenes_are_decisive(name):
  xml, qpos, views, kw = GPU_VIEWS[name]
  mjm = _load(xml)
  total, skipped, hits = _share(mjm, qpos, views, **kw)
  print(f"{name}: skipped {skipped} of {total} pixels ({skipped / total:.4f}); decisive first hits per geom type {hits}")
  assert skipped / total <= MAX_SKIPPED
  if name == "all types":
    assert (hits >= 10).all(), hits
  if name == "row":
    fr = scenes.host_frames_all(mjm)
    seg, _, _, ok = render_ref.render(mjm, fr["geom_xpos"], fr["geom_xmat"], fr["cam_xpos"][0], fr["cam_xmat"][0], mjm.cam_fovy[0], [0, 0], [0] * 4, 40, 24,
                                      fr["light_xpos"], fr["light_xdir"])
    assert (ok & (seg == 128)).sum() >= 10 and (ok & (seg >= 0) & (seg < 128)).sum() >= 10
