"""Textured mjw.render on the device (csrc/mjw_render.hip, mjw_render_tex) against the float64 yardstick
tests/texture_ref.py, on the frames read back from the device.

The bars are those of tests/test_gpu_render.py: on decisive pixels the segmentation is exact, the depth within
atol = rtol = 5e-4 and every RGB byte within one level; at most 2 % of the pixels are skipped; background pixels are
exact.  Images are at most 40 x 24.
"""

import ctypes

import numpy as np
import pytest

from tests import render_ref, render_scenes, texture_ref
from tests import texture_scenes as scenes
from tests.common import np_

pytestmark = pytest.mark.gpu

TOL = 5e-4
MAX_SKIPPED = 0.02
SENTINEL = 7


def _load(xml):
  from mujoco_warp_amd import mjcf

  return mjcf.load_model_from_string(xml)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
  d = tmp_path_factory.mktemp("texture")
  return dict(png=scenes.write_png(d / "t8.png", scenes.TEX8), obj=scenes.uv_sphere_obj(d / "ball.obj"))


def _device(mjm, nworld):
  import torch

  import mujoco_warp_amd as mjw

  m = mjw.put_model(mjm, device="cuda")
  d = mjw.make_data(mjm, nworld=nworld, device="cuda", m=m)
  mjw.forward(m, d)
  torch.cuda.synchronize()
  return m, d


def _context(mjm, nworld, **kw):
  import mujoco_warp_amd as mjw

  kw.setdefault("cam_res", scenes.RES_TILES)
  rc = mjw.create_render_context(mjm, nworld=nworld, device="cuda", render_rgb=True, render_depth=True, render_seg=True, **kw)
  for t in (rc.rgb_data, rc.depth_data, rc.seg_data):
    t.fill_(SENTINEL)
  return rc


def _render(m, d, rc):
  import torch

  import mujoco_warp_amd as mjw

  if getattr(rc, "render_flex", False):
    mjw.refit_bvh(m, d, rc)
  mjw.render(m, d, rc)
  torch.cuda.synchronize()
  return rc.rgb_data.cpu().numpy().copy(), rc.depth_data.cpu().numpy().astype(np.float64), rc.seg_data.cpu().numpy().copy()


def _row(t, w):
  a = np_(t)
  return a[w % a.shape[0]]


def _against_yardstick(mjm, m, d, rc, images, label, textured=True, only_geom=None):
  """Camera 0 of the context in every world against texture_ref on the device's frames; returns {w: yardstick tuple}.
  only_geom: compare only the pixels the device gives to this geom (the flex scene, whose flex the yardstick does not draw)."""
  nw = d.nworld
  fr = dict(geom_xpos=np_(d.geom_xpos).reshape(nw, mjm.ngeom, 3), geom_xmat=np_(d.geom_xmat).reshape(nw, mjm.ngeom, 3, 3),
            cam_xpos=np_(d.cam_xpos).reshape(nw, mjm.ncam, 3), cam_xmat=np_(d.cam_xmat).reshape(nw, mjm.ncam, 3, 3),
            light_xpos=np_(d.light_xpos).reshape(nw, mjm.nlight, 3), light_xdir=np_(d.light_xdir).reshape(nw, mjm.nlight, 3))
  rgb_d, depth_d, seg_d = images
  W, H = (int(v) for v in rc.cam_res.cpu().numpy()[0])
  n = W * H
  out, total, skipped = {}, 0, 0
  for w in range(nw):
    lab = f"{label}: {W} x {H} world {w}"
    args = (mjm, fr["geom_xpos"][w], fr["geom_xmat"][w], fr["cam_xpos"][w, 0], fr["cam_xmat"][w, 0], _row(m.cam_fovy, w)[0],
            _row(m.cam_sensorsize, w).reshape(-1, 2)[0], _row(m.cam_intrinsic, w).reshape(-1, 4)[0], W, H, fr["light_xpos"][w], fr["light_xdir"][w])
    kw = dict(use_shadows=rc.use_shadows, geom_rgba=_row(m.geom_rgba, w), mat_rgba=_row(m.mat_rgba, w), light_type=rc.light_type.cpu().numpy(),
              light_active=rc.light_active.cpu().numpy(), light_castshadow=rc.light_castshadow.cpu().numpy())
    if textured:
      ref = texture_ref.render(*args, mat_texid=_row(m.mat_texid, w), mat_texrepeat=_row(m.mat_texrepeat, w), **kw)
    else:  # the untextured renderer's own yardstick
      ref = render_ref.render(*args, **kw) + (None, None)
    seg, depth, rgb, ok = ref[:4]
    out[w] = ref
    got_seg, got_depth, packed = seg_d[w, :n], depth_d[w, :n], rgb_d[w, :n]
    got = render_ref.unpack(packed)
    assert np.all(got[:, 3] == 255), f"{lab}: alpha must be 255 (or a pixel was not written)"
    if only_geom is not None:
      ok = ok & (got_seg == only_geom)
      assert np.all(seg[ok] == only_geom), f"{lab}: seg"
    else:
      assert np.all((got_seg >= -1) & (got_seg < mjm.ngeom)), f"{lab}: a pixel was not written"
      bad = np.nonzero(ok & (got_seg != seg))[0]
      assert len(bad) == 0, f"{lab}: seg of pixel {bad[0]}: device {got_seg[bad[0]]}, yardstick {seg[bad[0]]}"
      background = got_seg == -1
      assert np.all(got_depth[background] == 0.0), f"{lab}: background depth must be 0"
      assert np.all((packed[background].astype(np.int64) & 0xFFFFFFFF) == render_ref.BACKGROUND_PACKED), f"{lab}: background colour"
      total += n
      skipped += int((~ok).sum())
    np.testing.assert_allclose(got_depth[ok], depth[ok], rtol=TOL, atol=TOL, err_msg=f"{lab}: depth")
    diff = np.abs(got[ok, :3] - rgb[ok])
    print(f"{lab}: {int(ok.sum())} pixels compared, largest RGB difference {diff.max(initial=0)} levels")
    assert diff.size == 0 or diff.max() <= 1, f"{lab}: an RGB byte is {diff.max()} levels off"
  if total:
    print(f"{label}: skipped {skipped} of {total} pixels")
    assert skipped <= MAX_SKIPPED * total, f"{label}: {skipped} of {total} pixels are non-decisive"
  return out


def _same(a, b, what, names=("rgb", "depth", "seg")):
  for x, y, name in zip(a, b, ("rgb", "depth", "seg")):
    if name in names:
      assert x.tobytes() == y.tobytes(), f"{what}: {name} differs"


# ---- 1. textured plane -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [scenes.RES_TILES, scenes.RES_WAVE])
def test_gpu_textured_plane(files, res):
  mjm = _load(scenes.plane_xml(files["png"]))
  m, d = _device(mjm, 1)
  rc = _context(mjm, 1, cam_res=res)
  assert rc.has_textures and rc.tile_threads == (64 if res == scenes.RES_WAVE else 256)
  img = _render(m, d, rc)
  ref = _against_yardstick(mjm, m, d, rc, img, "plane")[0]
  on = ref[0] == 0
  assert on.sum() > 0.3 * res[0] * res[1] and len(np.unique(ref[2][on], axis=0)) > 8  # the texture is in view
  off = _context(mjm, 1, cam_res=res, use_textures=False)
  assert not off.has_textures
  img_off = _render(m, d, off)
  _same(img, img_off, "depth and segmentation with and without textures", names=("depth", "seg"))
  assert img[0].tobytes() != img_off[0].tobytes()


# ---- 2. textured meshes ------------------------------------------------------------------------------------------------
def test_gpu_textured_meshes(files):
  from mujoco_warp_amd.bvh import BVH_MIN_FACES

  mjm = _load(scenes.mesh_xml(files["png"], files["obj"]))
  assert mjm.mesh_facenum.tolist() == [4, 80] and 4 < BVH_MIN_FACES <= 80  # the tetrahedron is looped over, the sphere walked
  m, d = _device(mjm, 1)
  rc = _context(mjm, 1)
  img = _render(m, d, rc)
  ref = _against_yardstick(mjm, m, d, rc, img, "meshes")[0]
  ok, seg, face = ref[3], ref[0], ref[4]
  assert (ok & (seg == 0)).sum() >= 40 and (ok & (seg == 1)).sum() >= 100 and len(np.unique(face[ok & (seg == 1)])) >= 8
  rc.bvh_min_faces = 0
  walk = _render(m, d, rc)
  rc.bvh_min_faces = 10**9
  loop = _render(m, d, rc)
  _same(img, walk, "default against the walk for every mesh")
  _same(img, loop, "default against the face loop for every mesh")
  off = _render(m, d, _context(mjm, 1, use_textures=False))
  _same(img, off, "depth and segmentation with and without textures", names=("depth", "seg"))
  assert img[0].tobytes() != off[0].tobytes()


# ---- 3. geoms that stay untextured -------------------------------------------------------------------------------------
def test_gpu_untextured_geoms_keep_their_colour(files):
  mjm = _load(scenes.untextured_xml(files["png"]))
  m, d = _device(mjm, 1)
  rc = _context(mjm, 1)
  assert rc.has_textures
  img = _render(m, d, rc)
  ref = _against_yardstick(mjm, m, d, rc, img, "untextured geoms")[0]
  assert np.isnan(ref[5]).all() and (np.bincount(ref[0][ref[0] >= 0], minlength=4)[:4] >= 15).all()
  _same(img, _render(m, d, _context(mjm, 1, use_textures=False)), "sphere, box and bare mesh with and without textures")


# ---- 4. per world --------------------------------------------------------------------------------------------------------
def test_gpu_textures_per_world(files):
  import torch

  mjm = _load(scenes.plane_xml(files["png"]))
  nworld = 3
  m, d = _device(mjm, nworld)
  a, b = mjm.tex_names.index("t8"), mjm.tex_names.index("chk")
  texid = -np.ones((3, mjm.nmat, 10), dtype=np.int32)
  texid[:, 0, 1] = (a, b, -1)
  m.mat_texid = torch.as_tensor(texid, device="cuda")
  rep = np.tile(np.asarray(mjm.mat_texrepeat, dtype=np.float32), (2, 1, 1))
  rep[1, 0] = (0.6, 2.5)
  m.mat_texrepeat = torch.as_tensor(rep, device="cuda")
  rgba = np.tile(np.asarray(mjm.mat_rgba, dtype=np.float32), (2, 1, 1))
  rgba[1, 0] = (0.5, 1.0, 0.7, 1.0)
  m.mat_rgba = torch.as_tensor(rgba, device="cuda")
  rc = _context(mjm, nworld)
  img = _render(m, d, rc)
  _against_yardstick(mjm, m, d, rc, img, "per world")
  n = scenes.RES_TILES[0] * scenes.RES_TILES[1]
  assert len({img[0][w, :n].tobytes() for w in range(nworld)}) == 3  # three different pictures
  _same([x[0:1] for x in img], [x[2:3] for x in img], "the geometry of worlds 0 and 2", names=("depth", "seg"))


# ---- 5. shadows ----------------------------------------------------------------------------------------------------------
def test_gpu_textures_with_shadows(files):
  mjm = _load(scenes.shadow_xml(files["png"]))
  m, d = _device(mjm, 1)
  rc = _context(mjm, 1, use_shadows=True)
  img = _render(m, d, rc)
  _against_yardstick(mjm, m, d, rc, img, "shadows")
  lit = _render(m, d, _context(mjm, 1, use_shadows=False))
  assert img[0].tobytes() != lit[0].tobytes()  # the occluder's shadow falls on the textured plane


# ---- 6. a flex context ---------------------------------------------------------------------------------------------------
def test_gpu_textured_floor_under_a_cloth(files):
  mjm = _load(scenes.flex_xml(files["png"]))
  m, d = _device(mjm, 1)
  rc = _context(mjm, 1, render_flex=True)
  assert rc.has_textures and rc.render_flex
  img = _render(m, d, rc)
  floor = 0
  _against_yardstick(mjm, m, d, rc, img, "floor under a cloth", only_geom=floor)
  n = scenes.RES_TILES[0] * scenes.RES_TILES[1]
  seg = img[2][0, :n]
  assert set(np.unique(seg)) == {-2, -1, floor} and (seg == -2).sum() >= 40 and (seg == floor).sum() >= 300
  off = _render(m, d, _context(mjm, 1, render_flex=True, use_textures=False))
  _same(img, off, "depth and segmentation with and without textures", names=("depth", "seg"))
  assert np.array_equal(img[0][0, :n][seg == -2], off[0][0, :n][seg == -2])  # flex pixels keep flex_rgba
  assert not np.array_equal(img[0][0, :n][seg == floor], off[0][0, :n][seg == floor])


# ---- 7. off means off ----------------------------------------------------------------------------------------------------
def test_gpu_use_textures_off_means_off(files):
  import torch

  import mujoco_warp_amd as mjw

  mjm = _load(render_scenes.RENDER_ALL_TYPES_XML)
  nworld = 3
  m = mjw.put_model(mjm, device="cuda")
  d = mjw.make_data(mjm, nworld=nworld, device="cuda", m=m)
  d.qpos[:] = torch.as_tensor(render_scenes.ALL_TYPES_QPOS, dtype=torch.float32, device="cuda")
  mjw.forward(m, d)
  torch.cuda.synchronize()
  kw = dict(cam_res=[(40, 24), (33, 17), (33, 17)])
  on, off = _context(mjm, nworld, **kw), _context(mjm, nworld, use_textures=False, **kw)
  assert not on.has_textures and not off.has_textures
  _same(_render(m, d, on), _render(m, d, off), "a model without textures")
  # the textured scene with use_textures=False is the untextured renderer's picture
  mjm = _load(scenes.plane_xml(files["png"]))
  m, d = _device(mjm, 1)
  rc = _context(mjm, 1, use_textures=False)
  _against_yardstick(mjm, m, d, rc, _render(m, d, rc), "textures off", textured=False)


# ---- 8. the C entry's refusals -------------------------------------------------------------------------------------------
def test_gpu_texture_abi_refusals(files):
  import importlib

  import torch

  from mujoco_warp_amd import _lib
  from mujoco_warp_amd.forward import _stream
  from mujoco_warp_amd.io import cdata, cmodel
  from mujoco_warp_amd.ray import _ray_model

  render = importlib.import_module("mujoco_warp_amd.render")  # (the package's `render` is the function)
  mjm = _load(scenes.plane_xml(files["png"]))
  m, d = _device(mjm, 1)
  rc = _context(mjm, 1)
  L = _lib.lib()
  assert L.mjw_abi_version() == 36 and L.mjw_sizeof_texture() == ctypes.sizeof(_lib.CTexture)
  tex = render._ctex(rc, m, d, "test")
  cr, bvh, rm = render._crender(rc), render._cbvh(rc, m, d, "test"), _ray_model(m)
  call = lambda t: L.mjw_render_tex(cmodel(m), cdata(d), ctypes.byref(rm), ctypes.byref(cr), ctypes.byref(bvh), None, t, _stream(d))
  assert call(None) == -1 and b"null" in L.mjw_last_error()
  for field, value, code in (("tex_data", None, -1), ("tex_adr", None, -1), ("tex_width", None, -1), ("mat_texid", None, -1), ("mat_texrepeat", None, -1),
                             ("ntex", -1, -4), ("ntexdata", -5, -4), ("ntexcoord", -1, -4), ("mat_texid_nb", 0, -4), ("mat_texrepeat_nb", 0, -4),
                             ("nmat", mjm.nmat + 1, -4), ("nmesh", 3, -4), ("nmeshface", 9, -4)):
    other = _lib.CTexture.from_buffer_copy(tex)
    setattr(other, field, value)
    assert call(ctypes.byref(other)) == code, field
  other = _lib.CTexture.from_buffer_copy(tex)
  other.ntexcoord, other.mesh_texcoord = 4, None  # a null table with a non-zero count
  assert call(ctypes.byref(other)) == -1
  torch.cuda.synchronize()
  assert all(bool((t == SENTINEL).all()) for t in (rc.rgb_data, rc.depth_data, rc.seg_data))  # nothing was launched
  assert call(ctypes.byref(tex)) == 0
  torch.cuda.synchronize()
  textured = rc.rgb_data.cpu().numpy().copy()
  assert bool((rc.seg_data != SENTINEL).all())
  # a mat_texid naming texture ntex, and a table shorter than its textures say, render as untextured
  plain = _render(m, d, _context(mjm, 1, use_textures=False))[0]
  assert textured.tobytes() != plain.tobytes()
  ids = m.mat_texid.clone()
  m.mat_texid = ids.clone()
  m.mat_texid[:, :, 1] = int(mjm.ntex)
  assert _render(m, d, rc)[0].tobytes() == plain.tobytes()
  m.mat_texid = ids
  short = _lib.CTexture.from_buffer_copy(tex)
  short.ntexdata = 7  # the 4 x 2 texture no longer fits: it samples nothing
  rc.rgb_data.fill_(SENTINEL)
  assert call(ctypes.byref(short)) == 0
  torch.cuda.synchronize()
  assert rc.rgb_data.cpu().numpy().tobytes() == plain.tobytes()
