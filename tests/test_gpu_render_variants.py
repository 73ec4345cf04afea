"""The instantiations of the one render kernel (csrc/mjw_render.hip render_kernel<NT, BVH, FLEX, TEX>) that no other
suite launches.

The suites beside this one reach 11 of the 16: everything without flexes and textures (tests/test_gpu_render.py,
test_gpu_bvh.py), flexes with BVH = false at both NT and with BVH, textures and NT = 256 (test_gpu_flex_render.py: its
scenes have no mesh, so the launch has no tree to walk, and its aloha model has textures), textures without flexes
except <64, walk>, and textures with flexes at NT = 256 (test_gpu_texture.py).  Left over:

  NT 256, walk, flex, no textures      NT 64, walk, flex, no textures      NT 64, walk, textures, no flex
  NT 64, loop, flex, textures          NT 64, walk, flex, textures

Each case here renders one scene that has meshes twice: through the context's trees (BVH = true), and with a per-world
batched `m.mesh_vert` of identical rows, for which the launch is the BVH = false kernel (as in
test_gpu_bvh.py::test_gpu_render_bvh).  The two must agree bit for bit in all three outputs, and the walk is held
against the float64 yardsticks at the bars of the neighbouring suites: on decisive pixels the segmentation is exact, the
depth within atol = rtol = 5e-4 and every RGB byte within one level; at most 2 % of the pixels are skipped; background
pixels are exact.  So every case also runs the loop twin of the instantiation it is listed for.

The yardstick of a scene with flexes and textures is put together from the two that exist: tests/flex_render_ref.py
gives segmentation, depth and the colour of flex pixels, tests/texture_ref.py (which draws no flex) the colour of geom
pixels, where it must see the same geom.  No light casts a shadow, so a geom pixel's colour does not depend on the flex.
The CPU test at the end holds every scene's skipped share under the 2 % with the yardsticks alone.
"""

import numpy as np
import pytest

from tests import flex_render_ref, render_ref, render_scenes, texture_ref
from tests import texture_scenes as scenes
from tests.common import np_
from tests.flex_render_scenes import saddle

TOL = 5e-4
MAX_SKIPPED = 0.02
SENTINEL = 7
NWORLD = 2

# (scene, resolution, textures): the instantiations the walk reaches are in the module docstring, in this order
CASES = [("cloth", scenes.RES_TILES, False), ("cloth", scenes.RES_WAVE, False), ("meshes", scenes.RES_WAVE, True), ("cloth", scenes.RES_WAVE, True)]
IDS = ["256-flex", "64-flex", "64-tex", "64-flex-tex"]


def cloth_xml(png, obj):
  """The textured floor under a 3 x 3 cloth of texture_scenes.flex_xml with that module's two textured meshes beside
  the cloth: the tetrahedron (4 faces) and the OBJ sphere (80)."""
  extra = f'<mesh name="tetra" {scenes.TETRA} {scenes.TETRA_UV}/><mesh name="ball" file="{obj}"/>'
  cloth = ('<flexcomp type="grid" name="sheet" dim="2" count="3 3 1" spacing=".5 .5 .1" pos="0.2 0.1 0" radius="0.02" mass="1" rgba=".8 .3 .2 1">'
           '<contact contype="0" conaffinity="0"/></flexcomp>')
  return (f'<mujoco model="variants"><option gravity="0 0 0"/>{scenes._asset(png, extra)}<worldbody><camera name="top" pos="0 0 3" fovy="45"/>{scenes.SUN}'
          '<geom name="floor" type="plane" size="1.9 1.1 .1" pos="0 0 -0.6" material="m8"/>'
          '<geom name="tetra" type="mesh" mesh="tetra" pos="-1.1 -0.3 -0.5" euler="20 30 40" material="m8"/>'
          f'<geom name="ball" type="mesh" mesh="ball" pos="1.0 -0.4 -0.1" euler="15 25 35" material="m8"/>{cloth}</worldbody></mujoco>')


def _model(name, png, obj):
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model_from_string(cloth_xml(png, obj) if name == "cloth" else scenes.mesh_xml(png, obj))
  assert mjm.nmesh == 2 and mjm.mesh_facenum.tolist() == [4, 80]
  return mjm


def _cloth_worlds(mjm):
  """The cloth of each world: two different bends of the rest grid."""
  from mujoco_warp_amd import bvh

  rest = bvh.flex_rest_xpos(mjm)
  return np.stack([saddle(rest, 0.5), saddle(rest, -0.4, tilt=0.3)])


def _yardstick(mjm, rc, fr, fxpos, W, H, textures):
  """seg, depth, rgb, ok of camera 0 in one world with the frames fr (module docstring); fxpos: None without flexes."""
  cam = (fr["cam_xpos"][0], fr["cam_xmat"][0], mjm.cam_fovy[0], np.asarray(mjm.cam_sensorsize).reshape(-1, 2)[0],
         np.asarray(mjm.cam_intrinsic).reshape(-1, 4)[0], W, H, fr["light_xpos"], fr["light_xdir"])
  lights = (np_(rc.light_type), np_(rc.light_active), np_(rc.light_castshadow))
  tseg, tdepth, trgb, tok = texture_ref.render(mjm, fr["geom_xpos"], fr["geom_xmat"], *cam, use_textures=textures, light_type=lights[0],
                                               light_active=lights[1], light_castshadow=lights[2])[:4]
  if fxpos is None:
    return tseg, tdepth, trgb, tok
  seg, _, depth, rgb, ok = flex_render_ref.render(mjm, fr["geom_xpos"], fr["geom_xmat"], fxpos, *cam, *lights)
  geom = seg >= 0
  return seg, depth, np.where(geom[:, None], trgb, rgb), ok & (~geom | (tok & (tseg == seg)))


def _against(images, w, ref, label):
  """World w of the device's images against its yardstick at the bars of the module docstring; returns the pixels skipped."""
  seg, depth, rgb, ok = ref
  n = len(seg)
  packed, got_depth, got_seg = images[0][w, :n], images[1][w, :n].astype(np.float64), images[2][w, :n]
  got = render_ref.unpack(packed)
  assert np.all(got[:, 3] == 255), f"{label}: alpha must be 255 (or a pixel was not written)"
  bad = np.nonzero(ok & (got_seg != seg))[0]
  assert len(bad) == 0, f"{label}: seg of pixel {bad[0]}: device {got_seg[bad[0]]}, yardstick {seg[bad[0]]}"
  background = got_seg == -1
  assert np.all(got_depth[background] == 0.0), f"{label}: background depth must be 0"
  assert np.all((packed[background].astype(np.int64) & 0xFFFFFFFF) == render_ref.BACKGROUND_PACKED), f"{label}: background colour"
  np.testing.assert_allclose(got_depth[ok], depth[ok], rtol=TOL, atol=TOL, err_msg=f"{label}: depth")
  diff = np.abs(got[ok, :3] - rgb[ok])
  print(f"{label}: {int(ok.sum())} of {n} pixels compared, largest RGB difference {diff.max(initial=0)} levels")
  assert diff.size == 0 or diff.max() <= 1, f"{label}: an RGB byte is {diff.max()} levels off"
  return int((~ok).sum())


@pytest.fixture(scope="module")
def files(tmp_path_factory):
  d = tmp_path_factory.mktemp("variants")
  return scenes.write_png(d / "t8.png", scenes.TEX8), scenes.uv_sphere_obj(d / "ball.obj")


@pytest.mark.gpu
@pytest.mark.parametrize("name,res,textures", CASES, ids=IDS)
def test_gpu_render_variant_walk_and_loop(files, name, res, textures):
  import torch

  import mujoco_warp_amd as mjw

  mjm = _model(name, *files)
  flex = name == "cloth"
  m = mjw.put_model(mjm, device="cuda")
  d = mjw.make_data(mjm, nworld=NWORLD, device="cuda", m=m)
  mjw.forward(m, d)
  fxpos = None
  if flex:
    fxpos = _cloth_worlds(mjm)
    d.flexvert_xpos[:] = torch.as_tensor(fxpos.astype(np.float32).reshape(d.flexvert_xpos.shape), device="cuda")
  torch.cuda.synchronize()

  def render():
    rc = mjw.create_render_context(mjm, nworld=NWORLD, device="cuda", cam_res=res, render_rgb=True, render_depth=True, render_seg=True,
                                   render_flex=flex, use_textures=textures)
    assert rc.tile_threads == (64 if res == scenes.RES_WAVE else 256) and rc.has_textures == textures and bool(getattr(rc, "render_flex", False)) == flex
    rc.bvh_min_faces = 0  # the walk takes both meshes through their trees
    for t in (rc.rgb_data, rc.depth_data, rc.seg_data):
      t.fill_(SENTINEL)
    mjw.refit_bvh(m, d, rc)
    mjw.render(m, d, rc)
    torch.cuda.synchronize()
    return rc, (rc.rgb_data.cpu().numpy().copy(), rc.depth_data.cpu().numpy().copy(), rc.seg_data.cpu().numpy().copy())

  rc, walk = render()
  keep = m.mesh_vert
  assert keep.shape[0] == 1
  try:  # identical rows per world: the trees no longer serve the call, the launch is the BVH = false kernel
    m.mesh_vert = keep.repeat(NWORLD, *([1] * (keep.dim() - 1))).contiguous()
    _, loop = render()
  finally:
    m.mesh_vert = keep
  for a, b, what in zip(walk, loop, ("rgb", "depth", "seg")):
    assert a.tobytes() == b.tobytes(), f"{what}: the walk differs from the face loop at {np.nonzero(a != b)}"

  W, H = res
  nw = NWORLD
  fr = dict(geom_xpos=np_(d.geom_xpos).reshape(nw, mjm.ngeom, 3), geom_xmat=np_(d.geom_xmat).reshape(nw, mjm.ngeom, 3, 3),
            cam_xpos=np_(d.cam_xpos).reshape(nw, mjm.ncam, 3), cam_xmat=np_(d.cam_xmat).reshape(nw, mjm.ncam, 3, 3),
            light_xpos=np_(d.light_xpos).reshape(nw, mjm.nlight, 3), light_xdir=np_(d.light_xdir).reshape(nw, mjm.nlight, 3))
  skipped, seen = 0, set()
  for w in range(nw):
    ref = _yardstick(mjm, rc, {k: v[w] for k, v in fr.items()}, np_(d.flexvert_xpos).reshape(nw, -1, 3)[w] if flex else None, W, H, textures)
    skipped += _against(walk, w, ref, f"{name} {W} x {H} textures {textures} world {w}")
    seen |= set(walk[2][w, : W * H].tolist())
  assert skipped <= MAX_SKIPPED * nw * W * H, f"{skipped} of {nw * W * H} pixels are non-decisive"
  assert {1, 2} <= seen if flex else {0, 1} <= seen, seen  # both meshes are in the picture
  assert not flex or -2 in seen


def test_variant_scenes_stay_inside_the_skipped_share(tmp_path):
  """The yardsticks alone, on host frames: every case skips at most 2 % of its pixels, over the two worlds as the GPU
  test counts them, and shows what it is meant to show."""
  import mujoco_warp_amd as mjw

  png, obj = scenes.write_png(tmp_path / "t8.png", scenes.TEX8), scenes.uv_sphere_obj(tmp_path / "ball.obj")
  for name, (W, H), textures in CASES:
    mjm = _model(name, png, obj)
    flex = name == "cloth"
    rc = mjw.create_render_context(mjm, nworld=NWORLD, device="cpu", cam_res=(W, H), render_flex=flex, use_textures=textures)
    fr = render_scenes.host_frames_all(mjm)
    worlds = _cloth_worlds(mjm) if flex else [None] * NWORLD
    skipped, seen = 0, set()
    for fxpos in worlds:
      seg, depth, rgb, ok = _yardstick(mjm, rc, fr, fxpos, W, H, textures)
      skipped += int((~ok).sum())
      seen |= set(seg[ok].tolist())
    print(f"{name} {W} x {H} textures {textures}: {skipped} of {NWORLD * W * H} pixels non-decisive; decisive pixels show {sorted(seen)}")
    assert skipped <= MAX_SKIPPED * NWORLD * W * H
    assert ({-2, 1, 2} if flex else {0, 1}) <= seen


def test_null_tables_are_refused_in_this_order(tmp_path):
  """The C entries refuse a null table their contract requires, after the model pointers and before anything is
  launched (this runs without a GPU).  Pinned: `mjw_render_flex` refuses a null flex table (-1) before it looks into a
  bvh made for another model (-4 when the flex table is there); `mjw_rays_bvh` refuses nray < 0 (-4) before a null bvh."""
  import ctypes
  import importlib

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import _lib
  from mujoco_warp_amd.io import cdata, cmodel
  from mujoco_warp_amd.ray import _ray_model

  render = importlib.import_module("mujoco_warp_amd.render")  # (the package's `render` is the function)
  mjm = _model("cloth", scenes.write_png(tmp_path / "t8.png", scenes.TEX8), scenes.uv_sphere_obj(tmp_path / "ball.obj"))
  m = mjw.put_model(mjm, device="cpu")
  d = mjw.make_data(mjm, nworld=NWORLD, device="cpu", m=m)
  rc = mjw.create_render_context(mjm, nworld=NWORLD, device="cpu", cam_res=scenes.RES_WAVE, render_flex=True)
  L = _lib.lib()
  cm, cd, rm, cr = cmodel(m), cdata(d), _ray_model(m), render._crender(rc)
  bvh, fr, tex = render._cbvh(rc, m, d, "test"), render._cflex(rc, m, d, "test"), render._ctex(rc, m, d, "test")
  head = (cm, cd, ctypes.byref(rm), ctypes.byref(cr))
  foreign = _lib.CBvh.from_buffer_copy(bvh)
  foreign.nmesh += 1

  def refused(code, word, got):
    assert got == code and word in L.mjw_last_error(), (got, L.mjw_last_error())

  refused(-1, b"mjw_render_bvh: null bvh", L.mjw_render_bvh(*head, None, None))
  refused(-1, b"mjw_render_flex: null flex", L.mjw_render_flex(*head, ctypes.byref(bvh), None, None))
  refused(-1, b"mjw_render_flex: null flex", L.mjw_render_flex(*head, ctypes.byref(foreign), None, None))
  refused(-4, b"mjw_render_flex: the bvh", L.mjw_render_flex(*head, ctypes.byref(foreign), ctypes.byref(fr), None))
  refused(-1, b"mjw_render_tex: null texture", L.mjw_render_tex(*head, ctypes.byref(bvh), ctypes.byref(fr), None, None))
  refused(-4, b"mjw_render_tex: the bvh", L.mjw_render_tex(*head, ctypes.byref(foreign), None, ctypes.byref(tex), None))
  refused(-1, b"null model", L.mjw_render_tex(None, cd, ctypes.byref(rm), ctypes.byref(cr), None, None, None, None))
  rays = lambda nray, b: L.mjw_rays_bvh(cm, cd, ctypes.byref(rm), None, 1, None, 1, nray, None, 1, None, None, None, None, b, None)
  refused(-1, b"mjw_rays_bvh: null bvh", rays(4, None))
  refused(-4, b"nray", rays(-1, None))
  refused(-4, b"mjw_rays_bvh: the bvh", rays(4, ctypes.byref(foreign)))
