"""Textured rendering on the host: what the MJCF compiler keeps of <texture>, <material> and mesh texture coordinates,
the tables create_render_context packs, the float64 yardstick tests/texture_ref.py, and the share of non-decisive
pixels of every scene and resolution tests/test_gpu_texture.py renders."""

import os

import numpy as np
import pytest

from tests import render_scenes, texture_ref
from tests import texture_scenes as scenes
from tests.common import ROOT


def _load(xml):
  from mujoco_warp_amd import mjcf

  return mjcf.load_model_from_string(xml)


def _tex(mjm, name):
  return texture_ref.texture(mjm, mjm.tex_names.index(name))


def _model(asset, world=""):
  return _load(f"<mujoco><asset>{asset}</asset><worldbody>{world}<body><freejoint/><geom size=\".1\"/></body></worldbody></mujoco>")


# ---- 1. compiler: builtin and PNG data ---------------------------------------------------------------------------------
def test_builtin_texture_bytes():
  mjm = _model('<texture name="chk" type="2d" builtin="checker" width="4" height="2" rgb1="1 0.5 0" rgb2="0 0.2 1"/>'
               '<texture name="flat" type="2d" builtin="flat" width="3" height="2" rgb1="0.3 0.6 0.9" rgb2="1 1 1"/>'
               '<texture name="edge" type="2d" builtin="flat" width="4" height="3" rgb1="0 0 0" mark="edge" markrgb="1 0 0.5"/>'
               '<texture name="cross" type="2d" builtin="flat" width="4" height="3" rgb1="0 0 0" mark="cross" markrgb="0 1 0" random="0.1"/>'
               '<texture name="noise" type="2d" builtin="flat" width="2" height="2" rgb1="0.5 0.5 0.5" mark="random" random="0.5"/>')
  assert mjm.ntex == 5 and mjm.tex_names == ["chk", "flat", "edge", "cross", "noise"]
  assert list(mjm.tex_type) == [0] * 5 and list(mjm.tex_nchannel) == [3] * 5
  assert list(mjm.tex_width) == [4, 3, 4, 4, 2] and list(mjm.tex_height) == [2, 2, 3, 3, 2]
  assert mjm.tex_data.dtype == np.uint8 and mjm.ntexdata == len(mjm.tex_data) == 3 * (8 + 6 + 12 + 12 + 4)
  assert list(mjm.tex_adr) == [0, 24, 42, 78, 114]
  a, b = [255, 128, 0], [0, 51, 255]  # floor(c * 255 + 0.5)
  assert _tex(mjm, "chk").tolist() == [[a, a, b, b], [b, b, a, a]]  # (r < 1) == (c < 2) is rgb1
  assert _tex(mjm, "flat").tolist() == [[[77, 153, 230]] * 3] * 2
  m, z = [255, 0, 128], [0, 0, 0]
  assert _tex(mjm, "edge").tolist() == [[m, m, m, m], [m, z, z, m], [m, m, m, m]]
  g = [0, 255, 0]
  assert _tex(mjm, "cross").tolist() == [[z, z, g, z], [g, g, g, g], [z, z, g, z]]  # row 3 // 2, column 4 // 2
  assert _tex(mjm, "noise").tolist() == [[[128, 128, 128]] * 2] * 2  # the noise is left out


def test_png_textures(tmp_path):
  rgb = np.arange(18, dtype=np.uint8).reshape(2, 3, 3) * 13
  grey = np.array([[0, 100], [200, 255]], dtype=np.uint8)
  rgba = np.concatenate([rgb, np.full((2, 3, 1), 77, dtype=np.uint8)], axis=2)
  deep = (rgb.astype(np.uint16) << 8) | 0x5A
  ga = np.stack([grey, 255 - grey], axis=2)
  p = {k: scenes.write_png(tmp_path / f"{k}.png", v, depth) for k, v, depth in (("rgb", rgb, 8), ("grey", grey, 8), ("rgba", rgba, 8), ("deep", deep, 16),
                                                                               ("ga", ga, 8))}
  mjm = _model("".join(f'<texture name="{k}" type="2d" file="{v}"/>' for k, v in p.items())
               + f'<texture name="h" type="2d" file="{p["rgb"]}" hflip="true"/><texture name="v" type="2d" file="{p["rgb"]}" vflip="true"/>'
               + f'<texture name="hv" type="2d" file="{p["rgba"]}" hflip="true" vflip="true"/>')
  assert list(mjm.tex_width) == [3, 2, 3, 3, 2, 3, 3, 3] and list(mjm.tex_height) == [2] * 8
  assert np.array_equal(_tex(mjm, "rgb"), rgb)  # rows in file order
  assert np.array_equal(_tex(mjm, "grey"), np.repeat(grey[:, :, None], 3, axis=2))
  assert np.array_equal(_tex(mjm, "rgba"), rgb)  # alpha dropped
  assert np.array_equal(_tex(mjm, "deep"), rgb)  # the high byte
  assert np.array_equal(_tex(mjm, "ga"), np.repeat(grey[:, :, None], 3, axis=2))
  assert np.array_equal(_tex(mjm, "h"), rgb[:, ::-1]) and np.array_equal(_tex(mjm, "v"), rgb[::-1]) and np.array_equal(_tex(mjm, "hv"), rgb[::-1, ::-1])


def test_texturedir_and_assetdir(tmp_path):
  from mujoco_warp_amd import mjcf

  os.makedirs(tmp_path / "img")
  scenes.write_png(tmp_path / "img" / "t.png", scenes.TEX8)
  for attr in ("texturedir", "assetdir"):
    xml = tmp_path / f"{attr}.xml"
    xml.write_text(f'<mujoco><compiler {attr}="img"/><asset><texture type="2d" file="t.png"/></asset><worldbody><body><freejoint/><geom size=".1"/>'
                   '</body></worldbody></mujoco>')
    mjm = mjcf.load_model(str(xml))
    assert mjm.tex_names == ["t"] and np.array_equal(texture_ref.texture(mjm, 0), scenes.TEX8)


def test_cube_and_skybox_recorded_without_data(tmp_path):
  jpg = tmp_path / "x.jpg"
  jpg.write_bytes(b"not an image")
  asset = ('<texture name="c" type="cube" builtin="flat" width="8" height="8" rgb1="1 0 0"/>'
           '<texture type="skybox" builtin="gradient" width="4" height="24" rgb1="1 1 1" rgb2="0 0 0"/>'
           '<texture name="g" type="2d" builtin="gradient" width="2" height="3" rgb1="1 1 1" rgb2="0 0 0"/>'
           f'<texture name="j" type="2d" file="{jpg}"/><material name="ok" texture="c"/>')
  mjm = _model(asset)
  assert list(mjm.tex_type) == [1, 2, 0, 0] and list(mjm.tex_adr) == [-1, -1, 0, -1] and mjm.ntexdata == 18
  assert _tex(mjm, "g")[:, 0, 0].tolist() == [255, 128, 0]  # this build's gradient: rgb1 at row 0 to rgb2 at the last row
  assert texture_ref.texture(mjm, 0) is None and texture_ref.texture(mjm, 3) is None
  with pytest.raises(NotImplementedError):  # another file type is refused only when a material uses it
    _model(asset + '<material name="bad" texture="j"/>')


# ---- 2. compiler: materials ----------------------------------------------------------------------------------------------
def test_material_texture_fields():
  mjm = _model('<texture name="a" type="2d" builtin="flat" width="2" height="2"/><texture name="b" type="2d" builtin="checker" width="2" height="2"/>'
               '<material name="none" rgba="1 0 0 1"/><material name="ma" texture="a"/>'
               '<material name="mb" texture="b" texrepeat="3 0.5" texuniform="true"/>'
               '<material name="layered"><layer role="rgb" texture="b"/></material>')
  assert mjm.nmat == 4 and mjm.mat_texid.shape == (4, 10) and mjm.mat_texid.dtype == np.int32
  assert mjm.mat_texid[:, 1].tolist() == [-1, 0, 1, 1]
  assert np.all(np.delete(mjm.mat_texid, 1, axis=1) == -1)
  assert mjm.mat_texrepeat.tolist() == [[1, 1], [1, 1], [3, 0.5], [1, 1]]
  assert mjm.mat_texuniform.tolist() == [False, False, True, False]
  with pytest.raises(ValueError, match="unknown texture"):
    _model('<material name="m" texture="nowhere"/>')


# ---- 3. compiler: meshes -------------------------------------------------------------------------------------------------
_OBJ = """v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0.5 0.5 1
vt 0 0
vt 1 0
vt 1 1
vt 0 1
vt 0.5 0.25
vn 0 0 1
f 1/1 2/2 3/3 4/4
f 1/1/1 2/2/1 5/5/1
f -4/-4 -3/-3 -1/-1
f 3/3 4/4 5/5
f 4/4 1/1 5/5
"""


def test_obj_texcoords(tmp_path):
  path = tmp_path / "pyr.obj"
  path.write_text(_OBJ)
  mjm = _model(f'<mesh name="pyr" file="{path}"/>')
  assert mjm.mesh_facenum.tolist() == [6] and mjm.ntexcoord == 5 and mjm.mesh_texcoordadr.tolist() == [0] and mjm.mesh_texcoordnum.tolist() == [5]
  assert mjm.mesh_texcoord.tolist() == [[0, 1], [1, 1], [1, 0], [0, 0], [0.5, 0.75]]  # (u, 1 - v)
  want = [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]]  # the quad fanned; negative indices from the end
  assert mjm.mesh_facetexcoord.tolist() == want and mjm.mesh_face.tolist() == want and mjm.mesh_facetexcoord.dtype == np.int32
  # one corner without vt: the mesh has no texcoords
  (tmp_path / "part.obj").write_text(_OBJ.replace("f 3/3 4/4 5/5", "f 3/3 4 5/5"))
  (tmp_path / "vn.obj").write_text(_OBJ.replace("f 3/3 4/4 5/5", "f 3//1 4//1 5//1"))
  for name in ("part", "vn"):
    bare = _model(f'<mesh name="pyr" file="{tmp_path / (name + ".obj")}"/>')
    assert bare.mesh_texcoordadr.tolist() == [-1] and bare.ntexcoord == 0 and bare.mesh_texcoord.shape == (0, 2)
    assert bare.mesh_face.tolist() == want and bare.mesh_facetexcoord.shape == (6, 3)


def test_inline_texcoord_survives_the_vertex_remap():
  # vertex 4 repeats vertex 1: the remap renames it in mesh_face and leaves the texcoord indices alone
  mjm = _model('<mesh name="a" vertex="0 0 0  1 0 0  0 1 0  0 0 1  1 0 0" face="0 2 1  0 4 3  1 2 3  0 3 2" '
               'texcoord="0 0  1 0  0 1  0.5 0.5  0.9 0.1"/><mesh name="b" vertex="0 0 0  1 0 0  0 1 0  0 0 1" face="0 2 1  0 1 3  1 2 3  0 3 2"/>')
  assert mjm.mesh_vertnum.tolist() == [4, 4] and mjm.mesh_face[:4].tolist() == [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]
  assert mjm.mesh_facetexcoord.tolist() == [[0, 2, 1], [0, 4, 3], [1, 2, 3], [0, 3, 2]] + [[0, 0, 0]] * 4
  assert mjm.mesh_texcoordadr.tolist() == [0, -1] and mjm.mesh_texcoordnum.tolist() == [5, 0]
  assert mjm.mesh_texcoord.tolist() == [[0, 0], [1, 0], [0, 1], [0.5, 0.5], [0.9, 0.1]]


def test_stl_has_no_texcoords(tmp_path):
  tri = "solid s\n" + "".join(f"facet normal 0 0 1\nouter loop\nvertex {a}\nvertex {b}\nvertex {c}\nendloop\nendfacet\n" for a, b, c in (
    ("0 0 0", "0 1 0", "1 0 0"), ("0 0 0", "1 0 0", "0 0 1"), ("1 0 0", "0 1 0", "0 0 1"), ("0 0 0", "0 0 1", "0 1 0"))) + "endsolid s\n"
  (tmp_path / "t.stl").write_text(tri)
  mjm = _model(f'<mesh name="t" file="{tmp_path / "t.stl"}"/>')
  assert mjm.mesh_texcoordadr.tolist() == [-1] and mjm.ntexcoord == 0


# ---- 4. the benchmark scenes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["models/humanoid.xml", "models/apptronik_apollo/scene_flat.xml"])
def test_benchmark_scene_floor_is_a_checker(path):
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model(os.path.join(ROOT, path))
  floor = [g for g in range(mjm.ngeom) if int(mjm.geom_type[g]) == 0]
  assert floor
  mat = int(mjm.geom_matid[floor[0]])
  tid = int(mjm.mat_texid[mat, 1])
  assert mjm.tex_names[tid] == "grid" and int(mjm.tex_type[tid]) == 0
  tex = texture_ref.texture(mjm, tid)
  assert tex.shape == (512, 512, 3) and tex[0, 0].tolist() == [26, 51, 77] and tex[0, 511].tolist() == [51, 77, 102] and tex[511, 511].tolist() == [26, 51, 77]
  if "humanoid" in path:
    body = mjm.tex_names.index("body")
    assert int(mjm.tex_type[body]) == 1 and int(mjm.tex_adr[body]) == -1 and texture_ref.texture(mjm, body) is None


# ---- 5. the context on the host ------------------------------------------------------------------------------------------
def test_context_tables(tmp_path):
  import torch

  import mujoco_warp_amd as mjw

  png = scenes.write_png(tmp_path / "t8.png", scenes.TEX8)
  obj = scenes.uv_sphere_obj(tmp_path / "ball.obj")
  mjm = _load(scenes.mesh_xml(png, obj))
  rc = mjw.create_render_context(mjm, cam_res=(4, 3), device="cpu")
  assert rc.has_textures and rc.use_textures
  assert mjm.tex_names == ["t8", "chk", "sky"]
  assert rc.tex_data.dtype == torch.int32 and rc.tex_data.shape == (8 + 24,)
  assert rc.tex_adr.tolist() == [0, 8, -1] and rc.tex_width.tolist() == [4, 6, 8] and rc.tex_height.tolist() == [2, 4, 48]
  words = rc.tex_data.numpy().astype(np.int64) & 0xFFFFFFFF
  t8 = scenes.TEX8.reshape(-1, 3).astype(np.int64)
  assert np.array_equal(words[:8], t8[:, 0] | t8[:, 1] << 8 | t8[:, 2] << 16 | 255 << 24)
  assert words[8] == 255 | 255 << 8 | 255 << 16 | 255 << 24  # the checker's marked edge
  assert rc.mesh_texcoord.dtype == torch.float32 and tuple(rc.mesh_texcoord.shape) == (mjm.ntexcoord, 2) and mjm.ntexcoord == 4 + 9 * 7
  assert rc.mesh_texcoordadr.tolist() == [0, 4] and tuple(rc.mesh_facetexcoord.shape) == (mjm.nmeshface, 3) and mjm.nmeshface == 4 + 80
  assert np.array_equal(rc.mesh_facetexcoord.numpy(), mjm.mesh_facetexcoord)
  m = mjw.put_model(mjm, device="cpu")
  assert m.mat_texid.dtype == torch.int32 and tuple(m.mat_texid.shape) == (1, 2, 10) and m.mat_texid[0, :, 1].tolist() == [0, -1]
  assert m.mat_texrepeat.dtype == torch.float32 and m.mat_texrepeat[0].tolist() == [[1.5, 0.75], [1.0, 1.0]]
  off = mjw.create_render_context(mjm, cam_res=(4, 3), device="cpu", use_textures=False)
  plain = mjw.create_render_context(_load(render_scenes.RENDER_ALL_TYPES_XML), cam_res=(4, 3), device="cpu")
  for c in (off, plain):
    assert not c.has_textures
    for name in ("tex_data", "tex_adr", "tex_width", "tex_height", "mesh_texcoord", "mesh_texcoordadr", "mesh_facetexcoord"):
      assert getattr(c, name).shape[0] == 0, name


# ---- 6. the yardstick ----------------------------------------------------------------------------------------------------
def test_yardstick_sampling():
  tex = scenes.TEX8
  H, W = tex.shape[:2]
  for r in range(H):
    for c in range(W):  # a texel centre returns the texel
      assert np.allclose(texture_ref.sample(tex, [[(c + 0.5) / W, (r + 0.5) / H]]), tex[r, c] / 255.0, atol=1e-12)
  # u = 0 lies between the last and the first column; v at a row centre
  got = texture_ref.sample(tex, [[0.0, 0.25], [1.0, 0.75], [-3.0, 0.25]])
  assert np.allclose(got[0], (tex[0, 0] / 255.0 + tex[0, 3] / 255.0) / 2) and np.allclose(got[1], (tex[1, 0] / 255.0 + tex[1, 3] / 255.0) / 2)
  assert np.allclose(got[2], got[0])
  # the repeat scales uv before the fraction is taken
  assert np.allclose(texture_ref.sample(tex, [[0.125 / 2, 0.25 / 4]], (2.0, 4.0)), tex[0, 0] / 255.0)
  one = np.full((3, 5, 3), 0, dtype=np.uint8) + np.array([10, 200, 90], dtype=np.uint8)
  uv = np.random.default_rng(0).uniform(-7, 7, (50, 2))
  assert np.allclose(texture_ref.sample(one, uv, (1.3, 0.4)), np.array([10, 200, 90]) / 255.0, atol=1e-12)


# ---- 7. the skip share of the GPU tests' scenes --------------------------------------------------------------------------
def _host_render(mjm, W, H, use_shadows=False):
  fr = render_scenes.host_frames_all(mjm)
  return texture_ref.render(mjm, fr["geom_xpos"], fr["geom_xmat"], fr["cam_xpos"][0], fr["cam_xmat"][0], mjm.cam_fovy[0],
                            np.asarray(mjm.cam_sensorsize).reshape(-1, 2)[0], np.asarray(mjm.cam_intrinsic).reshape(-1, 4)[0], W, H,
                            fr["light_xpos"], fr["light_xdir"], use_shadows=use_shadows)


def test_skip_share_of_the_gpu_scenes(tmp_path):
  png = scenes.write_png(tmp_path / "t8.png", scenes.TEX8)
  obj = scenes.uv_sphere_obj(tmp_path / "ball.obj")
  bare_obj = scenes.uv_sphere_obj(tmp_path / "bare.obj", vt=False)
  assert bare_obj
  cases = [("plane", scenes.plane_xml(png), scenes.RES_TILES, False), ("plane", scenes.plane_xml(png), scenes.RES_WAVE, False),
           ("mesh", scenes.mesh_xml(png, obj), scenes.RES_TILES, False), ("untextured", scenes.untextured_xml(png), scenes.RES_TILES, False),
           ("shadow", scenes.shadow_xml(png), scenes.RES_TILES, True), ("flex floor", scenes.flex_xml(png), scenes.RES_TILES, False)]
  for name, xml, (W, H), shadows in cases:
    mjm = _load(xml)
    seg, depth, rgb, ok, face, uv = _host_render(mjm, W, H, shadows)
    share = float((~ok).mean())
    print(f"{name} {W} x {H}: {int((~ok).sum())} of {W * H} pixels non-decisive ({share:.4f}); hits per geom {np.bincount(seg[seg >= 0], minlength=mjm.ngeom)}")
    assert share <= 0.02, f"{name} {W} x {H}: {share:.4f} of the pixels are non-decisive"
    if name == "plane":  # local coordinates of both signs, several texels, and background in view
      on = seg == 0
      assert on.sum() > 0.4 * W * H and (seg < 0).any()
      assert uv[on, 0].min() < -0.3 and uv[on, 0].max() > 0.3 and uv[on, 1].min() < -0.3 and uv[on, 1].max() > 0.3
      assert len(np.unique(rgb[on], axis=0)) > 8
    if name == "mesh":
      tetra, ball = seg == 0, seg == 1
      assert tetra.sum() >= 20 and ball.sum() >= 60 and np.all(face[tetra | ball] >= 0) and len(np.unique(face[ball])) >= 8
      assert not np.isnan(uv[tetra | ball]).any()
    if name == "untextured":  # nothing takes a texel: the image is render_ref's
      assert np.isnan(uv).all() and (np.bincount(seg[seg >= 0], minlength=4)[:4] >= 15).all()
      fr = render_scenes.host_frames_all(mjm)
      from tests import render_ref
      plain = render_ref.render(mjm, fr["geom_xpos"], fr["geom_xmat"], fr["cam_xpos"][0], fr["cam_xmat"][0], mjm.cam_fovy[0],
                                np.asarray(mjm.cam_sensorsize).reshape(-1, 2)[0], np.asarray(mjm.cam_intrinsic).reshape(-1, 4)[0], W, H,
                                fr["light_xpos"], fr["light_xdir"])
      assert np.array_equal(plain[2], rgb)
