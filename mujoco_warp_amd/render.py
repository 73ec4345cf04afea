"""Batched camera rendering: segmentation, depth and shaded RGB images of a model's cameras
(mujoco_warp/_src/render.py `render`, io.py `create_render_context`, render_util.py readers).

One HIP launch (`mjw_render_bvh`, `mjw_render_flex` for a context made with `render_flex`, `mjw_render_tex` for a context that has
textures; csrc/mjw_render.hip) on the Data's stream per `render` call: a workgroup per
world, camera and 16 x 16 pixel tile makes the pixel rays from `d.cam_xpos` / `d.cam_xmat` and the per-world
camera parameters, finds the nearest geom with the geom loop `rays` uses, and writes every pixel of every
enabled output.  No kinematics run here: the frames are those the last position stage left.

Meshes are intersected through a static BVH per mesh (bvh.py), built on the host when the context is made and
walked by the kernel in place of the loop over every face, with the same result bit for bit (meshes of fewer than
`rc.bvh_min_faces` faces, default bvh.BVH_MIN_FACES, keep the loop: the walk does not pay there).  The trees live
in the mesh's own frame and meshes are rigid, so they are never refit (`refit_bvh` leaves them alone).  They were
built from the host model's vertices: when `m.mesh_vert` is batched per world (leading dim > 1) the call falls
back to the face loop.

Flexes are drawn by a context made with `render_flex=True` (the default still refuses a model with flexes): cloth as
a shell of thickness 2 flex_radius around its elements, closed along the boundary edges, soft bodies as their
flex_shell triangles, ropes as one capsule per edge; segmentation -2, colour `flex_rgba`.  Each flex with faces has
a tree whose topology is built once over the rest pose and whose boxes `refit_bvh` refits to `d.flexvert_xpos`, per
world, in one launch (`mjw_flex_refit`, csrc/mjw_flexrender.hip).  `render` does not refit: call `refit_bvh` after the
step and before `render`, as code written for the reference does.  The faces are never stored: the context keeps
corner records and, per world, the node boxes and the vertex normals.

Textures (`use_textures`, the default): the 2D textures the MJCF compiler kept are packed into the context, one word per
texel, and the base colour of a pixel on a plane (uv = the hit in the plane's frame) or on a mesh with texture coordinates
(uv = the barycentric mean of the hit face's) is multiplied by a bilinear, repeating sample of the texture its material names,
before the ambient and light terms.  mat_texid / mat_texrepeat may be batched per world.  Other geom types, meshes without
texture coordinates and flexes keep their colour; cube and skybox textures are never sampled.  A context without textures
(use_textures=False, or a model with none) makes the launches it always made.

There is no BVH over the geoms (they are culled by bounding ball and box per wave) or over heightfields and no
orthographic cameras.
"""

from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .bvh import BVH_LEAF, BVH_MAX_DEPTH, BVH_MIN_FACES, FLEX_BVH_MIN_FACES, FLEX_INFO_WORDS, NODE_WORDS, build_flex_tables, build_mesh_bvh
from .types import Data, Model, RenderContext

TILE = 16  # pixels per side of a workgroup's tile (csrc/mjw_render.hip)
_CAMOUT_RGB, _CAMOUT_DEPTH, _CAMOUT_SEG = 1, 2, 16  # mjtCamOutBit


def _flags(given, ncam, mjm, active, bit, default):
  if given is None:
    out = getattr(mjm, "cam_output", None)
    return [bool(int(out[i]) & bit) for i in active] if out is not None else [default] * ncam
  if isinstance(given, (bool, np.bool_)):
    return [bool(given)] * ncam
  return [bool(x) for x in given]


def create_render_context(mjm, nworld: int = 1, cam_res=None, render_rgb=None, render_depth=None, render_seg=None, use_textures: bool = True,
                          use_shadows: bool = False, enabled_geom_groups: Sequence[int] = [0, 1, 2], cam_active: Optional[Sequence[bool]] = None,
                          flex_render_smooth: bool = True, use_precomputed_rays: bool = True, device=None, render_flex: bool = False) -> RenderContext:
  """Creates a render context on the device (io.py:2649-2904).

  cam_res: one (width, height) tuple for every active camera, a list with one per active camera, or None for
  `mjm.cam_resolution`.  render_rgb / render_depth / render_seg: a bool, a list with one bool per active camera,
  or None for the model's `cam_output` bits where the host model carries them, else RGB only.  A geom is drawn
  iff its group is one of enabled_geom_groups (each in 0..31).  cam_active: one bool per model camera (None: all).
  use_shadows: lights with castshadow throw shadows.  The BVHs of the model's meshes are built here, on the host
  (rc.mesh_bvh_node / mesh_bvh_tri / mesh_bvh_adr; empty for a model without meshes).

  render_flex: draw the model's flexes (module docstring).  The context then holds the flex tables (bvh.py
  `build_flex_tables`: rc.flex_info, flex_corner, flex_elem_vert, flex_edge_vert, flex_inc_adr, flex_inc, flex_bvh_node,
  flex_bvh_tri, flex_bvh_level, flex_radius, flex_rgba) and two per-world buffers, rc.flex_node_box (nworld, nodes +
  nflex, 6) and rc.flexvert_norm (nworld, nflexvert, 3), which `refit_bvh` fills; `render` refuses the context until
  it has.  flex_render_smooth: cloth faces are offset along the vertex normals (True) or along each element's own
  normal (False).  rc.flex_bvh_min_faces (a host int the caller may change, default bvh.FLEX_BVH_MIN_FACES; 0 walks
  every flex): flexes with fewer faces are intersected face by face, with the same image.  For a model without
  flexes the flag changes nothing.  Without it a model with flexes raises NotImplementedError: its flex elements
  would be silently invisible.

  use_textures: every 2D texture of the model that has data is packed into rc.tex_data (int32, one r | g << 8 | b << 16 |
  255 << 24 word per texel) with rc.tex_adr / tex_width / tex_height (ntex,; tex_adr -1 for a texture that is never
  sampled), next to device copies of mesh_texcoord, mesh_texcoordadr and mesh_facetexcoord; rc.has_textures is then True
  and `render` textures planes and meshes (module docstring).  With use_textures=False, and for a model without such
  textures, these tables are empty and `render` is what it is without them, bit for bit.

  Accepted and ignored: `use_precomputed_rays` (the rays are always made in the kernel, so per-world cam_fovy /
  cam_intrinsic work)."""
  from .io import _device

  nflex = int(getattr(mjm, "nflex", 0))
  if nflex > 0 and not render_flex:
    raise NotImplementedError("create_render_context: flex rendering is opt-in and the model has flexes: pass render_flex=True "
                              "(call refit_bvh before render)")
  dev = _device(device)
  nworld = int(nworld)
  if nworld < 1:
    raise ValueError(f"create_render_context: nworld must be positive, got {nworld}")
  ncam_model = int(mjm.ncam)
  if cam_active is not None:
    assert len(cam_active) == ncam_model, f"cam_active must have length {ncam_model} (got {len(cam_active)})"
    active = [i for i, on in enumerate(cam_active) if on]
  else:
    active = list(range(ncam_model))
  ncam = len(active)

  if cam_res is not None:
    if isinstance(cam_res, tuple):
      cam_res = [cam_res] * ncam
    assert len(cam_res) == ncam, f"Camera resolutions must be provided for all active cameras (got {len(cam_res)}, expected {ncam})"
    res = np.asarray(cam_res, dtype=np.int64).reshape(ncam, 2)
  else:
    res = np.asarray(mjm.cam_resolution, dtype=np.int64).reshape(ncam_model, 2)[active]
  if ncam and res.min() < 1:
    raise ValueError(f"create_render_context: camera resolutions must be positive, got {res.tolist()}")

  rgb = _flags(render_rgb, ncam, mjm, active, _CAMOUT_RGB, True)
  depth = _flags(render_depth, ncam, mjm, active, _CAMOUT_DEPTH, False)
  seg = _flags(render_seg, ncam, mjm, active, _CAMOUT_SEG, False)
  assert len(rgb) == ncam and len(depth) == ncam and len(seg) == ncam, (
    f"render_rgb, render_depth, and render_seg must be a bool or a list of bools with length {ncam}")

  groups = [int(g) for g in enabled_geom_groups]
  if any(g < 0 or g > 31 for g in groups):
    raise ValueError(f"create_render_context: enabled_geom_groups must lie in 0..31, got {groups}")
  group_mask = 0
  for g in groups:
    group_mask |= 1 << g

  rgb_adr, depth_adr, seg_adr = -np.ones(ncam, dtype=np.int64), -np.ones(ncam, dtype=np.int64), -np.ones(ncam, dtype=np.int64)
  ri = di = si = total = 0
  for i in range(ncam):
    npix = int(res[i, 0] * res[i, 1])
    if rgb[i]:
      rgb_adr[i], ri = ri, ri + npix
    if depth[i]:
      depth_adr[i], di = di, di + npix
    if seg[i]:
      seg_adr[i], si = si, si + npix
    total += npix
  if max(ri, di, si) >= 2**31:
    raise ValueError("create_render_context: more than 2^31 pixels in one output row")

  # the launch's tile table: cameras whose three outputs are all off get no tiles
  drawn = [i for i in range(ncam) if rgb[i] or depth[i] or seg[i]]
  if all(res[i, 0] * res[i, 1] <= 64 for i in drawn):
    tile_threads, tiles = 64, [(i, 0, 0, 0) for i in drawn]
  else:
    tile_threads = 256
    tiles = [(i, x0, y0, 0) for i in drawn for y0 in range(0, int(res[i, 1]), TILE) for x0 in range(0, int(res[i, 0]), TILE)]

  i32 = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a).astype(np.int32)), device=dev)
  nl = int(mjm.nlight)
  nmesh, nmeshface = int(getattr(mjm, "nmesh", 0)), int(getattr(mjm, "nmeshface", 0))
  if nmesh > 0:
    node, tri, adr, bvh_depth = build_mesh_bvh(mjm.mesh_vert, mjm.mesh_vertadr, mjm.mesh_face, mjm.mesh_faceadr, mjm.mesh_facenum)
  else:
    node, tri, adr, bvh_depth = build_mesh_bvh(np.zeros((0, 3)), [], np.zeros((0, 3)), [], [])
  flex = {}
  if nflex > 0:  # (flexes take no texture: their colour stays flex_rgba)
    t = build_flex_tables(mjm, smooth=bool(flex_render_smooth))
    nnode, nfv = int(t["node"].shape[0]), int(mjm.nflexvert)
    rgba = np.asarray(getattr(mjm, "flex_rgba", np.tile([0.5, 0.5, 0.5, 1.0], (nflex, 1))), dtype=np.float32).reshape(nflex, 4)
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32)), device=dev)
    flex = dict(
      render_flex=True,
      flex_render_smooth=bool(flex_render_smooth),
      flex_info=i32(t["info"]), flex_corner=i32(t["corner"]), flex_elem_vert=i32(t["elem_vert"]), flex_edge_vert=i32(t["edge_vert"]),
      flex_inc_adr=i32(t["inc_adr"]), flex_inc=i32(t["inc"]), flex_bvh_node=torch.as_tensor(t["node"], device=dev),
      flex_bvh_tri=i32(t["tri"]), flex_bvh_level=i32(t["level"]), flex_radius=f32(mjm.flex_radius), flex_rgba=f32(rgba),
      flex_node_box=torch.zeros((nworld, nnode + nflex, 6), dtype=torch.float32, device=dev),
      flexvert_norm=torch.zeros((nworld, nfv, 3), dtype=torch.float32, device=dev),
      flex_bvh_max_depth=int(t["depth"]),
      flex_bvh_min_faces=FLEX_BVH_MIN_FACES,
      _flex_frag=[np.asarray(x) for x in t["frag"]],
      _flex_counts=(nflex, nfv, int(mjm.nflexelem), int(mjm.nflexedge)),
      _flex_refit=False,
    )
  tex = _texture_tables(mjm, bool(use_textures))
  return RenderContext(
    **flex,
    has_textures=bool(tex["tex_data"].size),
    tex_data=torch.as_tensor(tex["tex_data"], device=dev), tex_adr=i32(tex["tex_adr"]), tex_width=i32(tex["tex_width"]),
    tex_height=i32(tex["tex_height"]), mesh_texcoord=torch.as_tensor(tex["mesh_texcoord"], device=dev),
    mesh_texcoordadr=i32(tex["mesh_texcoordadr"]), mesh_facetexcoord=i32(tex["mesh_facetexcoord"]),
    nworld=nworld,
    nrender=ncam,
    cam_res=i32(res.reshape(ncam, 2)),
    cam_id_map=i32(np.asarray(active, dtype=np.int64)),
    use_textures=bool(use_textures),
    use_shadows=bool(use_shadows),
    enabled_geom_groups=groups,
    group_mask=group_mask,
    background_color=255 << 24 | 25 << 16 | 25 << 8 | 51,
    rgb_adr=i32(rgb_adr),
    depth_adr=i32(depth_adr),
    seg_adr=i32(seg_adr),
    render_rgb=torch.as_tensor(rgb, dtype=torch.bool, device=dev).reshape(ncam),
    render_depth=torch.as_tensor(depth, dtype=torch.bool, device=dev).reshape(ncam),
    render_seg=torch.as_tensor(seg, dtype=torch.bool, device=dev).reshape(ncam),
    total_rays=int(total),
    light_type=i32(np.asarray(getattr(mjm, "light_type", np.zeros(nl))).reshape(-1)[:nl]),
    light_active=i32(np.asarray(getattr(mjm, "light_active", np.ones(nl))).reshape(-1)[:nl]),
    light_castshadow=i32(np.asarray(getattr(mjm, "light_castshadow", np.ones(nl))).reshape(-1)[:nl]),
    tile=i32(np.asarray(tiles, dtype=np.int64).reshape(len(tiles), 4)),
    tile_threads=tile_threads,
    rgb_data=torch.zeros((nworld, ri), dtype=torch.int32, device=dev),
    depth_data=torch.zeros((nworld, di), dtype=torch.float32, device=dev),
    seg_data=torch.zeros((nworld, max(si, 1)), dtype=torch.int32, device=dev),
    mesh_bvh_node=torch.as_tensor(node, device=dev),
    mesh_bvh_tri=torch.as_tensor(tri, device=dev),
    mesh_bvh_adr=torch.as_tensor(adr, device=dev),
    bvh_leaf_size=BVH_LEAF,
    bvh_max_depth=int(bvh_depth),
    bvh_min_faces=BVH_MIN_FACES,
    # host copies for the readers and for validation
    _res=[(int(w), int(h)) for w, h in res],
    _adr=dict(rgb=[int(x) for x in rgb_adr], depth=[int(x) for x in depth_adr], seg=[int(x) for x in seg_adr]),
    _ncam_model=ncam_model,
    _nlight=nl,
    _nmesh=nmesh,
    _nmeshface=nmeshface,
  )


def _texture_tables(mjm, use_textures: bool) -> dict:
  """The host arrays of a context's texture tables: every 2D texture with data packed one word per texel, and the mesh
  texcoord tables; all empty when use_textures is off or the model has no such texture."""
  ntex = int(getattr(mjm, "ntex", 0))
  out = dict(tex_data=np.zeros(0, np.int32), tex_adr=np.zeros(0, np.int32), tex_width=np.zeros(0, np.int32), tex_height=np.zeros(0, np.int32),
             mesh_texcoord=np.zeros((0, 2), np.float32), mesh_texcoordadr=np.zeros(0, np.int32), mesh_facetexcoord=np.zeros((0, 3), np.int32))
  if not use_textures or ntex == 0:
    return out
  adr, words, n = -np.ones(ntex, dtype=np.int64), [], 0
  for i in range(ntex):
    w, h, a = int(mjm.tex_width[i]), int(mjm.tex_height[i]), int(mjm.tex_adr[i])
    if int(mjm.tex_type[i]) != 0 or a < 0 or w < 1 or h < 1:
      continue
    b = np.asarray(mjm.tex_data[a : a + 3 * w * h], dtype=np.uint32).reshape(w * h, 3)
    words.append(b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16 | np.uint32(255 << 24))
    adr[i], n = n, n + w * h
  if n == 0:
    return out
  if n >= 2**31:
    raise ValueError("create_render_context: more than 2^31 texels")
  nmesh, nface = int(getattr(mjm, "nmesh", 0)), int(getattr(mjm, "nmeshface", 0))
  out.update(tex_data=np.concatenate(words).astype(np.uint32).view(np.int32), tex_adr=adr, tex_width=np.asarray(mjm.tex_width), tex_height=np.asarray(mjm.tex_height),
             mesh_texcoord=np.ascontiguousarray(np.asarray(getattr(mjm, "mesh_texcoord", np.zeros((0, 2))), dtype=np.float32).reshape(-1, 2)),
             mesh_texcoordadr=np.asarray(getattr(mjm, "mesh_texcoordadr", -np.ones(nmesh))).reshape(nmesh),
             mesh_facetexcoord=np.asarray(getattr(mjm, "mesh_facetexcoord", np.zeros((nface, 3)))).reshape(nface, 3))
  return out


def _ctex(rc: RenderContext, m: Model, d: Data, who: str) -> _lib.CTexture:
  """mjw_texture_t of a context that has textures and the Model's current mat_texid / mat_texrepeat (built per call: a
  caller may have replaced them with per-world batches); ValueError when a table has not the shape its count asks for."""
  dev = d.qpos.device
  nmat = int(m.nmat)
  c = _lib.CTexture()
  for name, dtype, tail in (("tex_data", torch.int32, ()), ("tex_adr", torch.int32, ()), ("tex_width", torch.int32, ()), ("tex_height", torch.int32, ()),
                            ("mesh_texcoord", torch.float32, (2,)), ("mesh_texcoordadr", torch.int32, ()), ("mesh_facetexcoord", torch.int32, (3,))):
    setattr(c, name, _lib.check_tensor(who, "rc." + name, getattr(rc, name), dtype, dev, (None,) + tail).data_ptr())
  ntex = int(rc.tex_adr.shape[0])
  if int(rc.tex_width.shape[0]) != ntex or int(rc.tex_height.shape[0]) != ntex:
    raise ValueError(f"{who}: rc.tex_adr / tex_width / tex_height must hold the same number of textures")
  nmesh, nface = int(rc.mesh_texcoordadr.shape[0]), int(rc.mesh_facetexcoord.shape[0])
  if nmesh not in (0, int(m.nmesh)) or nface not in (0, int(m.nmeshface)):
    raise ValueError(f"{who}: rc.mesh_texcoordadr / mesh_facetexcoord must hold {m.nmesh} meshes and {m.nmeshface} faces (or none)")
  texid = _lib.check_tensor(who, "m.mat_texid", getattr(m, "mat_texid", None), torch.int32, dev, (None, nmat, 10))
  texrep = _lib.check_tensor(who, "m.mat_texrepeat", getattr(m, "mat_texrepeat", None), torch.float32, dev, (None, nmat, 2))
  if texid.shape[0] < 1 or texrep.shape[0] < 1:
    raise ValueError(f"{who}: m.mat_texid / m.mat_texrepeat need a leading batch dimension of at least 1")
  c.ntex, c.ntexdata, c.nmat, c.nmesh, c.ntexcoord, c.nmeshface = ntex, int(rc.tex_data.shape[0]), nmat, nmesh, int(rc.mesh_texcoord.shape[0]), nface
  c.mat_texid, c.mat_texid_nb = texid.data_ptr(), int(texid.shape[0])
  c.mat_texrepeat, c.mat_texrepeat_nb = texrep.data_ptr(), int(texrep.shape[0])
  c._keep = (texid, texrep)
  return c


def _crender(rc: RenderContext) -> _lib.CRender:
  c = _lib.CRender()
  c.group_mask, c.use_shadows = int(rc.group_mask), int(bool(rc.use_shadows))
  c.nrender, c.ntile, c.tile_threads = int(rc.nrender), int(rc.tile.shape[0]), int(rc.tile_threads)
  n, nl, dev = int(rc.nrender), int(rc._nlight), rc.rgb_data.device
  if len(rc._res) != n:
    raise ValueError(f"render: the context's host tables must hold {n} cameras")
  for name, shape in (("cam_id_map", (n,)), ("cam_res", (n, 2)), ("rgb_adr", (n,)), ("depth_adr", (n,)), ("seg_adr", (n,)), ("tile", (None, 4)),
                      ("light_type", (nl,)), ("light_active", (nl,)), ("light_castshadow", (nl,))):
    setattr(c, name, _lib.check_tensor("render", "rc." + name, getattr(rc, name), torch.int32, dev, shape).data_ptr())
  for name, dtype in (("rgb", torch.int32), ("depth", torch.float32), ("seg", torch.int32)):
    t = _lib.check_tensor("render", f"rc.{name}_data", getattr(rc, name + "_data"), dtype, dev, (int(rc.nworld), None))
    need = max((a + w * h for a, (w, h) in zip(rc._adr[name], rc._res) if a >= 0), default=0)
    if t.shape[1] < need:
      raise ValueError(f"render: rc.{name}_data must hold {need} pixels per world, it holds {t.shape[1]}")
    setattr(c, name, t.data_ptr())
    setattr(c, name + "_ld", int(t.shape[1]))
  return c


def _made_for(who: str, rc: RenderContext, m: Model, d: Data) -> None:
  """The one check per call (render, refit_bvh, rays) that the context was made for this nworld, device and model."""
  if int(rc.nworld) != int(d.nworld):
    raise ValueError(f"{who}: the render context was made for nworld = {rc.nworld}, the Data has {d.nworld}")
  if rc.rgb_data.device != d.qpos.device:
    raise ValueError(f"{who}: the render context is on {rc.rgb_data.device}, the Data is on {d.qpos.device}")
  names = ["cameras", "lights", "meshes", "mesh faces"]
  made, have = [rc._ncam_model, rc._nlight, rc._nmesh, rc._nmeshface], [m.ncam, m.nlight, m.nmesh, m.nmeshface]
  if _is_flex(rc):
    names += ["flexes", "flex vertices", "flex elements", "flex edges"]
    made, have = made + list(rc._flex_counts), have + [m.nflex, m.nflexvert, m.nflexelem, m.nflexedge]
  if [int(x) for x in made] != [int(x) for x in have]:
    say = lambda counts: ", ".join(f"{int(x)} {name}" for x, name in zip(counts, names))
    raise ValueError(f"{who}: the render context was made for a model with {say(made)}; this one has {say(have)}")


def _cbvh(rc: RenderContext, m: Model, d: Data, who: str) -> _lib.CBvh:
  """mjw_bvh_t of the context's trees (the caller has made the `_made_for` check; the builders share one signature,
  this one reads nothing of m)."""
  nmesh, nface = int(rc._nmesh), int(rc._nmeshface)
  dev = d.qpos.device
  node = _lib.check_tensor(who, "rc.mesh_bvh_node", rc.mesh_bvh_node, torch.float32, dev, (None, NODE_WORDS))
  tri = _lib.check_tensor(who, "rc.mesh_bvh_tri", rc.mesh_bvh_tri, torch.int32, dev, (nface,))
  adr = _lib.check_tensor(who, "rc.mesh_bvh_adr", rc.mesh_bvh_adr, torch.int32, dev, (nmesh, 4))
  if int(rc.bvh_leaf_size) > BVH_LEAF or int(rc.bvh_max_depth) > BVH_MAX_DEPTH:
    raise ValueError(f"{who}: the context's BVH has leaves of {rc.bvh_leaf_size} triangles and {rc.bvh_max_depth} levels; "
                     f"the kernel takes {BVH_LEAF} and {BVH_MAX_DEPTH}")
  c = _lib.CBvh()
  c.nmesh, c.nnode, c.ntri = nmesh, int(node.shape[0]), nface
  c.leaf_size, c.max_depth, c.min_faces = int(rc.bvh_leaf_size), int(rc.bvh_max_depth), max(int(rc.bvh_min_faces), 0)
  c.node, c.tri, c.adr = node.data_ptr(), tri.data_ptr(), adr.data_ptr()
  return c


_FLEX_TABLES = (("info", "flex_info", torch.int32, (FLEX_INFO_WORDS,)), ("flex_radius", "flex_radius", torch.float32, ()),
                ("flex_rgba", "flex_rgba", torch.float32, (4,)), ("corner", "flex_corner", torch.int32, (3, 3)),
                ("elem_vert", "flex_elem_vert", torch.int32, (3,)), ("edge_vert", "flex_edge_vert", torch.int32, (2,)),
                ("inc_adr", "flex_inc_adr", torch.int32, ()), ("inc", "flex_inc", torch.int32, ()), ("node", "flex_bvh_node", torch.float32, (NODE_WORDS,)),
                ("tri", "flex_bvh_tri", torch.int32, ()), ("level", "flex_bvh_level", torch.int32, ()))


def _is_flex(rc: RenderContext) -> bool:
  return bool(getattr(rc, "render_flex", False))


def _cflex(rc: RenderContext, m: Model, d: Data, who: str) -> _lib.CFlexRender:
  """mjw_flexrender_t of a context made with render_flex (the caller has made the `_made_for` check); ValueError when
  a table has not the shape its counts ask for (the kernels trust the counts)."""
  nflex, nfv, nelem, nedge = rc._flex_counts
  dev = d.qpos.device
  c = _lib.CFlexRender()
  nface = int(_lib.check_tensor(who, "rc.flex_corner", rc.flex_corner, torch.int32, dev, (None, 3, 3)).shape[0])
  rows = dict(flex_info=nflex, flex_radius=nflex, flex_rgba=nflex, flex_elem_vert=nelem, flex_edge_vert=nedge, flex_inc_adr=nfv + 1, flex_bvh_tri=nface)
  for cname, name, dtype, tail in _FLEX_TABLES:
    setattr(c, cname, _lib.check_tensor(who, "rc." + name, getattr(rc, name), dtype, dev, (rows.get(name),) + tail).data_ptr())
  nnode = int(rc.flex_bvh_node.shape[0])
  for name, shape in (("flex_node_box", (int(rc.nworld), nnode + nflex, 6)), ("flexvert_norm", (int(rc.nworld), nfv, 3))):
    _lib.check_tensor(who, "rc." + name, getattr(rc, name), torch.float32, dev, shape)
  if int(rc.flex_bvh_max_depth) > BVH_MAX_DEPTH:
    raise ValueError(f"{who}: the context's flex trees have {rc.flex_bvh_max_depth} levels; the kernel takes {BVH_MAX_DEPTH}")
  c.nflex, c.nflexvert, c.nflexelem, c.nflexedge, c.nface, c.nnode = nflex, nfv, nelem, nedge, nface, nnode
  c.ninc, c.nlevel = int(rc.flex_inc.shape[0]), int(rc.flex_bvh_level.shape[0])
  c.leaf_size, c.max_depth, c.min_faces = BVH_LEAF, int(rc.flex_bvh_max_depth), max(int(rc.flex_bvh_min_faces), 0)
  c.node_box, c.vert_norm = rc.flex_node_box.data_ptr(), rc.flexvert_norm.data_ptr()
  return c


def render(m: Model, d: Data, rc: RenderContext) -> None:
  """Renders every camera of the context in every world into rc.rgb_data / rc.depth_data / rc.seg_data
  (render.py:515-830), in one launch on the Data's stream; capturable in a graph.

  Segmentation: the geom id of the nearest drawn geom, -1 for background.  Depth: the distance along the
  camera's optical axis, 0 for background.  RGB: mat_rgba (geoms with a material) or geom_rgba, on a context that has
  textures times the texture sample of planes and of meshes with texture coordinates (module docstring), shaded with a
  hemispheric ambient term and the active lights (directional, point with 1 / (1 + 0.02 r^2), spot with the
  reference's cone), clamped and packed as a << 24 | r << 16 | g << 8 | b; background (25, 25, 51, 255).  A geom
  is drawn iff its group is enabled in the context: alpha plays no part.  cam_fovy, cam_intrinsic, geom_rgba,
  mat_rgba, mat_texid and mat_texrepeat may be batched per world.  The camera, light and geom frames are those of the last position
  stage (`forward`, `step`, `kinematics` + `camlight`).  Meshes are walked through the context's BVHs; with a
  per-world batched `m.mesh_vert` (leading dim > 1), which the trees were not built from, the launch loops over
  every face instead.  Both give the same images bit for bit.

  A context made with render_flex also draws the flexes, from the boxes and normals the last `refit_bvh` left (it does
  not refit; before the first `refit_bvh` it raises ValueError): the nearest hit over geoms and flexes, a flex only
  when strictly nearer than every geom; segmentation -2, colour flex_rgba (no material, texture or group filter), the
  normal of a flex triangle its winding normal turned to face the ray; flexes throw and receive shadows like geoms."""
  if not isinstance(rc, RenderContext):
    raise ValueError("render: rc must be a RenderContext from create_render_context")
  _made_for("render", rc, m, d)
  from .forward import _stream
  from .io import cdata, cmodel
  from .ray import _ray_model

  bvh = _cbvh(rc, m, d, "render")
  rm = _ray_model(m)
  c = _crender(rc)
  fr = _cflex(rc, m, d, "render") if _is_flex(rc) else None
  if fr is not None and not rc._flex_refit:
    raise ValueError("render: the context's flex trees have never been refit: call refit_bvh(m, d, rc) after the step and before render")
  tex = _ctex(rc, m, d, "render") if bool(getattr(rc, "has_textures", False)) else None
  if c.ntile == 0:
    return
  # the entry that takes what the context has, and its arguments after the bvh (a null flex table: no flexes)
  if tex is not None:
    entry, more = "mjw_render_tex", (ctypes.byref(fr) if fr is not None else None, ctypes.byref(tex))
  elif fr is not None:
    entry, more = "mjw_render_flex", (ctypes.byref(fr),)
  else:
    entry, more = "mjw_render_bvh", ()
  rcode = getattr(_lib.lib(), entry)(cmodel(m), cdata(d), ctypes.byref(rm), ctypes.byref(c), ctypes.byref(bvh), *more, _stream(d))
  _lib.check(rcode, entry)


def refit_bvh(m: Model, d: Data, rc: RenderContext) -> None:
  """Refits the flex trees of a context made with render_flex to `d.flexvert_xpos`: one launch (`mjw_flex_refit`) on
  the Data's stream writes, per world, the vertex normals, every node's box and the whole-flex boxes; capturable in a
  graph.  Call it after the step (or `forward`) and before `render`, once per step.

  For every other context it does nothing.  The per-mesh trees live in each mesh's own frame: meshes are rigid, so a
  moving geom moves its frame and the tree stays valid, and there is no BVH over the geoms to refit.  So code written
  for the reference (`refit_bvh` before every `render`) runs unchanged.  Returns None either way."""
  if not isinstance(rc, RenderContext) or not _is_flex(rc):
    return None
  from .forward import _stream
  from .io import cdata, cmodel

  _made_for("refit_bvh", rc, m, d)
  fr = _cflex(rc, m, d, "refit_bvh")
  rcode = _lib.lib().mjw_flex_refit(cmodel(m), cdata(d), ctypes.byref(fr), _stream(d))
  _lib.check(rcode, "mjw_flex_refit")
  rc._flex_refit = True
  return None


def _view(rc, camera_index, which, out, shape_tail, dtype, name):
  if not isinstance(rc, RenderContext):
    raise ValueError(f"{name}: rc must be a RenderContext")
  ci = int(camera_index)
  if ci < 0 or ci >= int(rc.nrender):
    raise ValueError(f"{name}: camera_index {ci} is not one of the context's {rc.nrender} cameras")
  adr = rc._adr[which][ci]
  if adr < 0:
    raise ValueError(f"{name}: camera {ci} does not render {which} in this context")
  w, h = rc._res[ci]
  data = getattr(rc, which + "_data")
  shape = (int(rc.nworld), h, w) + shape_tail
  if not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != dtype or out.device != data.device:
    raise ValueError(f"{name}: the output must be a {dtype} tensor of shape {shape} on {data.device}")
  return data[:, adr : adr + w * h].reshape(int(rc.nworld), h, w)


def get_rgb(rc: RenderContext, camera_index: int, rgb_out: torch.Tensor) -> None:
  """The RGB image of the context's camera `camera_index` (an index into its rendered cameras) as float32
  (nworld, H, W, 3) in [0, 1], byte / 255."""
  px = _view(rc, camera_index, "rgb", rgb_out, (3,), torch.float32, "get_rgb")
  for i, shift in enumerate((16, 8, 0)):
    rgb_out[..., i] = ((px >> shift) & 0xFF).to(torch.float32) / 255.0


def get_depth(rc: RenderContext, camera_index: int, depth_scale: float, depth_out: torch.Tensor) -> None:
  """clamp(depth / depth_scale, 0, 1) of the context's camera `camera_index` as float32 (nworld, H, W)."""
  px = _view(rc, camera_index, "depth", depth_out, (), torch.float32, "get_depth")
  torch.clamp(px / float(depth_scale), 0.0, 1.0, out=depth_out)


def get_segmentation(rc: RenderContext, camera_index: int, seg_out: torch.Tensor) -> None:
  """The geom id per pixel (-1: background) of the context's camera `camera_index` as int32 (nworld, H, W)."""
  px = _view(rc, camera_index, "seg", seg_out, (), torch.int32, "get_segmentation")
  seg_out.copy_(px)
