"""Batched ray casting over all geom types (mujoco_warp/_src/ray.py:1168-1312 `ray` / `rays`).

One HIP launch (`mjw_rays`, csrc/mjw_ray.hip) on the Data's stream: for every world and ray the nearest geom
along `pnt + x vec`, x >= 0, at the frames `d.geom_xpos` / `d.geom_xmat` the last position stage left (no
kinematics run here, so it serves dense and sparse models alike).  Without a render context meshes are brute
force over their triangles.  With `rc`, a RenderContext of the same model and nworld (render.py), the launch is
`mjw_rays_bvh`: every mesh is walked through the context's static BVH (bvh.py) with the same result bit for bit.
The trees were built from the host model's vertices, so with a per-world batched `m.mesh_vert` (leading dim > 1)
the call runs the face loop all the same.  Any other `rc` is refused.  Flex elements are not hit (as on the
reference's path without `rc`).
"""

from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from .types import Data, Model


def _ray_model(m: Model) -> _lib.CRayModel:
  """The side struct mjw_ray_model_t from the Model's current tensors (built per call: a caller may have
  replaced geom_rgba / mat_rgba with per-world batches)."""
  ng, nmat, nface = int(m.ngeom), int(m.nmat), int(m.nmeshface)
  chk = lambda name, dtype, *shape: _lib.check_tensor("ray model", "m." + name, getattr(m, name), dtype, m.geom_type.device, shape)
  c = _lib.CRayModel()
  c.ngeom, c.nmat, c.nmeshface = ng, nmat, nface
  c.geom_group = chk("geom_group", torch.int32, ng).data_ptr()
  c.geom_matid = chk("geom_matid", torch.int32, ng).data_ptr()
  rgba, mat = chk("geom_rgba", torch.float32, None, ng, 4), chk("mat_rgba", torch.float32, None, nmat, 4)
  if rgba.shape[0] < 1 or mat.shape[0] < 1:
    raise ValueError("ray model: m.geom_rgba / m.mat_rgba need a leading batch dimension of at least 1")
  c.geom_rgba, c.geom_rgba_nb = rgba.data_ptr(), int(rgba.shape[0])
  c.mat_rgba, c.mat_rgba_nb = mat.data_ptr(), int(mat.shape[0])
  c.mesh_face = chk("mesh_face", torch.int32, nface, 3).data_ptr()
  c.mesh_faceadr = chk("mesh_faceadr", torch.int32, None).data_ptr()
  c.mesh_facenum = chk("mesh_facenum", torch.int32, None).data_ptr()
  c._keep = (rgba, mat)  # the tensors whose pointers the struct holds
  return c


def rays(m: Model, d: Data, pnt: torch.Tensor, vec: torch.Tensor, geomgroup: Optional[Sequence[int]], flg_static: bool,
         bodyexclude: torch.Tensor, dist: torch.Tensor, geomid: torch.Tensor, normal: torch.Tensor, rc=None) -> None:
  """Ray intersections for every world and ray (ray.py:1212-1312).

  pnt, vec: float32 (nb, nray, 3), nb = 1 or nworld (world w reads row w % nb); vec is not normalised and
  `dist` is in units of |vec|.  geomgroup: None or six ints (all -1 / None: no filter; else a geom is skipped
  when geomgroup[clamp(geom_group, 0, 5)] == 0).  flg_static False skips geoms of bodies welded to the world.
  bodyexclude: int32 (nray,), geoms of that body are skipped (-1: none).  Geoms with alpha 0 (their
  material's when they have one, else their own rgba) are skipped.  Outputs: dist float32 (nworld, nray),
  geomid int32 (nworld, nray), normal float32 (nworld, nray, 3); a miss gives -1, -1, 0, and equal distances
  go to the lowest geom id.  rc: None, or a RenderContext made for this model and nworld, whose mesh BVHs then
  replace the loop over every mesh face (same results); a context of another model or nworld raises ValueError."""
  bvh = None
  if rc is not None:
    from .types import RenderContext

    if not isinstance(rc, RenderContext):
      raise NotImplementedError("rays: rc must be None or a RenderContext from create_render_context (its mesh BVHs are walked)")
    from .render import _cbvh, _made_for

    _made_for("rays", rc, m, d)
    bvh = _cbvh(rc, m, d, "rays")
  dev = d.qpos.device
  nworld = int(d.nworld)
  chk = lambda name, t, dtype, *shape: _lib.check_tensor("rays", name, t, dtype, dev, shape)
  nb, nray = (int(n) for n in chk("pnt", pnt, torch.float32, None, None, 3).shape[:2])
  nbv = int(chk("vec", vec, torch.float32, None, nray, 3).shape[0])
  if nb not in (1, nworld) or nbv not in (1, nworld):
    raise ValueError(f"rays: pnt / vec batch must be 1 or nworld = {nworld}, got {nb} / {nbv}")
  chk("bodyexclude", bodyexclude, torch.int32, nray)
  chk("dist", dist, torch.float32, nworld, nray)
  chk("geomid", geomid, torch.int32, nworld, nray)
  chk("normal", normal, torch.float32, nworld, nray, 3)
  group = None
  if geomgroup is not None:
    g = [int(x) for x in geomgroup]
    if len(g) != 6:
      raise ValueError(f"rays: geomgroup must be None or six ints, got {len(g)}")
    group = (ctypes.c_int * 6)(*g)
  rm = _ray_model(m)
  if nray == 0:
    return
  from .forward import _stream
  from .io import cdata, cmodel

  L = _lib.lib()
  args = (cmodel(m), cdata(d), ctypes.byref(rm), pnt.data_ptr(), nb, vec.data_ptr(), nbv, nray, group,
          int(bool(flg_static)), bodyexclude.data_ptr(), dist.data_ptr(), geomid.data_ptr(), normal.data_ptr())
  if bvh is None:
    _lib.check(L.mjw_rays(*args, _stream(d)), "mjw_rays")
  else:
    _lib.check(L.mjw_rays_bvh(*args, ctypes.byref(bvh), _stream(d)), "mjw_rays_bvh")


def ray(m: Model, d: Data, pnt: torch.Tensor, vec: torch.Tensor, geomgroup: Optional[Sequence[int]] = None, flg_static: bool = True,
        bodyexclude: int = -1, rc=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
  """One ray per world (ray.py:1168-1209): pnt, vec of shape (nb, 1, 3) with nb = 1 (the same ray in every
  world) or nworld.  Returns dist (nworld, 1), geomid (nworld, 1), normal (nworld, 1, 3).  rc: as for `rays`."""
  if rc is not None:
    from .types import RenderContext

    if not isinstance(rc, RenderContext):
      raise NotImplementedError("ray: rc must be None or a RenderContext from create_render_context (its mesh BVHs are walked)")
  if not isinstance(pnt, torch.Tensor) or pnt.dim() != 3 or pnt.shape[1] != 1:
    raise ValueError("ray: pnt must have shape (nb, 1, 3)")
  dev = d.qpos.device
  nworld = int(d.nworld)
  excl = torch.full((1,), int(bodyexclude), dtype=torch.int32, device=dev)
  dist = torch.empty((nworld, 1), dtype=torch.float32, device=dev)
  geomid = torch.empty((nworld, 1), dtype=torch.int32, device=dev)
  normal = torch.empty((nworld, 1, 3), dtype=torch.float32, device=dev)
  rays(m, d, pnt, vec, geomgroup, flg_static, excl, dist, geomid, normal, rc=rc)
  return dist, geomid, normal
