"""A float64 numpy yardstick for textured rendering (tests/test_texture.py, tests/test_gpu_texture.py).

It wraps tests/render_ref.py: the same pixel rays, first hits (`cast`) and light loop (`shade`), with a base colour per
pixel: mat_rgba / geom_rgba times, where the rule of the render kernel gives one, a bilinear sample of the material's
2D texture.  The rule: the geom has a valid material, role 1 of mat_texid names a 2D texture with data, and the geom
is a plane (uv = the hit in the plane's frame, x and y) or a mesh with texture coordinates (uv = the barycentric mean
of the hit face's three uvs).  Every other pixel keeps its base colour.

Sampling: s = frac(uv * texrepeat); x = s.x W - 0.5, y = s.y H - 0.5; the four texels around (floor x, floor y), indices
modulo W and H, weights x - floor x and y - floor y, texel = byte / 255, row y of the texture is v.

A pixel is decisive by render_ref's rule and, on a textured mesh, only if the six 1e-4-perturbed rays hit the same face.
"""

import numpy as np

from tests import ray_ref, render_ref

PLANE, MESH = 0, 7
ROLE_RGB = 1
_SCALE = 16.0  # the light loop is run on a base colour of 1 / 16 (exact in binary) so that its clip to [0, 1] never acts


def texture(mjm, i):
  """(H, W, 3) uint8 of the model's 2D texture i, or None for one without data or of another type."""
  if i < 0 or i >= int(mjm.ntex) or int(mjm.tex_type[i]) != 0 or int(mjm.tex_adr[i]) < 0:
    return None
  w, h, a = int(mjm.tex_width[i]), int(mjm.tex_height[i]), int(mjm.tex_adr[i])
  return np.asarray(mjm.tex_data[a : a + 3 * w * h], dtype=np.uint8).reshape(h, w, 3)


def sample(tex, uv, repeat=(1.0, 1.0)):
  """Bilinear, repeating sample of tex (H, W, 3) uint8 at uv (n, 2): (n, 3) float64 in [0, 1]."""
  tex = np.asarray(tex, dtype=np.float64) / 255.0
  H, W = tex.shape[:2]
  s = np.asarray(uv, dtype=np.float64).reshape(-1, 2) * np.asarray(repeat, dtype=np.float64)
  s = s - np.floor(s)
  x, y = s[:, 0] * W - 0.5, s[:, 1] * H - 0.5
  x0, y0 = np.floor(x), np.floor(y)
  fx, fy = (x - x0)[:, None], (y - y0)[:, None]
  ix0, iy0 = x0.astype(np.int64) % W, y0.astype(np.int64) % H
  ix1, iy1 = (ix0 + 1) % W, (iy0 + 1) % H
  return (1 - fy) * ((1 - fx) * tex[iy0, ix0] + fx * tex[iy0, ix1]) + fy * ((1 - fx) * tex[iy1, ix0] + fx * tex[iy1, ix1])


def mesh_face(mjm, g, xpos, xmat, pnt, vec):
  """The face of mesh geom g each ray hits first (Moller-Trumbore; the lowest face among equal distances; -1: none) and
  the barycentric weights (n, 3) of the hit over the face's three corners."""
  i = int(mjm.geom_dataid[g])
  va, fa = int(mjm.mesh_vertadr[i]), int(mjm.mesh_faceadr[i])
  vert = np.asarray(mjm.mesh_vert, dtype=np.float64).reshape(-1, 3)[va : va + int(mjm.mesh_vertnum[i])]
  face = np.asarray(mjm.mesh_face).reshape(-1, 3)[fa : fa + int(mjm.mesh_facenum[i])]
  R = np.asarray(xmat[g], dtype=np.float64).reshape(3, 3)
  lp, lv = (pnt - np.asarray(xpos[g], dtype=np.float64)) @ R, vec @ R
  v0, v1, v2 = vert[face[:, 0]], vert[face[:, 1]], vert[face[:, 2]]
  e1, e2 = v1 - v0, v2 - v0
  p = np.cross(lv[:, None, :], e2[None])
  det = (p * e1[None]).sum(-1)
  ok = np.abs(det) > ray_ref.MINVAL
  inv = 1.0 / np.where(ok, det, 1.0)
  t = lp[:, None, :] - v0[None]
  u = (t * p).sum(-1) * inv
  q = np.cross(t, e1[None])
  v = (lv[:, None, :] * q).sum(-1) * inv
  dist = (q * e2[None]).sum(-1) * inv
  dist = np.where(ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (dist >= 0), dist, np.inf)
  f = dist.argmin(axis=1)
  r = np.arange(len(lp))
  hit = ~np.isinf(dist[r, f])
  bary = np.stack([1.0 - u[r, f] - v[r, f], u[r, f], v[r, f]], axis=1)
  return np.where(hit, f, -1), np.where(hit[:, None], bary, 0.0)


def render(mjm, xpos, xmat, cam_xpos, cam_xmat, fovy, sensorsize, intrinsic, W, H, light_xpos, light_xdir, groups=(0, 1, 2), use_shadows=False,
           geom_rgba=None, mat_rgba=None, mat_texid=None, mat_texrepeat=None, use_textures=True, light_type=None, light_active=None,
           light_castshadow=None):
  """One camera of one world.  Returns seg (H*W,), depth (H*W,), rgb (H*W, 3) ints, ok (H*W,) decisive, face (H*W,)
  (the hit face of a textured mesh pixel, else -1), uv (H*W, 2) (nan where the pixel takes no texel)."""
  local = render_ref.pixel_rays(fovy, sensorsize, intrinsic, W, H)
  vec = local @ np.asarray(cam_xmat, dtype=np.float64).reshape(3, 3).T
  pnt = np.broadcast_to(np.asarray(cam_xpos, dtype=np.float64), vec.shape).copy()
  skip = render_ref.drawn_skip(mjm, groups)
  g, x, n, ok = render_ref.cast(mjm, xpos, xmat, pnt, vec, skip)
  hit = g >= 0
  depth = np.where(hit, x * -local[:, 2], 0.0)
  hitp = pnt + vec * np.where(hit, x, 0.0)[:, None]

  rgba = np.asarray(mjm.geom_rgba if geom_rgba is None else geom_rgba, dtype=np.float64).reshape(-1, 4)
  mrgba = np.asarray(mjm.mat_rgba if mat_rgba is None else mat_rgba, dtype=np.float64).reshape(-1, 4)
  texid = np.asarray(mjm.mat_texid if mat_texid is None else mat_texid).reshape(-1, 10)
  texrep = np.asarray(mjm.mat_texrepeat if mat_texrepeat is None else mat_texrepeat, dtype=np.float64).reshape(-1, 2)
  gi = np.where(hit, g, 0)
  matid = np.asarray(mjm.geom_matid)[gi]
  base = np.where((matid >= 0)[:, None], mrgba[np.maximum(matid, 0), :3] if len(mrgba) else 0.0, rgba[gi, :3])
  base = np.where(hit[:, None], base, 0.0)
  face, uv = np.full(len(g), -1), np.full((len(g), 2), np.nan)
  if use_textures:
    for gg in np.unique(g[hit]):
      mat = int(mjm.geom_matid[gg])
      if mat < 0:
        continue
      tex = texture(mjm, int(texid[mat, ROLE_RGB]))
      gtype = int(mjm.geom_type[gg])
      if tex is None or gtype not in (PLANE, MESH):
        continue
      idx = np.nonzero(g == gg)[0]
      if gtype == PLANE:
        R = np.asarray(xmat[gg], dtype=np.float64).reshape(3, 3)
        uv[idx] = ((hitp[idx] - np.asarray(xpos[gg], dtype=np.float64)) @ R)[:, :2]
      else:
        mesh = int(mjm.geom_dataid[gg])
        tadr = int(mjm.mesh_texcoordadr[mesh])
        if tadr < 0:
          continue
        f, bary = mesh_face(mjm, gg, xpos, xmat, pnt[idx], vec[idx])
        assert np.all(f >= 0), "a pixel whose first hit is the mesh names no face"
        for v2 in render_ref._perturbed(vec[idx]):
          ok[idx] &= mesh_face(mjm, gg, xpos, xmat, pnt[idx], v2)[0] == f
        ftc = np.asarray(mjm.mesh_facetexcoord).reshape(-1, 3)[int(mjm.mesh_faceadr[mesh]) + f]
        tc = np.asarray(mjm.mesh_texcoord, dtype=np.float64).reshape(-1, 2)[tadr + ftc]  # (n, 3, 2)
        uv[idx] = (bary[:, :, None] * tc).sum(axis=1)
        face[idx] = f
      base[idx] = base[idx] * sample(tex, uv[idx], texrep[mat])

  nl = len(np.asarray(light_xpos).reshape(-1, 3))
  lt = np.asarray(mjm.light_type if light_type is None else light_type).reshape(-1)[:nl]
  la = np.asarray(mjm.light_active if light_active is None else light_active).reshape(-1)[:nl]
  lc = np.asarray(mjm.light_castshadow if light_castshadow is None else light_castshadow).reshape(-1)[:nl]
  unit_g, unit_m = np.full((int(mjm.ngeom), 4), 1.0 / _SCALE), np.full((max(int(mjm.nmat), 1), 4), 1.0 / _SCALE)
  factor, sok = render_ref.shade(mjm, xpos, xmat, g, hitp, n, np.asarray(light_xpos).reshape(-1, 3), np.asarray(light_xdir).reshape(-1, 3), lt, la, lc,
                                 skip, use_shadows, unit_g, unit_m)
  assert factor.max(initial=0.0) < 1.0, "the light loop clipped: too many lights for the 1 / 16 base"
  col = np.clip(base * factor * _SCALE, 0.0, 1.0)
  rgb = np.where(hit[:, None], np.floor(col * 255.0).astype(np.int64), np.array(render_ref.BACKGROUND))
  return g, depth, rgb, ok & sok, face, uv
