"""A float64 numpy renderer: the yardstick of tests/test_render.py and tests/test_gpu_render.py.

It makes the pixel rays by the reference's compute_ray formulas, finds the first hits with tests/ray_ref.py
(cast_all / nearest) under its own skip mask -- the group rule only: a geom is drawn iff its group is enabled,
alpha plays no part -- and shades with the reference's hemispheric ambient term, its three light kinds and
its shadow rule.  Like ray_ref it takes the frames as arguments, so the GPU tests pass what the device computed
and only the render code is under test.

A pixel is decisive when its primary ray is decisive by the rule of ray_ref.cast (first and second geom more
than 1e-3 apart; the same geom, a distance within 1e-2 max(1, dist) and a normal within 1e-2 under six 1e-4
perturbations of the direction) and, with shadows, no shadow ray's occlusion changes under the same six
perturbations of its direction.  Only decisive pixels are fit to compare with fp32.
"""

import numpy as np

from tests import ray_ref

AMB_HI, AMB_LO = np.array([0.4, 0.4, 0.45]), np.array([0.1, 0.1, 0.12])
BACKGROUND = (25, 25, 51)
BACKGROUND_PACKED = 255 << 24 | 25 << 16 | 25 << 8 | 51
SPOT, DIRECTIONAL, POINT = 0, 1, 2


def pixel_rays(fovy, sensorsize, intrinsic, W, H):
  """Directions in the camera frame, (H * W, 3), pixel (px, py) at row py * W + px (render_util.py:67-125, znear 1)."""
  aspect = W / H
  sensor_w, sensor_h = float(sensorsize[0]), float(sensorsize[1])
  if sensor_h != 0.0:
    fx, fy, cx, cy = (float(v) for v in intrinsic)
    sensor_aspect = sensor_w / sensor_h
    if aspect > sensor_aspect:
      sensor_h = sensor_w / aspect
    elif aspect < sensor_aspect:
      sensor_w = sensor_h * aspect
    left, right = -(sensor_w * 0.5 - cx) / fx, (sensor_w * 0.5 + cx) / fx
    top, bottom = (sensor_h * 0.5 - cy) / fy, -(sensor_h * 0.5 + cy) / fy
  else:
    half_h = np.tan(0.5 * np.deg2rad(float(fovy)))
    half_w = half_h * aspect
    left, right, top, bottom = -half_w, half_w, half_h, -half_h
  py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
  u, v = (px.ravel() + 0.5) / W, (py.ravel() + 0.5) / H
  d = np.stack([left + (right - left) * u, top + (bottom - top) * v, -np.ones(W * H)], axis=1)
  return d / np.linalg.norm(d, axis=1, keepdims=True)


def drawn_skip(mjm, groups):
  """(ngeom,) bool: geoms not drawn -- exactly those whose group is not one of `groups`."""
  return ~np.isin(np.asarray(mjm.geom_group), [int(g) for g in groups])


def _perturbed(vec):
  eps = 1e-4 * np.linalg.norm(vec, axis=1)
  for k in range(3):
    for s in (-1.0, 1.0):
      v2 = vec.copy()
      v2[:, k] += s * eps
      yield v2


def cast(mjm, xpos, xmat, pnt, vec, skip):
  """ray_ref.cast with a given skip mask: geomid, dist, normal, decisive."""
  g, x, n, gap = ray_ref.nearest(*ray_ref.cast_all(mjm, xpos, xmat, pnt, vec, skip))
  ok = ~((gap <= 1e-3) & (g >= 0))
  for v2 in _perturbed(vec):
    g2, x2, n2, _ = ray_ref.nearest(*ray_ref.cast_all(mjm, xpos, xmat, pnt, v2, skip))
    ok &= (g2 == g) & (np.abs(x2 - x) <= 1e-2 * np.maximum(1.0, x)) & (np.abs(n2 - n).max(axis=1) <= 1e-2)
  return g, x, n, ok


def occluded(mjm, xpos, xmat, pnt, vec, skip, limit):
  """(n,) bool: some drawn geom lies at 0 <= dist < limit along the ray."""
  dist, _ = ray_ref.cast_all(mjm, xpos, xmat, pnt, vec, skip)
  return ((dist >= 0) & (dist < limit[None, :])).any(axis=0)


def shade(mjm, xpos, xmat, g, hitp, normal, light_xpos, light_xdir, light_type, light_active, light_castshadow, skip, use_shadows=False,
          geom_rgba=None, mat_rgba=None):
  """Colours (n, 3) in [0, 1] of the hits (g >= 0; other rows are zero) and the pixels whose shadows are decisive."""
  rgba = np.asarray(mjm.geom_rgba if geom_rgba is None else geom_rgba, dtype=np.float64).reshape(-1, 4)
  mrgba = np.asarray(mjm.mat_rgba if mat_rgba is None else mat_rgba, dtype=np.float64).reshape(-1, 4)
  hit = g >= 0
  gi = np.where(hit, g, 0)
  matid = np.asarray(mjm.geom_matid)[gi]
  base = np.where((matid >= 0)[:, None], mrgba[np.maximum(matid, 0), :3] if len(mrgba) else 0.0, rgba[gi, :3])
  ln = np.linalg.norm(normal, axis=1, keepdims=True)
  n = np.where(ln > 0, normal / np.where(ln > 0, ln, 1.0), np.array([0.0, 0.0, 1.0]))
  h = 0.5 * (n[:, 2:3] + 1.0)
  res = 0.5 * base * (AMB_HI * h + AMB_LO * (1.0 - h))
  ok = np.ones(len(g), dtype=bool)
  for l in range(len(light_type)):
    if not light_active[l]:
      continue
    if light_type[l] == DIRECTIONAL:
      L = np.broadcast_to(-np.asarray(light_xdir[l], dtype=np.float64) / np.linalg.norm(light_xdir[l]), hitp.shape).copy()
      r = np.full(len(g), np.inf)
      att = np.ones(len(g))
    else:
      L = np.asarray(light_xpos[l], dtype=np.float64) - hitp
      r = np.linalg.norm(L, axis=1)
      L = L / np.where(r > 0, r, 1.0)[:, None]
      att = 1.0 / (1.0 + 0.02 * r * r)
      if light_type[l] == SPOT:
        sd = np.asarray(light_xdir[l], dtype=np.float64) / np.linalg.norm(light_xdir[l])
        att = att * np.clip((-(L @ sd) - 0.85) / 0.10, 0.0, 1.0)
    ndotl = np.maximum(0.0, (normal * L).sum(-1))
    visible = np.ones(len(g))
    if use_shadows and light_castshadow[l]:
      lit = hit & (ndotl > 0)
      idx = np.nonzero(lit)[0]
      if len(idx):
        origin = hitp[idx] + 1e-4 * normal[idx]
        limit = np.full(len(idx), 1e8) if light_type[l] == DIRECTIONAL else r[idx] - 1e-3
        occ = occluded(mjm, xpos, xmat, origin, L[idx], skip, limit)
        for v2 in _perturbed(L[idx]):
          ok[idx] &= occluded(mjm, xpos, xmat, origin, v2, skip, limit) == occ
        visible[idx[occ]] = 0.3
    res = res + base * (ndotl * att * visible)[:, None]
  return np.where(hit[:, None], np.clip(res, 0.0, 1.0), 0.0), ok


def render(mjm, xpos, xmat, cam_xpos, cam_xmat, fovy, sensorsize, intrinsic, W, H, light_xpos, light_xdir, groups=(0, 1, 2), use_shadows=False,
           geom_rgba=None, mat_rgba=None, light_type=None, light_active=None, light_castshadow=None):
  """One camera of one world.  Returns seg (H*W,) int (-1 background), depth (H*W,) (0 background), rgb (H*W, 3)
  ints (the background colour where nothing is hit), ok (H*W,) bool decisive."""
  local = pixel_rays(fovy, sensorsize, intrinsic, W, H)
  vec = local @ np.asarray(cam_xmat, dtype=np.float64).reshape(3, 3).T
  pnt = np.broadcast_to(np.asarray(cam_xpos, dtype=np.float64), vec.shape).copy()
  skip = drawn_skip(mjm, groups)
  g, x, n, ok = cast(mjm, xpos, xmat, pnt, vec, skip)
  hit = g >= 0
  depth = np.where(hit, x * -local[:, 2], 0.0)
  nl = len(np.asarray(light_xpos).reshape(-1, 3))
  lt = np.asarray(mjm.light_type if light_type is None else light_type).reshape(-1)[:nl]
  la = np.asarray(mjm.light_active if light_active is None else light_active).reshape(-1)[:nl]
  lc = np.asarray(mjm.light_castshadow if light_castshadow is None else light_castshadow).reshape(-1)[:nl]
  hitp = pnt + vec * np.where(hit, x, 0.0)[:, None]
  col, sok = shade(mjm, xpos, xmat, g, hitp, n, np.asarray(light_xpos).reshape(-1, 3), np.asarray(light_xdir).reshape(-1, 3), lt, la, lc, skip,
                   use_shadows, geom_rgba, mat_rgba)
  rgb = np.where(hit[:, None], np.floor(col * 255.0).astype(np.int64), np.array(BACKGROUND))
  return g, depth, rgb, ok & sok


def unpack(packed):
  """(..., ) packed int32 pixels -> (..., 4) ints r, g, b, a."""
  p = np.asarray(packed).astype(np.int64) & 0xFFFFFFFF
  return np.stack([(p >> 16) & 0xFF, (p >> 8) & 0xFF, p & 0xFF, (p >> 24) & 0xFF], axis=-1)
