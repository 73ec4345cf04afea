"""A float64 numpy ray caster: the yardstick of tests/test_ray.py and tests/test_gpu_ray.py.

Written for the tests, vectorised over rays, one geom at a time.  Where an independent method is cheap it is
used instead of the device's: Moller-Trumbore for triangles, the heightfield as a base box, every surface
triangle and wall quads (two triangles each) up to the elevation profile, the capsule's normal from the
nearest point of its axis segment, the box's from the hit point.  It takes the geom frames as arguments: the
GPU tests pass the device's own d.geom_xpos / d.geom_xmat, so that only the ray code is under test.

Conventions (MuJoCo's mj_ray, as mujoco_warp keeps them): dist is in units of |vec|; planes are hit from the
front only and inside the rendered rectangle; an origin inside a solid hits the far side; mesh triangles are
two-sided with the normal of their winding, normalize((v0 - v2) x (v1 - v2)); a miss is dist -1, geomid -1,
normal 0; equal distances go to the lowest geom id.
"""

import numpy as np

MINVAL = 1e-15
PLANE, HFIELD, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX, MESH = range(8)


def _unit(v):
  n = np.linalg.norm(v, axis=-1, keepdims=True)
  return np.where(n > 0, v / np.where(n > 0, n, 1.0), 0.0)


def _quad(a, b, c):
  """Roots of a x^2 + 2 b x + c: (nearest non-negative root or -1, x0, x1)."""
  det = b * b - a * c
  ok = det >= MINVAL
  s = np.sqrt(np.where(ok, det, 1.0))
  den = 1.0 / np.where(a != 0, a, MINVAL)
  x0 = np.where(ok, (-b - s) * den, -1.0)
  x1 = np.where(ok, (-b + s) * den, -1.0)
  return np.where(x0 >= 0, x0, np.where(x1 >= 0, x1, -1.0)), x0, x1


def _keep_nearer(x, n, sol, nsol, cond=True):
  """(x, n) with the candidate (sol, nsol) taken where it is a hit, allowed by cond, and nearer."""
  take = cond & (sol >= 0) & ((x < 0) | (sol < x))
  return np.where(take, sol, x), np.where(take[:, None], nsol, n)


def _hit(lp, lv, x):
  return lp + np.where(x >= 0, x, 0.0)[:, None] * lv


def plane(lp, lv, size):
  ok = lv[:, 2] <= -MINVAL
  x = -lp[:, 2] / np.where(ok, lv[:, 2], 1.0)
  p = lp[:, :2] + x[:, None] * lv[:, :2]
  inside = ((size[0] <= 0) | (np.abs(p[:, 0]) <= size[0])) & ((size[1] <= 0) | (np.abs(p[:, 1]) <= size[1]))
  x = np.where(ok & (x >= 0) & inside, x, -1.0)
  return x, np.where((x >= 0)[:, None], np.array([0.0, 0.0, 1.0]), 0.0)


def sphere(lp, lv, r):
  x = _quad((lv * lv).sum(-1), (lv * lp).sum(-1), (lp * lp).sum(-1) - r * r)[0]
  return x, np.where((x >= 0)[:, None], _unit(_hit(lp, lv, x)), 0.0)


def capsule(lp, lv, size):
  r, h = size[0], size[1]
  n0 = np.zeros_like(lp)
  x = np.full(len(lp), -1.0)
  sol = _quad(lv[:, 0] ** 2 + lv[:, 1] ** 2, lv[:, 0] * lp[:, 0] + lv[:, 1] * lp[:, 1], lp[:, 0] ** 2 + lp[:, 1] ** 2 - r * r)[0]
  x, _ = _keep_nearer(x, n0, sol, n0, np.abs(lp[:, 2] + sol * lv[:, 2]) <= h)
  for s in (1.0, -1.0):
    ld = lp - np.array([0.0, 0.0, s * h])
    _, x0, x1 = _quad((lv * lv).sum(-1), (lv * ld).sum(-1), (ld * ld).sum(-1) - r * r)
    for xx in (x0, x1):
      x, _ = _keep_nearer(x, n0, xx, n0, s * (lp[:, 2] + xx * lv[:, 2]) >= h)
  # normal: from the nearest point of the axis segment to the hit
  p = _hit(lp, lv, x)
  q = np.zeros_like(p)
  q[:, 2] = np.clip(p[:, 2], -h, h)
  return x, np.where((x >= 0)[:, None], _unit(p - q), 0.0)


def ellipsoid(lp, lv, size):
  s = 1.0 / (size * size)
  x = _quad((s * lv * lv).sum(-1), (s * lv * lp).sum(-1), (s * lp * lp).sum(-1) - 1.0)[0]
  return x, np.where((x >= 0)[:, None], _unit(s * _hit(lp, lv, x)), 0.0)


def cylinder(lp, lv, size):
  r, h = size[0], size[1]
  x = np.full(len(lp), -1.0)
  n = np.zeros_like(lp)
  ok = np.abs(lv[:, 2]) > MINVAL
  for s in (-1.0, 1.0):
    sol = (s * h - lp[:, 2]) / np.where(ok, lv[:, 2], 1.0)
    p = lp[:, :2] + sol[:, None] * lv[:, :2]
    x, n = _keep_nearer(x, n, sol, np.broadcast_to(np.array([0.0, 0.0, s]), lp.shape), ok & ((p * p).sum(-1) <= r * r))
  sol = _quad(lv[:, 0] ** 2 + lv[:, 1] ** 2, lv[:, 0] * lp[:, 0] + lv[:, 1] * lp[:, 1], lp[:, 0] ** 2 + lp[:, 1] ** 2 - r * r)[0]
  radial = _hit(lp, lv, sol) * np.array([1.0, 1.0, 0.0])
  return _keep_nearer(x, n, sol, _unit(radial), np.abs(lp[:, 2] + sol * lv[:, 2]) <= h)


def box(lp, lv, size, centre=None):
  if centre is not None:
    lp = lp - centre
  x = np.full(len(lp), -1.0)
  for i in range(3):
    ok = np.abs(lv[:, i]) > MINVAL
    j, k = [(1, 2), (0, 2), (0, 1)][i]
    for side in (-1.0, 1.0):
      sol = (side * size[i] - lp[:, i]) / np.where(ok, lv[:, i], 1.0)
      pj, pk = lp[:, j] + sol * lv[:, j], lp[:, k] + sol * lv[:, k]
      hit = ok & (sol >= 0) & (np.abs(pj) <= size[j]) & (np.abs(pk) <= size[k])
      x = np.where(hit & ((x < 0) | (sol < x)), sol, x)
  # normal: the face the hit point lies on (the coordinate nearest to its face)
  p = _hit(lp, lv, x)
  axis = np.argmin(np.abs(np.abs(p) - size), axis=1)
  n = np.zeros_like(lp)
  rows = np.arange(len(lp))
  n[rows, axis] = np.sign(p[rows, axis])
  return x, np.where((x >= 0)[:, None], n, 0.0)


def triangle(lp, lv, v0, v1, v2):
  """Moller-Trumbore, two-sided, edges included; the normal is the winding's, normalize((v0 - v2) x (v1 - v2))."""
  e1, e2 = v1 - v0, v2 - v0
  p = np.cross(lv, e2)
  det = p @ e1
  ok = np.abs(det) > MINVAL
  inv = 1.0 / np.where(ok, det, 1.0)
  t = lp - v0
  u = (t * p).sum(-1) * inv
  q = np.cross(t, e1)
  v = (lv * q).sum(-1) * inv
  dist = (q @ e2) * inv
  x = np.where(ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (dist >= 0), dist, -1.0)
  return x, np.broadcast_to(_unit(np.cross(v0 - v2, v1 - v2)), lp.shape)


def mesh(lp, lv, vert, face, aabb):
  """Every triangle of the face list (Moller-Trumbore over rays x faces at once), the nearest hit; equal
  distances go to the lowest face.  Rays that miss the (slightly grown) box of geom_aabb are left out, which
  loses nothing: the box encloses every vertex."""
  assert np.all(np.abs(vert - aabb[:3]) <= aabb[3:] * (1 + 1e-9) + 1e-12), "geom_aabb does not enclose the mesh"
  x = np.full(len(lp), -1.0)
  n = np.zeros_like(lp)
  cand = np.nonzero(box(lp, lv, aabb[3:] * (1 + 1e-6) + 1e-9, centre=aabb[:3])[0] >= 0)[0]
  if len(cand) == 0 or len(face) == 0:
    return x, n
  v0, v1, v2 = vert[face[:, 0]], vert[face[:, 1]], vert[face[:, 2]]
  e1, e2 = v1 - v0, v2 - v0
  p = np.cross(lv[cand, None, :], e2[None, :, :])
  det = (p * e1[None]).sum(-1)
  ok = np.abs(det) > MINVAL
  inv = 1.0 / np.where(ok, det, 1.0)
  t = lp[cand, None, :] - v0[None, :, :]
  u = (t * p).sum(-1) * inv
  q = np.cross(t, e1[None])
  v = (lv[cand, None, :] * q).sum(-1) * inv
  dist = (q * e2[None]).sum(-1) * inv
  dist = np.where(ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (dist >= 0), dist, np.inf)
  f = dist.argmin(axis=1)
  best = dist[np.arange(len(cand)), f]
  hit = ~np.isinf(best)
  x[cand[hit]] = best[hit]
  n[cand[hit]] = _unit(np.cross(v0 - v2, v1 - v2))[f[hit]]
  return x, n


def hfield(lp, lv, hsize, nrow, ncol, data):
  sx, sy, top, base = (float(v) for v in hsize)
  x, n = box(lp, lv, np.array([sx, sy, base / 2]), centre=np.array([0.0, 0.0, -base / 2]))
  dx, dy = 2 * sx / (ncol - 1), 2 * sy / (nrow - 1)
  H = np.asarray(data, dtype=np.float64).reshape(nrow, ncol) * top

  def P(r, c):
    return np.array([dx * c - sx, dy * r - sy, H[r, c]])

  def Z(p):
    return np.array([p[0], p[1], 0.0])

  for r in range(nrow - 1):
    for c in range(ncol - 1):
      for tri in ((P(r, c), P(r, c + 1), P(r + 1, c + 1)), (P(r, c), P(r + 1, c + 1), P(r + 1, c))):
        sol, nsol = triangle(lp, lv, *tri)
        x, n = _keep_nearer(x, n, sol, nsol)
  # side walls: the quad under each edge segment of the profile, from z = 0 up to it; normal = outward
  walls = [(P(r, c), P(r + 1, c), np.array([-1.0 if c == 0 else 1.0, 0.0, 0.0])) for r in range(nrow - 1) for c in (0, ncol - 1)]
  walls += [(P(r, c), P(r, c + 1), np.array([0.0, -1.0 if r == 0 else 1.0, 0.0])) for c in range(ncol - 1) for r in (0, nrow - 1)]
  for a, b, out in walls:
    for tri in ((Z(a), Z(b), b), (Z(a), b, a)):
      sol, _ = triangle(lp, lv, *tri)
      x, n = _keep_nearer(x, n, sol, np.broadcast_to(out, lp.shape))
  return x, n


def eliminated(mjm, geomgroup=None, flg_static=True, geom_rgba=None, mat_rgba=None):
  """(ngeom,) bool: geoms no ray may hit (transparent, filtered group, static); bodyexclude is per ray."""
  rgba = np.asarray(mjm.geom_rgba if geom_rgba is None else geom_rgba, dtype=np.float64).reshape(-1, 4)
  mrgba = np.asarray(mjm.mat_rgba if mat_rgba is None else mat_rgba, dtype=np.float64).reshape(-1, 4)
  matid = np.asarray(mjm.geom_matid)
  out = np.where(matid < 0, rgba[:, 3] == 0, mrgba[np.maximum(matid, 0), 3] == 0 if len(mrgba) else False)
  if not flg_static:
    out = out | (np.asarray(mjm.body_weldid)[np.asarray(mjm.geom_bodyid)] == 0)
  if geomgroup is not None and not all(int(g) == -1 for g in geomgroup):
    gg = np.asarray([int(g) for g in geomgroup])
    out = out | (gg[np.clip(np.asarray(mjm.geom_group), 0, 5)] == 0)
  return out


def cast_all(mjm, xpos, xmat, pnt, vec, skip=None):
  """Every ray against every geom: dist (ngeom, n) (-1: miss), world-frame normals (ngeom, n, 3).
  xpos (ngeom, 3), xmat (ngeom, 3, 3): the geom frames; skip: (ngeom,) bool geoms left out."""
  pnt, vec = np.asarray(pnt, dtype=np.float64), np.asarray(vec, dtype=np.float64)
  ng = int(mjm.ngeom)
  dist = np.full((ng, len(pnt)), -1.0)
  nrm = np.zeros((ng, len(pnt), 3))
  for g in range(ng):
    if skip is not None and skip[g]:
      continue
    R = np.asarray(xmat[g], dtype=np.float64).reshape(3, 3)
    lp, lv = (pnt - np.asarray(xpos[g], dtype=np.float64)) @ R, vec @ R
    t, size = int(mjm.geom_type[g]), np.asarray(mjm.geom_size[g], dtype=np.float64)
    if t == PLANE:
      x, n = plane(lp, lv, size)
    elif t == SPHERE:
      x, n = sphere(lp, lv, size[0])
    elif t == CAPSULE:
      x, n = capsule(lp, lv, size)
    elif t == ELLIPSOID:
      x, n = ellipsoid(lp, lv, size)
    elif t == CYLINDER:
      x, n = cylinder(lp, lv, size)
    elif t == BOX:
      x, n = box(lp, lv, size)
    elif t == MESH:
      i = int(mjm.geom_dataid[g])
      va, fa = int(mjm.mesh_vertadr[i]), int(mjm.mesh_faceadr[i])
      vert = np.asarray(mjm.mesh_vert, dtype=np.float64).reshape(-1, 3)[va : va + int(mjm.mesh_vertnum[i])]
      face = np.asarray(mjm.mesh_face).reshape(-1, 3)[fa : fa + int(mjm.mesh_facenum[i])]
      x, n = mesh(lp, lv, vert, face, np.asarray(mjm.geom_aabb, dtype=np.float64).reshape(-1, 6)[g])
    elif t == HFIELD:
      i = int(mjm.geom_dataid[g])
      nrow, ncol, adr = int(mjm.hfield_nrow[i]), int(mjm.hfield_ncol[i]), int(mjm.hfield_adr[i])
      x, n = hfield(lp, lv, np.asarray(mjm.hfield_size).reshape(-1, 4)[i], nrow, ncol, np.asarray(mjm.hfield_data).reshape(-1)[adr : adr + nrow * ncol])
    else:
      raise NotImplementedError(t)
    dist[g] = x
    nrm[g] = np.where((x >= 0)[:, None], n @ R.T, 0.0)
  return dist, nrm


def nearest(dist, nrm, geom_bodyid=None, bodyexclude=None):
  """First hit of each ray: geomid (n,), dist (n,), normal (n, 3), gap (n,) to the second-nearest geom
  (inf when fewer than two geoms are hit).  bodyexclude: (n,) body ids whose geoms the ray skips."""
  dd = np.where(dist < 0, np.inf, dist)
  if bodyexclude is not None:
    dd = np.where(np.asarray(geom_bodyid)[:, None] == np.asarray(bodyexclude)[None, :], np.inf, dd)
  n = dd.shape[1]
  if dd.shape[0] == 0:
    return np.full(n, -1), np.full(n, -1.0), np.zeros((n, 3)), np.full(n, np.inf)
  g = dd.argmin(0)  # the first minimum: the lowest geom id among equal distances
  x = dd[g, np.arange(n)]
  srt = np.sort(dd, axis=0)
  second = srt[1] if dd.shape[0] > 1 else np.full(n, np.inf)
  gap = np.where(np.isinf(second), np.inf, second - np.where(np.isinf(srt[0]), 0.0, srt[0]))
  miss = np.isinf(x)
  return np.where(miss, -1, g), np.where(miss, -1.0, x), np.where(miss[:, None], 0.0, nrm[g, np.arange(n)]), gap


def cast(mjm, xpos, xmat, pnt, vec, geomgroup=None, flg_static=True, bodyexclude=None, geom_rgba=None, mat_rgba=None):
  """rays() of one world: geomid, dist, normal, decisive (each per ray).

  A ray is decisive when its best and second-best geom distances differ by more than 1e-3 and six perturbed
  copies (one component of vec moved by +-1e-4 |vec|) give the same geom id, a distance within
  1e-2 max(1, dist) and a normal within 1e-2.  Only decisive rays are fit to compare with fp32."""
  pnt, vec = np.asarray(pnt, dtype=np.float64), np.asarray(vec, dtype=np.float64)
  skip = eliminated(mjm, geomgroup, flg_static, geom_rgba, mat_rgba)
  body = np.asarray(mjm.geom_bodyid)
  g, x, n, gap = nearest(*cast_all(mjm, xpos, xmat, pnt, vec, skip), body, bodyexclude)
  ok = ~((gap <= 1e-3) & (g >= 0))
  eps = 1e-4 * np.linalg.norm(vec, axis=1)
  for k in range(3):
    for s in (-1.0, 1.0):
      v2 = vec.copy()
      v2[:, k] += s * eps
      g2, x2, n2, _ = nearest(*cast_all(mjm, xpos, xmat, pnt, v2, skip), body, bodyexclude)
      ok &= (g2 == g) & (np.abs(x2 - x) <= 1e-2 * np.maximum(1.0, x)) & (np.abs(n2 - n).max(axis=1) <= 1e-2)
  return g, x, n, ok
