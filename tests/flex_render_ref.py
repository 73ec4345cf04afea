"""A float64 numpy restatement of the flex surface and of a render with flexes: the yardstick of
tests/test_flex_render.py and tests/test_gpu_flex_render.py.

The surface, per flex f with r = flex_radius[f], from the vertex positions it is given:
  dim 2  vertex normal = normalize(sum over the incident elements, ascending, of normalize((v1 - v0) x (v2 - v0))), zero
         where the sum (or an element's area) is zero; element e gives face 2e = (v0 + r n0, v1 + r n1, v2 + r n2) and
         face 2e + 1 = (v0 - r n0, v2 - r n2, v1 - r n1); boundary fragment s = (i0, i1), an edge with exactly one
         element, in edge order, gives face 2 nelem + 2s = (v0 + r n0, v1 - r n1, v1 + r n1) and the next
         (v1 - r n1, v0 + r n0, v0 - r n0).  smooth = False: the element faces use the element's own normal at all three
         corners, the fragment faces keep the vertex normals.
  dim 3  one face per flex_shell triangle, the vertices themselves
  dim 1  no faces: every edge a capsule of radius r (a sphere when its ends coincide); nothing at r == 0
The hit is the nearest over geoms (tests/ray_ref.py, tests/render_ref.py) and flexes; a flex replaces a geom only when
strictly nearer, the lower flex id wins a tie, within a flex the lower face id.  Segmentation -2, colour flex_rgba,
the normal of a triangle its winding normal turned to face the ray; flexes throw and receive shadows like geoms.

It is written from the definitions with loops over elements and edges and shares no code with the library's tables
(mujoco_warp_amd/bvh.py build_flex_tables).  Decisive pixels follow render_ref: the same object (geom id, or flex id),
a distance within 1e-2 max(1, dist) and a normal within 1e-2 under the six 1e-4 perturbations of the direction, and no
shadow ray's occlusion changing under the same perturbations; as in ray_ref.cast, a pixel whose two nearest objects
(geoms or flexes) lie within 1e-3 of each other is not decisive either.
"""

import numpy as np

from tests import ray_ref, render_ref


def _unit(v):
  n = np.linalg.norm(v)
  return v / n if n > 0 else np.zeros(3)


def fragments(mjm, f):
  """The boundary fragments of dim-2 flex f, local vertex ids: its edges used by exactly one element, in edge order."""
  va, ne = int(mjm.flex_elemdataadr[f]), int(mjm.flex_elemnum[f])
  el = np.asarray(mjm.flex_elem).reshape(-1)[va : va + 3 * ne].reshape(ne, 3)
  ea, n = int(mjm.flex_edgeadr[f]), int(mjm.flex_edgenum[f])
  out = []
  for a, b in np.asarray(mjm.flex_edge).reshape(-1, 2)[ea : ea + n]:
    if sum(1 for t in el if a in t and b in t) == 1:
      out.append((int(a), int(b)))
  return out


def vertex_normals(mjm, f, x):
  """(nvert, 3) of dim-2 flex f from its vertex positions x (nvert, 3)."""
  va, ne = int(mjm.flex_elemdataadr[f]), int(mjm.flex_elemnum[f])
  el = np.asarray(mjm.flex_elem).reshape(-1)[va : va + 3 * ne].reshape(ne, 3)
  out = np.zeros_like(x)
  for t in el:  # ascending element order
    n = _unit(np.cross(x[t[1]] - x[t[0]], x[t[2]] - x[t[0]]))
    for v in t:
      out[v] += n
  return np.array([_unit(v) for v in out]).reshape(-1, 3)


def faces(mjm, f, xpos, smooth=True):
  """(nface, 3, 3) float64: the triangles of flex f (dim 2 or 3) from all flex vertex positions xpos (nflexvert, 3)."""
  dim, r = int(mjm.flex_dim[f]), float(mjm.flex_radius[f])
  x = np.asarray(xpos, dtype=np.float64).reshape(-1, 3)[int(mjm.flex_vertadr[f]) : int(mjm.flex_vertadr[f]) + int(mjm.flex_vertnum[f])]
  out = []
  if dim == 2:
    va, ne = int(mjm.flex_elemdataadr[f]), int(mjm.flex_elemnum[f])
    el = np.asarray(mjm.flex_elem).reshape(-1)[va : va + 3 * ne].reshape(ne, 3)
    vn = vertex_normals(mjm, f, x)
    for t in el:
      n = vn[t] if smooth else np.tile(_unit(np.cross(x[t[1]] - x[t[0]], x[t[2]] - x[t[0]])), (3, 1))
      out.append([x[t[0]] + r * n[0], x[t[1]] + r * n[1], x[t[2]] + r * n[2]])
      out.append([x[t[0]] - r * n[0], x[t[2]] - r * n[2], x[t[1]] - r * n[1]])
    for i0, i1 in fragments(mjm, f):
      out.append([x[i0] + r * vn[i0], x[i1] - r * vn[i1], x[i1] + r * vn[i1]])
      out.append([x[i1] - r * vn[i1], x[i0] + r * vn[i0], x[i0] - r * vn[i0]])
  elif dim == 3:
    sa, ns = int(mjm.flex_shelldataadr[f]), int(mjm.flex_shellnum[f])
    for t in np.asarray(mjm.flex_shell).reshape(-1)[sa : sa + 3 * ns].reshape(ns, 3):
      out.append([x[t[0]], x[t[1]], x[t[2]]])
  return np.asarray(out, dtype=np.float64).reshape(-1, 3, 3)


def _triangles(pnt, vec, tri):
  """Nearest of the triangles (nface, 3, 3) per ray, the lowest face among equal distances: dist (-1 miss) and the
  winding normal turned to face the ray."""
  n = len(pnt)
  x, nrm = np.full(n, -1.0), np.zeros((n, 3))
  for t in tri:
    sol, nt = ray_ref.triangle(pnt, vec, t[0], t[1], t[2])
    x, nrm = ray_ref._keep_nearer(x, nrm, sol, nt)
  flip = (nrm * vec).sum(-1) > 0
  return x, np.where(flip[:, None], -nrm, nrm)


def _capsules(mjm, f, xpos, pnt, vec):
  r = float(mjm.flex_radius[f])
  n = len(pnt)
  x, nrm = np.full(n, -1.0), np.zeros((n, 3))
  if not r > 0:
    return x, nrm
  va, ea, ne = int(mjm.flex_vertadr[f]), int(mjm.flex_edgeadr[f]), int(mjm.flex_edgenum[f])
  for a, b in np.asarray(mjm.flex_edge).reshape(-1, 2)[ea : ea + ne]:
    p0, p1 = xpos[va + a], xpos[va + b]
    mid, ax = 0.5 * (p0 + p1), p1 - p0
    length = np.linalg.norm(ax)
    if length > 0:
      z = ax / length
      e = np.zeros(3)
      e[np.argmin(np.abs(z))] = 1.0
      u = _unit(np.cross(z, e))
      R = np.stack([u, np.cross(z, u), z], axis=1)  # columns: the capsule frame's axes
      sol, nl = ray_ref.capsule((pnt - mid) @ R, vec @ R, np.array([r, 0.5 * length]))
      nw = nl @ R.T
    else:
      sol, nw = ray_ref.sphere(pnt - mid, vec, r)
    x, nrm = ray_ref._keep_nearer(x, nrm, sol, nw)
  return x, nrm


def cast_flex(mjm, xpos, pnt, vec, smooth=True):
  """Every ray against every flex: dist (nflex, n) (-1 miss) and normals (nflex, n, 3)."""
  nflex = int(mjm.nflex)
  xpos = np.asarray(xpos, dtype=np.float64).reshape(-1, 3)
  dist, nrm = np.full((nflex, len(pnt)), -1.0), np.zeros((nflex, len(pnt), 3))
  for f in range(nflex):
    if int(mjm.flex_dim[f]) == 1:
      dist[f], nrm[f] = _capsules(mjm, f, xpos, pnt, vec)
    else:
      dist[f], nrm[f] = _triangles(pnt, vec, faces(mjm, f, xpos, smooth))
  return dist, nrm


def _first(mjm, gxpos, gxmat, fxpos, pnt, vec, skip, smooth):
  """The first hit over geoms and flexes: object (geom id, -2 - flex id for a flex, -1 miss), dist, normal, and whether
  the two nearest objects are more than 1e-3 apart."""
  g, x, n, gap = ray_ref.nearest(*ray_ref.cast_all(mjm, gxpos, gxmat, pnt, vec, skip))
  fd, fn = cast_flex(mjm, fxpos, pnt, vec, smooth)
  obj, ok = g.copy(), ~((gap <= 1e-3) & (g >= 0))
  if len(fd):
    fdd = np.where(fd < 0, np.inf, fd)
    fi = fdd.argmin(0)  # the lowest flex id among equal distances
    fx = fdd[fi, np.arange(len(pnt))]
    take = fx < np.where(g >= 0, x, np.inf)  # strictly nearer than the geom
    both = (g >= 0) & ~np.isinf(fx)
    ok &= ~(both & (np.abs(fx - np.where(g >= 0, x, 0.0)) <= 1e-3))
    srt = np.sort(fdd, axis=0)
    if len(fd) > 1:
      two = ~np.isinf(srt[1])
      ok &= ~(two & (np.where(two, srt[1], 1.0) - np.where(two, srt[0], 0.0) <= 1e-3))
    obj = np.where(take, -2 - fi, obj)
    x = np.where(take, fx, x)
    n = np.where(take[:, None], fn[fi, np.arange(len(pnt))], n)
  return obj, x, n, ok


def _occluded(mjm, gxpos, gxmat, fxpos, pnt, vec, skip, limit, smooth):
  dist, _ = ray_ref.cast_all(mjm, gxpos, gxmat, pnt, vec, skip)
  fd, _ = cast_flex(mjm, fxpos, pnt, vec, smooth)
  d = np.concatenate([dist, fd], axis=0)
  return ((d >= 0) & (d < limit[None, :])).any(axis=0)


def render(mjm, gxpos, gxmat, fxpos, cam_xpos, cam_xmat, fovy, sensorsize, intrinsic, W, H, light_xpos, light_xdir, light_type, light_active,
           light_castshadow, groups=(0, 1, 2), use_shadows=False, smooth=True, geom_rgba=None, mat_rgba=None, flex_rgba=None):
  """One camera of one world.  Returns seg (H*W,) (-1 background, -2 flex), flexid (H*W,) (-1: no flex), depth, rgb
  (H*W, 3) ints, ok (H*W,) decisive."""
  local = render_ref.pixel_rays(fovy, sensorsize, intrinsic, W, H)
  vec = local @ np.asarray(cam_xmat, dtype=np.float64).reshape(3, 3).T
  pnt = np.broadcast_to(np.asarray(cam_xpos, dtype=np.float64), vec.shape).copy()
  skip = render_ref.drawn_skip(mjm, groups)
  obj, x, n, ok = _first(mjm, gxpos, gxmat, fxpos, pnt, vec, skip, smooth)
  for v2 in render_ref._perturbed(vec):
    o2, x2, n2, _ = _first(mjm, gxpos, gxmat, fxpos, pnt, v2, skip, smooth)
    ok &= (o2 == obj) & (np.abs(x2 - x) <= 1e-2 * np.maximum(1.0, x)) & (np.abs(n2 - n).max(axis=1) <= 1e-2)
  hit = obj != -1
  isflex = obj <= -2
  depth = np.where(hit, x * -local[:, 2], 0.0)
  hitp = pnt + vec * np.where(hit, x, 0.0)[:, None]

  # shading, as render_ref.shade with the flex colour and flexes among the occluders
  rgba = np.asarray(mjm.geom_rgba if geom_rgba is None else geom_rgba, dtype=np.float64).reshape(-1, 4)
  mrgba = np.asarray(mjm.mat_rgba if mat_rgba is None else mat_rgba, dtype=np.float64).reshape(-1, 4)
  frgba = np.asarray(mjm.flex_rgba if flex_rgba is None else flex_rgba, dtype=np.float64).reshape(-1, 4)
  gi = np.where(obj >= 0, obj, 0)
  matid = np.asarray(mjm.geom_matid)[gi] if int(mjm.ngeom) else np.full(len(obj), -1)
  base = np.where((matid >= 0)[:, None], mrgba[np.maximum(matid, 0), :3] if len(mrgba) else 0.0, rgba[gi, :3] if len(rgba) else 0.0)
  base = np.where(isflex[:, None], frgba[np.where(isflex, -2 - obj, 0), :3], base)
  ln = np.linalg.norm(n, axis=1, keepdims=True)
  nu = np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), np.array([0.0, 0.0, 1.0]))
  h = 0.5 * (nu[:, 2:3] + 1.0)
  res = 0.5 * base * (render_ref.AMB_HI * h + render_ref.AMB_LO * (1.0 - h))
  light_xpos, light_xdir = np.asarray(light_xpos, dtype=np.float64).reshape(-1, 3), np.asarray(light_xdir, dtype=np.float64).reshape(-1, 3)
  for l in range(len(light_xpos)):
    if not light_active[l]:
      continue
    if light_type[l] == render_ref.DIRECTIONAL:
      L = np.broadcast_to(-light_xdir[l] / np.linalg.norm(light_xdir[l]), hitp.shape).copy()
      r = np.full(len(obj), np.inf)
      att = np.ones(len(obj))
    else:
      L = light_xpos[l] - hitp
      r = np.linalg.norm(L, axis=1)
      L = L / np.where(r > 0, r, 1.0)[:, None]
      att = 1.0 / (1.0 + 0.02 * r * r)
      if light_type[l] == render_ref.SPOT:
        sd = light_xdir[l] / np.linalg.norm(light_xdir[l])
        att = att * np.clip((-(L @ sd) - 0.85) / 0.10, 0.0, 1.0)
    ndotl = np.maximum(0.0, (n * L).sum(-1))
    visible = np.ones(len(obj))
    if use_shadows and light_castshadow[l]:
      idx = np.nonzero(hit & (ndotl > 0))[0]
      if len(idx):
        origin = hitp[idx] + 1e-4 * n[idx]
        limit = np.full(len(idx), 1e8) if light_type[l] == render_ref.DIRECTIONAL else r[idx] - 1e-3
        occ = _occluded(mjm, gxpos, gxmat, fxpos, origin, L[idx], skip, limit, smooth)
        for v2 in render_ref._perturbed(L[idx]):
          ok[idx] &= _occluded(mjm, gxpos, gxmat, fxpos, origin, v2, skip, limit, smooth) == occ
        visible[idx[occ]] = 0.3
    res = res + base * (ndotl * att * visible)[:, None]
  col = np.where(hit[:, None], np.clip(res, 0.0, 1.0), 0.0)
  rgb = np.where(hit[:, None], np.floor(col * 255.0).astype(np.int64), np.array(render_ref.BACKGROUND))
  seg = np.where(isflex, -2, obj)
  return seg, np.where(isflex, -2 - obj, -1), depth, rgb, ok
