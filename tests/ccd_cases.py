"""The convex collision code (csrc/mjw_ccd.h) at its capacity and degeneracy edges: the cases, their proofs and the
acceptance rule shared by tests/test_ccd_cases.py (CPU) and tests/test_gpu_ccd_edges.py (device).

A case is one 48-float record of the device's known-answer entry (csrc/mjw_kat.hip, which = 0: one wavefront runs
ccd_raw and, when asked, box multi-contact over its own LDS workspace) plus a predicate over the fp64 oracle's trace
(oracle/oracle_ccd.h ccd_trace) that proves the edge the case is named after is reached.  Everything is generated here
from seeds; the meshes are point sets made in code (Fibonacci spheres, n-gon prisms, a 5 x 5 x 5 lattice cube, and
copies with duplicated and permuted vertices).

Families (FAMILIES[name]() -> Family):
  types      the 21 unordered pairs of sphere, capsule, ellipsoid, cylinder, box and mesh in four bands: separated
             beyond the margin, separated inside margin 0.01, 1 mm deep, and geom2's centre inside geom1.  The
             centre distance of the first three is found by bisection on the fp64 oracle (64 iterations), so the
             bands stay 0.5 mm and more away from touching and fp32 and fp64 decide alike.
  aligned    identity and exactly quarter-turned rotations, offsets along one, two and three axes, concentric geoms,
             capsule / cylinder axes parallel, crossing and collinear, boxes face-face, edge-edge, vertex-face and
             edge-face, box yaw 0 / 45 / 90 degrees: GJK leaves simplices of every dimension, so polytope2 / 3 / 4,
             both fall-throughs to polytope3 and the dim < 2 return are all taken, and box supports see ccd_sign(0).
  capacity   EPA iteration counts 2 .. 64 on pairs that use them all (nvert = 5 + it, the last vertex slot), that
             leave the face array one short of full and exactly full, and that overflow it (EPA then reports no
             contact); the longest horizon the search reached (12 of 24 edges: no input overflows it); records of
             different iteration counts in one launch (each case runs in the layout of its own count inside LDS
             sized for the largest).  The search runs the aligned poses and fine prisms at every count.
  meshverts  meshes of 4, 63, 64, 65, 127, 128, 129 and 200 vertices against mesh, box and sphere, the supporting
             vertex in the first and the last stride, at index 0 and at index nvert - 1, and exact ties between
             lanes (lattice cube, duplicated vertices): the lowest index has to win.
  scale      geoms of 1 mm and of 10 m (at 10 m spheres, capsules and boxes: fp32 GJK on an ellipsoid or a cylinder of
             that size is off by centimetres), 100:1 plates, needles and discs met face-on by the standard geoms,
             ccd_tolerance 1e-6 / 1e-4 / 1e-2, margin zero and non-zero (a margin turns `discrete` and multi-contact
             off).  Seed 7 of 1 .. 11 tried: the others leave one of the fp32 oracle builds above half a cap.
  multibox   box-box face overlaps whose clipped polygon has 3 .. 8 vertices (the trace's polygon count), and
             overlaps narrowing towards a strip; count, distance and normal are compared, and on the device every kept
             point has to lie inside both faces (box_points_outside; DESIGN section 5 explains the pruning tie that
             forbids a point-by-point comparison).

Acceptance rule (`classify`), per case, for a result `got` = (ncon, dist, x1, x2):
  pass       against the fp64 oracle: equal count, |dist| within 2e-5, witness points within 2e-4 (2e-3 when an
             ellipsoid or a cylinder takes part) -- the bars of tests/test_collision_types.py.  With multi-contact
             requested the normal (x1 - x2, normalised) within 2e-3 takes the witness points' place.  The witness bar
             is otherwise dropped only where the fp64 oracle proves the witness undefined (`ambiguity`: it jumps when
             geom2 is nudged by a micrometre or turned by 2e-5 rad -- a face on a face, an edge along a face, several
             equally deep directions): there the normal is compared, or, where the normal jumps as well, that the
             witness points lie the reported distance apart.  About 43 % of `aligned`, 64 % of `meshverts`, 97 % of
             `types` and 99 % of `scale` keep the full witness bar.
  tie        misses those bars, an fp32 oracle build (liborc32 or liborc32f) misses them on the same case too, and
             `got` equals one of the two at the bar of tests/test_gpu_golden.py (1e-6 absolute or 1e-4 relative
             distance, same count).
  unmatched  anything else; it then has to satisfy a path-independent property (`property_ok`): with D the fp64
             oracle's depth at 64 iterations, the reported depth is at most D + 2e-5, and geom2 moved by the
             reported depth along the reported normal is at fp64 GJK distance within 2e-5 + tolerance of zero when
             EPA converged (in the fp64 oracle and both fp32 builds, at the case's own iteration count), or at most
             that when it stopped early.  A result of no contact counts as an EPA that stopped early with depth 0: the
             reference's EPA gives up that way (face array full, horizon overflow, degenerate face), and the 1 % cap
             on the unmatched is what bounds it.
Caps (`CAPS`): ties <= 2 % of a family at default iterations, <= 8 % in `capacity` and in any family with an iteration
count below 35; unmatched <= 1 %.  The fp32 oracle builds themselves, put through the rule in `got`'s place (the tie
clause then asks the other build), have to stay inside half of each cap (tests/test_ccd_cases.py).
"""
import functools

import numpy as np

SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX, MESH = 2, 3, 4, 5, 6, 7
NAMES = {2: "sphere", 3: "capsule", 4: "ellipsoid", 5: "cylinder", 6: "box", 7: "mesh"}
SIZES = {2: (0.12, 0, 0), 3: (0.08, 0.12, 0), 4: (0.14, 0.09, 0.06), 5: (0.1, 0.08, 0), 6: (0.1, 0.07, 0.05), 7: (0, 0, 0)}
REC, OUT = 48, 8
DEFAULT_IT = 35
CAPS = {"tie_default": 0.02, "tie_capped": 0.08, "unmatched": 0.01}
ROUTES = (2, 3, 4, 23, 43)
TRACE = ("gjk_iter", "gjk_dim", "route", "status", "epa_iter", "epa_exit", "nvert", "nface", "horizon", "multi", "poly_np",
         "cap_vert", "cap_face", "inflated", "attach_fail", "ngjk")
T = {k: i for i, k in enumerate(TRACE)}
EXIT = {"converged": 1, "repeated vertex": 2, "iterations exhausted": 3, "no valid face": 4, "face array full": 5,
        "horizon overflow": 6, "degenerate face": 7, "lower2 > upper2": 8}


# ---- meshes -----------------------------------------------------------------------------------------------------
def fib_sphere(n, r=0.1):
  """n points on a sphere of radius r (golden-angle spiral); generic: no two supports tie."""
  i = np.arange(n) + 0.5
  z = 1 - 2 * i / n
  ph = i * np.pi * (3 - np.sqrt(5))
  s = np.sqrt(1 - z * z)
  return r * np.stack([s * np.cos(ph), s * np.sin(ph), z], 1)


def prism(n, r=0.1, h=0.05):
  """A regular n-gon prism about z: 2 n vertices, bottom ring then top ring."""
  a = 2 * np.pi * np.arange(n) / n
  ring = np.stack([r * np.cos(a), r * np.sin(a)], 1)
  return np.concatenate([np.c_[ring, np.full(n, -h)], np.c_[ring, np.full(n, h)]])


def lattice_cube(k=5, h=0.08):
  """k^3 lattice points of a cube of half side h: whole faces and edges tie under axis directions."""
  g = np.linspace(-h, h, k)
  return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def duplicated(v, seed):
  """Every vertex twice, the copies permuted: each support has a tie at two indices."""
  rng = np.random.default_rng(seed)
  vv = np.concatenate([v, v])
  return vv[rng.permutation(len(vv))]


def rolled(v, k):
  return np.roll(v, k, axis=0)


class MeshPool:
  """The launch's mesh vertices, concatenated; add() returns (vertadr, nvert)."""

  def __init__(self):
    self.v, self.n, self.key = [], 0, {}

  def add(self, name, verts):
    if name not in self.key:
      v = np.asarray(verts, np.float32)
      self.key[name] = (self.n, len(v))
      self.v.append(v)
      self.n += len(v)
    return self.key[name]

  def verts(self):
    return np.concatenate(self.v) if self.v else np.zeros((1, 3), np.float32)


# ---- records ----------------------------------------------------------------------------------------------------
def rot(axis, deg):
  a = np.asarray(axis, float)
  a = a / np.linalg.norm(a)
  t = np.deg2rad(deg)
  K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
  R = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K
  return np.where(np.abs(R) < 1e-15, 0.0, R) if deg % 90 else np.round(R)  # exact quarter turns


def rand_rot(rng):
  q = rng.normal(size=4)
  w, x, y, z = q / np.linalg.norm(q)
  return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rand_dir(rng):
  u = rng.normal(size=3)
  return u / np.linalg.norm(u)


I3 = np.eye(3)


def record(t1, t2, p1, R1, s1, p2, R2, s2, margin=0.0, tol=1e-6, it=DEFAULT_IT, multi=0, m1=(0, 0), m2=(0, 0)):
  r = np.zeros(REC, np.float32)
  r[0], r[1] = t1, t2
  r[2:5], r[5:14], r[14:17] = p1, np.asarray(R1).reshape(9), s1
  r[17:20], r[20:29], r[29:32] = p2, np.asarray(R2).reshape(9), s2
  r[32], r[33], r[34], r[35] = margin, tol, it, multi
  r[36], r[37], r[38], r[39] = m1[0], m1[1], m2[0], m2[1]
  return r


class Family:
  def __init__(self, name):
    self.name, self.pool = name, MeshPool()
    self.recs, self.ids, self.preds = [], [], []

  def add(self, cid, rec, pred=None):
    """pred: (label, f(trace row, fp64 out row) -> bool) or None."""
    self.recs.append(rec)
    self.ids.append(cid)
    self.preds.append(pred)

  def arrays(self):
    return np.stack(self.recs), self.pool.verts()

  @property
  def capped(self):
    return self.name == "capacity" or bool((np.stack(self.recs)[:, 34] < DEFAULT_IT).any())

  def aux(self):
    """The aux buffer of mjw_kat(0, ...): the batch's largest iteration count, then the mesh vertices."""
    recs, mv = self.arrays()
    return np.concatenate([[recs[:, 34].max()], mv.reshape(-1)]).astype(np.float32)


def _oracle(recs, mv, bits=64, trace=False):
  from oracle import orc

  return orc.kat_ccd_batch(recs, mv, real_bits=bits, trace=trace)


def place(recs, mv, u, target, lo, hi):
  """Move geom2 of every record to t u with the fp64 oracle's signed distance (margin 0, 64 iterations) equal to
  `target`, by bisection over t in [lo, hi] (arrays); a pair EPA gives up on counts as penetrating."""
  recs = recs.copy()
  probe = recs.copy()
  probe[:, 32], probe[:, 33], probe[:, 34], probe[:, 35] = 0, 1e-6, 64, 0
  lo, hi = np.array(lo, float), np.array(hi, float)
  for _ in range(30):
    t = 0.5 * (lo + hi)
    probe[:, 17:20] = probe[:, 2:5] + t[:, None] * u
    o = _oracle(probe, mv)
    d = np.where(o[:, 0] < 1, -1e9, o[:, 1])
    above = d > target
    hi = np.where(above, t, hi)
    lo = np.where(above, lo, t)
  recs[:, 17:20] = recs[:, 2:5] + (0.5 * (lo + hi))[:, None] * u
  return recs


def _geom(fam, t, mesh=None):
  """(size, (vertadr, nvert), bounding radius, inner radius) of the family's standard geom of type t."""
  if t == MESH:
    name, v = mesh if mesh is not None else ("fib65", fib_sphere(65))
    return np.zeros(3), fam.pool.add(name, v), float(np.linalg.norm(v, axis=1).max()), 0.02
  s = np.array(SIZES[t], float)
  rad = {SPHERE: s[0], CAPSULE: s[0] + s[1], ELLIPSOID: s.max(), CYLINDER: np.hypot(s[0], s[1]), BOX: np.linalg.norm(s)}[t]
  inner = {SPHERE: s[0], CAPSULE: s[0], ELLIPSOID: s.min(), CYLINDER: min(s[0], s[1]), BOX: s.min()}[t]
  return s, (0, 0), float(rad), float(inner)


# ---- predicates ---------------------------------------------------------------------------------------------------
def p_band(lo, hi):
  return (f"fp64 distance in ({lo}, {hi})", lambda tr, o: o[0] == 1 and lo < o[1] < hi)


def p_trace(label, f):
  return (label, lambda tr, o: bool(f({k: int(tr[i]) for k, i in T.items()}, o)))


# ---- families ---------------------------------------------------------------------------------------------------
BANDS = {"beyond": (0.012, 0.0), "inmargin": (0.004, 0.01), "shallow": (-0.001, 0.0)}


def fam_types(nseed=8):
  fam = Family("types")
  kinds = (SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX, MESH)
  pairs = [(a, b) for i, a in enumerate(kinds) for b in kinds[i:]]
  for band, (target, margin) in BANDS.items():
    recs, us, los, his, ids = [], [], [], [], []
    for t1, t2 in pairs:
      rng = np.random.default_rng(1000 * t1 + 10 * t2 + len(band))
      s1, m1, R1b, in1 = _geom(fam, t1)
      s2, m2, R2b, in2 = _geom(fam, t2)
      for k in range(nseed):
        recs.append(record(t1, t2, np.zeros(3), rand_rot(rng), s1, np.zeros(3), rand_rot(rng), s2, margin=margin, m1=m1, m2=m2))
        us.append(rand_dir(rng))
        los.append(0.5 * max(in1, in2))
        his.append(R1b + R2b + 0.2)
        ids.append(f"{NAMES[t1]}-{NAMES[t2]}-{band}-{k}")
    placed = place(np.stack(recs), fam.pool.verts(), np.stack(us), target, los, his)
    # the oracle's distance carries the margin (both geoms inflated by half of it)
    win = {"beyond": (0.0115, 0.0125), "inmargin": (-0.0065, -0.0055), "shallow": (-0.0015, -0.0005)}[band]
    for r, cid in zip(placed, ids):
      fam.add(cid, r, p_band(*win))
  for t1, t2 in pairs:  # deep: geom2's centre inside geom1
    rng = np.random.default_rng(77 + 10 * t1 + t2)
    s1, m1, _, in1 = _geom(fam, t1)
    s2, m2, _, _ = _geom(fam, t2)
    for k in range(nseed):
      p2 = 0.4 * in1 * rand_dir(rng)
      fam.add(f"{NAMES[t1]}-{NAMES[t2]}-deep-{k}", record(t1, t2, np.zeros(3), rand_rot(rng), s1, p2, rand_rot(rng), s2, m1=m1, m2=m2),
              ("geom2's centre inside geom1: fp64 depth above 5 mm or EPA gives up", lambda tr, o: o[0] == 0 or o[1] < -0.005))
  return fam


AXES = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1), (-1, 0, 0), (0, 0, -1), (1, -1, 0), (-1, 1, -1)]


# (type1, type2, geom2's rotation axis and degrees, index into AXES, fraction of the summed inner radii): found by
# a sweep of identity / 45 / 90 degree rotations and offsets in steps of 0.05 on the fp64 oracle's trace
ROUTE43 = ((ELLIPSOID, MESH, (0, 0, 1), 0, 6, 0.3), (ELLIPSOID, MESH, (0, 0, 1), 90, 10, 0.3), (CAPSULE, BOX, (1, 0, 0), 45, 3, 0.15),
           (ELLIPSOID, CYLINDER, (1, 0, 0), 45, 0, 0.55), (ELLIPSOID, BOX, (1, 1, 0), 90, 5, 0.45))


def fam_aligned():
  fam = Family("aligned")
  kinds = (SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX, MESH)
  cube = ("lattice5", lattice_cube())
  quarter = [I3, rot((0, 0, 1), 90), rot((1, 0, 0), 90), rot((0, 1, 0), 90)]
  # identity / quarter-turn rotations, geom2 at fractions of the summed extent along 1, 2 and 3 axes, and concentric
  for i, t1 in enumerate(kinds):
    for t2 in kinds[i:]:
      s1, m1, R1b, in1 = _geom(fam, t1, cube)
      s2, m2, R2b, in2 = _geom(fam, t2, cube)
      for qi, R2 in enumerate(quarter):
        if (t2 == SPHERE and qi > 0) or (t2 in (CAPSULE, CYLINDER) and qi == 1):
          continue  # the same pose again
        for ai, ax in enumerate(AXES):
          u = np.array(ax, float)
          for fi, f in enumerate((0.0, 0.45, 0.6, 0.9, 1.3)):
            if f == 0.0 and ai > 0:
              continue
            p2 = f * (in1 + in2) * u / np.abs(u).max()
            fam.add(f"{NAMES[t1]}-{NAMES[t2]}-q{qi}-a{ai}-f{fi}", record(t1, t2, np.zeros(3), I3, s1, p2, R2, s2, m1=m1, m2=m2))
  # poses whose GJK ends on a tetrahedron with the origin on one of its faces: polytope4 hands over to polytope3
  for t1, t2, ax, deg, ai, f in ROUTE43:
    s1, m1, _, in1 = _geom(fam, t1, cube)
    s2, m2, _, in2 = _geom(fam, t2, cube)
    p2 = f * (in1 + in2) * np.array(AXES[ai], float) / np.abs(AXES[ai]).max()
    fam.add(f"{NAMES[t1]}-{NAMES[t2]}-route43-{deg}-a{ai}", record(t1, t2, np.zeros(3), I3, s1, p2, rot(ax, deg), s2, m1=m1, m2=m2),
            p_trace("polytope4 falls through to polytope3", lambda t, o: t["route"] == 43))
  # capsule / cylinder axes parallel, crossing and collinear, touching depths 1 mm .. deep
  for t1 in (CAPSULE, CYLINDER):
    for t2 in (CAPSULE, CYLINDER):
      s1, s2 = np.array(SIZES[t1]), np.array(SIZES[t2])
      for name, R2, p2s in (("parallel", I3, [(s1[0] + s2[0] - d, 0, 0) for d in (0.001, 0.01, 0.05)]),
                            ("crossing", rot((1, 0, 0), 90), [(0, 0, 0), (s1[0] + s2[0] - 0.005, 0, 0), (0.01, 0, 0)]),
                            ("collinear", I3, [(0, 0, s1[1] + s2[1] + (s1[0] + s2[0] if t1 == t2 == CAPSULE else 0) - d) for d in (0.001, 0.02)])):
        for k, p2 in enumerate(p2s):
          fam.add(f"{NAMES[t1]}-{NAMES[t2]}-{name}-{k}", record(t1, t2, np.zeros(3), I3, s1, p2, R2, s2))
  # boxes: face-face, edge-edge at 90 degrees, vertex-face, edge-face; yaw exactly 0, 45, 90
  a, b = np.array([0.1, 0.07, 0.05]), np.array([0.06, 0.06, 0.06])
  diag = np.sqrt(3) * 0.06
  e45x, e45y = rot((1, 0, 0), 45), rot((0, 1, 0), 45)
  vtx = rot((1, -1, 0), np.rad2deg(np.arccos(1 / np.sqrt(3))))  # a cube diagonal onto z
  for d in (0.001, 0.004, 0.02):
    for yaw in (0, 45, 90):
      for off in ((0, 0), (0.03, 0), (0.03, 0.02)):
        fam.add(f"box-box-face-yaw{yaw}-d{d}-o{off}", record(BOX, BOX, np.zeros(3), I3, a, (off[0], off[1], a[2] + b[2] - d), rot((0, 0, 1), yaw), b))
    fam.add(f"box-box-edge-edge-d{d}", record(BOX, BOX, np.zeros(3), e45x, b, (0, 0, 2 * np.sqrt(2) * 0.06 - d), e45y, b))
    fam.add(f"box-box-vertex-face-d{d}", record(BOX, BOX, np.zeros(3), I3, a, (0, 0, a[2] + diag - d), vtx, b))
    fam.add(f"box-box-edge-face-d{d}", record(BOX, BOX, np.zeros(3), I3, a, (0, 0, a[2] + np.sqrt(2) * 0.06 - d), e45x, b))
    fam.add(f"box-box-face-sep-d{d}", record(BOX, BOX, np.zeros(3), I3, a, (0, 0, a[2] + b[2] + d), I3, b))
  return fam


# capacity: the search space is the aligned family's poses plus fine prisms and discs seen from their axis, each run
# at every iteration count of CAP_ITS on the fp64 oracle; per count and edge the first CAP_PER poses whose trace shows the
# edge are kept (the selection is this code: nothing but the parameters is committed).  profiles/ccd_edges.json has the
# size of the search and what it did not reach.
CAP_ITS = (2, 3, 4, 8, 16, 35, 64)
CAP_PER = 30
HORIZON_MIN = 11  # the longest horizon the search reaches is 11 or 12 of the 24 edges
CAP_EDGES = {
  "exhausted": ("EPA uses every iteration and the last vertex slot", lambda t, o: t["epa_exit"] == 3 and t["nvert"] == t["cap_vert"]),
  "full-1": ("nface == cap_face - 1", lambda t, o: t["cap_face"] > 0 and t["nface"] == t["cap_face"] - 1 and t["epa_exit"] != 5),
  "full": ("nface == cap_face, no overflow", lambda t, o: t["cap_face"] > 0 and t["nface"] == t["cap_face"] and t["epa_exit"] != 5),
  "overflow": ("face array full: EPA reports no contact", lambda t, o: t["epa_exit"] == 5 and o[0] == 0),
  "horizon": (f"horizon of {HORIZON_MIN} edges or more", lambda t, o: t["horizon"] >= HORIZON_MIN),
  "horizon-overflow": ("horizon overflow: EPA reports no contact", lambda t, o: t["epa_exit"] == 6 and o[0] == 0),
}


def capacity_candidates():
  """(records, ids, pool) of the search space, at the default iteration count."""
  al = family("aligned")
  recs, ids = list(al.recs), list(al.ids)
  fam = Family("capacity-search")
  fam.pool = al.pool
  for n, h in ((48, 0.05), (96, 0.05), (96, 0.002)):
    m = fam.pool.add(f"prism{n}-{h}", prism(n, 0.1, h))
    for t2, s2 in ((SPHERE, (0.05, 0, 0)), (ELLIPSOID, SIZES[ELLIPSOID]), (BOX, SIZES[BOX]), (CYLINDER, SIZES[CYLINDER])):
      for off in ((0, 0), (0.03, 0), (0.05, 0.02), (0.09, 0)):
        for dz in (0.0, 0.3, 0.8):
          for tilt in (0, 2):
            z = dz * (h + max(s2))
            recs.append(record(t2, MESH, (off[0], off[1], z), rot((1, 0, 0), tilt), s2, np.zeros(3), I3, np.zeros(3), m2=m))
            ids.append(f"{NAMES[t2]}-prism{n}-{h}-o{off}-z{dz}-t{tilt}")
  return np.stack(recs), ids, fam.pool


def capacity_search():
  """Per iteration count: (records at that count, fp64 out, trace, {edge: indices reaching it})."""
  recs0, ids, pool = capacity_candidates()
  mv = pool.verts()
  out = {}
  for it in CAP_ITS:
    recs = recs0.copy()
    recs[:, 34] = it
    o, tr = _oracle(recs, mv, 64, trace=True)
    # keep the well-conditioned poses: the fp64 answer holds when geom2 is nudged by one and by three micrometres
    steady = np.ones(len(recs), bool)
    for sgn, d in ((1, (0.6, -0.64, 0.48)), (-1, (0.6, -0.64, 0.48)), (3, (0.36, 0.8, -0.48)), (-3, (0.36, 0.8, -0.48))):
      nudged = recs.copy()
      nudged[:, 17:20] += np.float32(sgn * 1e-6) * np.array(d, np.float32)
      on = _oracle(nudged, mv, 64)
      steady &= (on[:, 0] == o[:, 0]) & ((o[:, 0] < 1) | (np.abs(on[:, 1] - o[:, 1]) <= 1e-5))
    hit = {}
    for edge, (_, f) in CAP_EDGES.items():
      hit[edge] = [i for i in range(len(recs)) if steady[i] and f({k: int(tr[i, j]) for k, j in T.items()}, o[i])]
    out[it] = (recs, o, tr, hit)
  return out, ids, pool


def fam_capacity():
  fam = Family("capacity")
  found, ids, pool = capacity_search()
  fam.pool = pool
  for it in CAP_ITS:  # records of every count interleaved in one launch
    recs, _, _, hit = found[it]
    for edge, idx in hit.items():
      for i in idx[:CAP_PER]:
        fam.add(f"it{it}-{edge}-{ids[i]}", recs[i], p_trace(CAP_EDGES[edge][0], CAP_EDGES[edge][1]))
  order = np.argsort([hash_id(c) for c in fam.ids], kind="stable")  # mix the counts through the launch
  fam.recs, fam.ids, fam.preds = [fam.recs[i] for i in order], [fam.ids[i] for i in order], [fam.preds[i] for i in order]
  return fam


def hash_id(cid):
  import zlib

  return zlib.crc32(cid.encode())


def fam_meshverts():
  fam = Family("meshverts")
  rng = np.random.default_rng(42)
  box = np.array(SIZES[BOX])
  for n in (4, 63, 64, 65, 127, 128, 129, 200):
    base = fib_sphere(n)
    # a spike moved to a chosen index makes that vertex the support towards geom2: first / last stride, index 0 / n - 1
    for where, idx in (("first", 0), ("last", n - 1), ("stride-last", (n - 1) // 64 * 64 if n > 64 else n // 2), ("lane63", min(63, n - 1))):
      v = base.copy()
      u = v[idx] / np.linalg.norm(v[idx])
      v[idx] = 0.13 * u
      m = fam.pool.add(f"fib{n}-{where}", v)
      for t2, s2, reach in ((SPHERE, (0.05, 0, 0), 0.05), (BOX, box, None), (MESH, None, None)):
        for depth in (0.002, -0.01):
          R2 = rand_rot(rng)
          if t2 == MESH:
            m2 = fam.pool.add(f"fib{n}-rolled", rolled(base, 5))
            r = record(MESH, MESH, np.zeros(3), I3, np.zeros(3), (0.13 + 0.1 - depth) * u, R2, np.zeros(3), m1=m, m2=m2)
          else:
            ext = reach if reach else float(np.abs(R2.T @ u) @ box)
            r = record(MESH, t2, np.zeros(3), I3, np.zeros(3), (0.13 + ext - depth) * u, R2, s2, m1=m)
          pred = (f"fp64 witness on the mesh is vertex {idx}", functools.partial(lambda tr, o, p: np.abs(o[2:5] - p).max() < 2e-3, p=v[idx].astype(np.float32)))
          fam.add(f"n{n}-{where}-{NAMES[t2]}-{'pen' if depth > 0 else 'sep'}", r, pred if t2 == SPHERE else None)
  # exact ties across lanes: lattice cube faces under axis directions, duplicated and permuted vertex sets
  cube = lattice_cube()
  sets = [("lattice5", cube), ("lattice5-dup", duplicated(cube, 1)), ("prism12-dup", duplicated(prism(12), 2)), ("fib65-dup", duplicated(fib_sphere(65), 3)),
          ("lattice5-rolled", rolled(cube, 37)), ("prism48", prism(48)), ("prism48-dup", duplicated(prism(48), 4))]
  for name, v in sets:
    m = fam.pool.add(name, v)
    ext = np.abs(v).max(0)
    for ai, ax in enumerate(AXES[:9]):
      u = np.array(ax, float)
      reach = float((ext * np.abs(u)).sum() / np.linalg.norm(u))
      un = u / np.linalg.norm(u)
      for t2, s2 in ((SPHERE, (0.05, 0, 0)), (BOX, (0.05, 0.05, 0.05)), (MESH, None)):
        for depth in (0.003, 0.02):
          if t2 == MESH:
            m2 = fam.pool.add("lattice5-dup", duplicated(cube, 1))
            r2 = float((0.08 * np.abs(u)).sum() / np.linalg.norm(u))
            r = record(MESH, MESH, np.zeros(3), I3, np.zeros(3), (reach + r2 - depth) * un, I3, np.zeros(3), m1=m, m2=m2)
          else:
            r2 = 0.05 if t2 == SPHERE else float((0.05 * np.abs(u)).sum() / np.linalg.norm(u))
            r = record(MESH, t2, np.zeros(3), I3, np.zeros(3), (reach + r2 - depth) * un, I3, s2, m1=m)
          fam.add(f"{name}-a{ai}-{NAMES[t2]}-d{depth}", r)
  return fam


def fam_scale(seed=7):
  fam = Family("scale")
  rng = np.random.default_rng(seed)
  recs, us, los, his, ids, targets = [], [], [], [], [], []

  def push(cid, r, u, lo, hi, target):
    recs.append(r), us.append(u), los.append(lo), his.append(hi), ids.append(cid), targets.append(target)

  kinds = (SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX)
  # the standard sizes are ~ 0.1: scaled to 1 mm and to 10 m, a tenth of the size deep
  for scale, sname in ((0.01, "1mm"), (100.0, "10m")):
    # at 10 m only the geoms with exact supports: GJK on an ellipsoid or a cylinder of that size is off by centimetres
    # in fp32 (both fp32 oracle builds; profiles/ccd_edges.json), far outside any bar stated in metres
    ks = kinds if scale < 1 else (SPHERE, CAPSULE, BOX)
    for i, t1 in enumerate(ks):
      for t2 in ks[i:]:
        s1, s2 = np.array(SIZES[t1]) * scale, np.array(SIZES[t2]) * scale
        for tol in (1e-6, 1e-4, 1e-2):
          for margin in (0.0, 0.01):
            for k in range(2):
              push(f"{NAMES[t1]}-{NAMES[t2]}-{sname}-tol{tol}-m{margin}-{k}",
                   record(t1, t2, np.zeros(3), rand_rot(rng), s1, np.zeros(3), rand_rot(rng), s2, margin=margin, tol=tol),
                   rand_dir(rng), 0.03 * scale, 0.6 * scale, -0.01 * scale)
  # 100:1 plates, needles and discs against the standard geoms, 2 mm deep
  thin = {"plate": (BOX, (1.0, 1.0, 0.01)), "needle": (CAPSULE, (0.005, 0.5, 0)), "disc": (CYLINDER, (0.5, 0.005, 0)),
          "needle-box": (BOX, (0.005, 0.005, 0.5))}
  for n1, (t1, s1) in thin.items():
    for t2 in (SPHERE, CAPSULE, BOX):
      for k in range(6):
        for margin in (0.0, 0.01):
          # the partner comes down on the plate's or the disc's face, or onto the needle's side, 15 degrees off square
          Rt, Rp = rand_rot(rng), rand_rot(rng)
          u = Rt @ rot(rand_dir(rng), 15) @ np.array([0, 0, 1.0] if n1 in ("plate", "disc") else [1.0, 0, 0])
          a, b = ((t1, s1, Rt), (t2, SIZES[t2], Rp)) if t1 <= t2 else ((t2, SIZES[t2], Rp), (t1, s1, Rt))
          push(f"{n1}-{NAMES[t2]}-{k}-m{margin}", record(a[0], b[0], np.zeros(3), a[2], a[1], np.zeros(3), b[2], b[1], margin=margin),
               u, 0.0005, 1.8, -0.002)
  recs, us, tg = np.stack(recs), np.stack(us), np.array(targets)
  placed = {}
  for t in np.unique(tg):
    sel = np.nonzero(tg == t)[0]
    placed.update(zip(sel, place(recs[sel], fam.pool.verts(), us[sel], t, np.array(los)[sel], np.array(his)[sel])))
  for i in range(len(recs)):
    fam.add(ids[i], placed[i], ("fp64 oracle answers; 2e-5 deep or more it is a contact", lambda tr, o, r=placed[i]: o[0] == 1 and (o[1] < 0 or r[33] > 1e-5 or r[14] < 0.005)))
  return fam


_CONVEX = {(2, 4), (2, 7), (3, 4), (3, 5), (3, 7), (4, 4), (4, 5), (4, 6), (4, 7), (5, 5), (5, 6), (5, 7), (6, 6), (6, 7), (7, 7),
           (2, 2), (2, 3), (3, 3), (2, 5), (2, 6), (3, 6)}

# multibox: (offset x, offset y, yaw degrees), lower and upper half sizes, and the clipped polygon's vertex count before
# pruning; the poses come from a seeded search over offsets and whole-degree yaws on the fp64 oracle's trace
_A, _B, _S, _T = (0.1, 0.08, 0.05), (0.06, 0.05, 0.03), (0.06, 0.06, 0.05), (0.06, 0.06, 0.03)
MULTIBOX = (
  ((0.031, 0.103, 36), _A, _B, 3), ((0.11, -0.084, 46), _A, _B, 3), ((0.003, 0.103, 24), _A, _B, 3),
  ((-0.116, 0.075, 3), _A, _B, 4), ((0.099, 0.026, 87), _A, _B, 4), ((0.01, 0.104, 65), _A, _B, 4),
  ((-0.046, -0.003, 64), _A, _B, 5), ((0.017, -0.043, 64), _A, _B, 5), ((-0.065, -0.108, 71), _A, _B, 5),
  ((0.033, -0.055, 27), _A, _B, 6), ((-0.048, -0.019, 48), _A, _B, 6), ((0.035, 0.028, 60), _A, _B, 6),
  ((0.011, -0.018, 27), _S, _T, 7), ((-0.012, -0.006, 78), _S, _T, 7), ((0.005, -0.017, 72), _S, _T, 7),
  ((-0.016, -0.006, 48), _S, _T, 8), ((0.012, 0.009, 60), _S, _T, 8), ((-0.015, -0.001, 64), _S, _T, 8),
)


def fam_multibox():
  fam = Family("multibox")
  for (ox, oy, yaw), a, b, npoly in MULTIBOX:
    for d in (0.001, 0.002, 0.004):
      for tilt in (0.0, 0.05):  # inside FACE_TOL (0.0016 rad ~ 0.09 degrees) the faces still count as parallel
        R2 = rot((0, 0, 1), yaw) @ rot((1, 0, 0), tilt)
        fam.add(f"poly{npoly}-o{ox},{oy}-yaw{yaw}-d{d}-t{tilt}", record(BOX, BOX, np.zeros(3), I3, a, (ox, oy, a[2] + b[2] - d), R2, b, multi=1),
                p_trace(f"multi-contact clips a polygon of {npoly} vertices", functools.partial(lambda t, o, n: t["multi"] == 1 and t["poly_np"] == n, n=npoly)))
  # overlaps narrowing towards a strip: the upper box slides off the edge, 20 mm .. 0.1 mm of overlap left
  a, b = (0.1, 0.08, 0.05), (0.05, 0.05, 0.03)
  for w in (0.02, 0.005, 0.001, 0.0003, 0.0001):
    for yaw in (0, 90):
      fam.add(f"strip-{w}-yaw{yaw}", record(BOX, BOX, np.zeros(3), I3, a, (a[0] + b[0] - w, 0.01, a[2] + b[2] - 0.002), rot((0, 0, 1), yaw), b, multi=1),
              p_trace("multi-contact ran on the strip", lambda t, o: t["multi"] == 1 and t["poly_np"] >= 2))
  return fam


FAMILIES = {"types": fam_types, "aligned": fam_aligned, "capacity": fam_capacity, "meshverts": fam_meshverts, "scale": fam_scale,
            "multibox": fam_multibox}


@functools.lru_cache(maxsize=None)
def family(name):
  return FAMILIES[name]()


@functools.lru_cache(maxsize=None)
def references(name):
  """The oracle answers of a family, computed once: fp64 (with trace), liborc32, liborc32f, and fp64 at 64 iterations."""
  recs, mv = family(name).arrays()
  o64, tr = _oracle(recs, mv, 64, trace=True)
  r64 = recs.copy()
  r64[:, 34] = 64
  o32, tr32 = _oracle(recs, mv, 32, trace=True)
  o32f, tr32f = _oracle(recs, mv, "32f", trace=True)
  return dict(o64=o64, trace=tr, o32=o32, o32f=o32f, trace32=tr32, trace32f=tr32f, deep=_oracle(r64, mv, 64),
              amb=ambiguity(recs, mv, o64))


def _small_rot(axis, angle):
  K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], float)
  return np.eye(3) + angle * K


def ambiguity(recs, mv, o64):
  """Per case, proven on the fp64 oracle alone: 0 the witness points are well defined, 1 they are not but the normal is,
  2 neither is.  Geom2 is nudged by 1 um along two directions and turned by 2e-5 rad about three axes, each both ways; a
  well-defined witness follows by micrometres.  Where a witness point jumps by more than 1e-4 (+ 1e-4 of the geoms' size)
  the closest points form a segment or a face, or several directions are equally deep: any of them is a right answer and
  the witness bar cannot be asked.  Where the normal turns by more than 1e-3 as well, only the distance and the witness
  gap are left.  A probe that changes the count or moves the distance by more than 1e-5 also counts as 2."""
  amb = np.zeros(len(recs), int)
  size = np.maximum(np.abs(recs[:, 14:17]).max(1), np.abs(recs[:, 29:32]).max(1)).astype(float)
  size = np.maximum(size, np.abs(recs[:, 17:20] - recs[:, 2:5]).max(1))
  thr = 1e-4 + 1e-4 * size
  n0 = _unit(o64[:, 2:5] - o64[:, 5:8])
  probes = [("t", np.array(d) * sg) for d in ((0.6, -0.64, 0.48), (0.36, 0.8, -0.48)) for sg in (1, -1)]
  probes += [("r", np.array(a) * sg) for a in ((1.0, 0, 0), (0, 0.6, 0.8), (0.8, 0.6, 0)) for sg in (1, -1)]
  for kind, v in probes:
    r = recs.copy()
    if kind == "t":
      r[:, 17:20] += (1e-5 * np.maximum(size, 0.01))[:, None].astype(np.float32) * v.astype(np.float32)
    else:
      R = _small_rot(v, 2e-5)
      r[:, 20:29] = np.einsum("ij,njk->nik", R, recs[:, 20:29].reshape(-1, 3, 3).astype(float)).reshape(-1, 9).astype(np.float32)
    o = _oracle(r, mv, 64)
    has = (o[:, 0] >= 1) & (o64[:, 0] >= 1)
    wit = np.abs(o[:, 2:8] - o64[:, 2:8]).max(1) > thr
    nrm = np.abs(_unit(o[:, 2:5] - o[:, 5:8]) - n0).max(1) > 1e-3
    bad = (o[:, 0] != o64[:, 0]) | (has & (np.abs(o[:, 1] - o64[:, 1]) > 1e-5 + 1e-4 * size))
    amb = np.maximum(amb, np.where(bad | (has & nrm), 2, np.where(has & wit, 1, 0)))
  return amb


# ---- acceptance rule ----------------------------------------------------------------------------------------------
def _unit(v):
  n = np.linalg.norm(v, axis=-1, keepdims=True)
  return v / np.where(n > 0, n, 1)


def meets_bars(recs, got, want, amb):
  """Per case: `got` against `want` at the project's bars (count, 2e-5 distance, witness points 2e-4 / 2e-3); `amb`
  (ambiguity()) names the cases whose witness points, or normal too, the fp64 oracle itself shows to be undefined."""
  smooth = np.isin(recs[:, 0], (ELLIPSOID, CYLINDER)) | np.isin(recs[:, 1], (ELLIPSOID, CYLINDER))
  tolp = np.where(smooth, 2e-3, 2e-4)
  same = got[:, 0] == want[:, 0]
  none = want[:, 0] < 1  # EPA gave up: no contact, nothing further to compare
  dist = np.abs(got[:, 1] - want[:, 1]) <= 2e-5
  wit = np.abs(got[:, 2:8] - want[:, 2:8]).max(1) <= tolp
  nrm = np.abs(_unit(got[:, 2:5] - got[:, 5:8]) - _unit(want[:, 2:5] - want[:, 5:8])).max(1) <= 2e-3
  multi = (recs[:, 35] != 0) | (amb == 1)
  # 2: the direction is ambiguous too; what is left to ask of the witness points is that they are as far apart as the
  # distance says
  sym = (amb == 2) & (recs[:, 35] == 0)
  gap = np.abs(np.linalg.norm(got[:, 2:5] - got[:, 5:8], axis=1) - np.abs(got[:, 1])) <= tolp
  return same & (none | (dist & np.where(sym, gap, np.where(multi, nrm, wit))))


def equals_build(got, build):
  """tests/test_gpu_golden.py: same count, distance within 1e-6 absolute or 1e-4 relative."""
  return (got[:, 0] == build[:, 0]) & ((build[:, 0] < 1) | (np.abs(got[:, 1] - build[:, 1]) <= np.maximum(1e-6, 1e-4 * np.abs(build[:, 1]))))


def property_ok(name, got, idx):
  """The path-independent check of the unmatched cases `idx` (see the module docstring)."""
  fam, ref = family(name), references(name)
  recs, mv = fam.arrays()
  ok = np.zeros(len(idx), bool)
  if not len(idx):
    return ok
  sub, g, deep = recs[idx].copy(), got[idx], ref["deep"][idx]
  # "EPA converged": the device keeps no trace, so the strict clause holds where EPA (or, when EPA did not run, GJK)
  # converged in the fp64 oracle and in both fp32 builds; a result of no contact is an EPA that gave up
  conv = np.ones(len(idx), bool)
  for key in ("trace", "trace32", "trace32f"):
    tr = ref[key][idx]
    conv &= np.isin(tr[:, T["epa_exit"]], (1, 2)) | ((tr[:, T["epa_exit"]] == 0) & (tr[:, T["gjk_iter"]] < recs[idx, 34]))
  has = g[:, 0] >= 1
  # geom2 moved by |dist| along x1 - x2: out of a penetration, or up to geom1 from a separation (the witness points meet)
  n = _unit(g[:, 2:5] - g[:, 5:8])
  sub[:, 17:20] += (np.where(has, np.abs(g[:, 1]), 0.0)[:, None] * n).astype(np.float32)
  sub[:, 34], sub[:, 35] = 64, 0
  moved = _oracle(sub, mv, 64)
  # slack: 2e-5 + tolerance, and the fp32 rounding of the moved position (the record is fp32)
  slack = 2e-5 + recs[idx, 33].astype(float) + 4 * np.spacing(np.abs(sub[:, 17:20]).max(1).astype(np.float32)).astype(float)
  dmoved = np.where(moved[:, 0] >= 1, moved[:, 1], -1e9)
  for k in range(len(idx)):
    if not has[k]:  # EPA gave up (depth 0, nothing moved): the pair has to be in touch or inside, as the oracle's EPA exits are
      ok[k] = deep[k, 0] < 1 or deep[k, 1] <= slack[k]
    else:  # signed: a distance never below the true one (a depth never above it) ...
      not_deeper = deep[k, 0] < 1 or g[k, 1] >= deep[k, 1] - 2e-5
      # ... and the move ends in touch (converged) or still inside (stopped early)
      sep = abs(dmoved[k]) <= slack[k] if conv[k] else dmoved[k] <= slack[k]
      ok[k] = not_deeper and sep
  return ok


def classify(name, got, others):
  """Apply the rule to `got` (n, 8); `others`: the fp32 oracle results a tie may lean on.  Returns a dict with the
  per-case class (0 pass, 1 tie, 2 unmatched), the property verdict of the unmatched and the shares."""
  fam, ref = family(name), references(name)
  recs, _ = fam.arrays()
  got = np.asarray(got, np.float64)
  ok = meets_bars(recs, got, ref["o64"], ref["amb"])
  build_misses = np.zeros(len(recs), bool)
  equal = np.zeros(len(recs), bool)
  for b in others:
    build_misses |= ~meets_bars(recs, b, ref["o64"], ref["amb"])
    equal |= equals_build(got, b)
  cls = np.where(ok, 0, np.where(build_misses & equal, 1, 2))
  un = np.nonzero(cls == 2)[0]
  prop = property_ok(name, got, un)
  n = len(recs)
  err = np.abs(got[:, 1] - ref["o64"][:, 1])[(got[:, 0] >= 1) & (ref["o64"][:, 0] >= 1) & (cls == 0)]
  return dict(cls=cls, unmatched=un, property=prop, n=n, tie=float((cls == 1).sum()) / n, un=float(len(un)) / n,
              passed=float((cls == 0).sum()) / n, worst_dist=float(err.max()) if len(err) else 0.0,
              tie_cap=CAPS["tie_capped" if fam.capped else "tie_default"], un_cap=CAPS["unmatched"])


def verdict(name, res, share=1.0):
  """Failure strings of a classify() result against `share` of the caps."""
  fam = family(name)
  out = []
  if res["tie"] > share * res["tie_cap"]:
    out.append(f"{name}: ties {res['tie']:.4f} > {share * res['tie_cap']}: " + ", ".join(fam.ids[i] for i in np.nonzero(res["cls"] == 1)[0][:8]))
  if res["un"] > share * res["un_cap"]:
    out.append(f"{name}: unmatched {res['un']:.4f} > {share * res['un_cap']}: " + ", ".join(fam.ids[i] for i in res["unmatched"][:8]))
  bad = res["unmatched"][~res["property"]]
  if len(bad):
    out.append(f"{name}: unmatched cases fail the depth / separation property: " + ", ".join(fam.ids[i] for i in bad[:8]))
  return out


def check_predicates(name):
  """(failures, reached): the cases whose predicate fails on the fp64 trace, and what the family reaches."""
  fam, ref = family(name), references(name)
  bad = []
  for i, p in enumerate(fam.preds):
    if p is not None and not p[1](ref["trace"][i], ref["o64"][i]):
      bad.append(f"{name}/{fam.ids[i]}: {p[0]}: trace {dict(zip(TRACE, ref['trace'][i].tolist()))} out {ref['o64'][i, :2].tolist()}")
  return bad, reached(ref["trace"])


def reached(tr):
  ran = tr[:, T["cap_face"]] > 0
  return dict(
    routes=sorted(int(r) for r in np.unique(tr[ran, T["route"]])),
    exits=sorted(int(e) for e in np.unique(tr[:, T["epa_exit"]]) if e),
    dim_lt2=int(((tr[:, T["gjk_dim"]] < 2) & (tr[:, T["cap_face"]] == 0) & (tr[:, T["inflated"]] == 0)).sum()),
    status=sorted(int(s) for s in np.unique(tr[ran, T["status"]])),
    peak_nvert=int(tr[:, T["nvert"]].max()), peak_horizon=int(tr[:, T["horizon"]].max()),
    peak_face_fill=float(np.max(np.where(ran, tr[:, T["nface"]] / np.maximum(tr[:, T["cap_face"]], 1), 0))),
    multi=int(tr[:, T["multi"]].sum()), poly_np=sorted(int(v) for v in np.unique(tr[tr[:, T["multi"]] > 0, T["poly_np"]])),
  )


# ---- device -------------------------------------------------------------------------------------------------------
OUT_PTS = 32  # mjw_kat(2, ...): the 8 floats, then the contact points on geom1 (w1[4][3]) and on geom2 (w2[4][3])


def _kat(which, recs, aux, nout):
  import torch

  from mujoco_warp_amd import _lib

  L = _lib.lib()
  dev = torch.device("cuda", 0)
  x = torch.as_tensor(np.ascontiguousarray(recs, np.float32).reshape(-1), device=dev)
  a = torch.as_tensor(np.ascontiguousarray(aux, np.float32).reshape(-1), device=dev)
  out = torch.full((len(recs) * nout,), float("nan"), dtype=torch.float32, device=dev)
  _lib.check(L.mjw_kat(which, x.data_ptr(), a.data_ptr(), out.data_ptr(), len(recs), torch.cuda.current_stream(dev).cuda_stream), "mjw_kat")
  torch.cuda.synchronize()
  return out.cpu().numpy().reshape(len(recs), nout).astype(np.float64)


def run_device(name, points=False):
  """The family through mjw_kat: one launch, one wavefront per case; (n, 8) float64, or (n, 32) with the points."""
  fam = family(name)
  recs, _ = fam.arrays()
  return _kat(2 if points else 0, recs, fam.aux(), OUT_PTS if points else OUT)


def box_points_outside(recs, got):
  """Box-box records with multi-contact: every reported contact point -- on geom1 and on geom2 -- has to lie inside both
  faces, i.e. within both boxes grown by the reported depth (the faces are that far apart) + 1e-5 for fp32.  Returns the
  offending (case, point) list.  Computed in fp64 from the record."""
  bad = []
  for c in range(len(recs)):
    r = recs[c].astype(np.float64)
    n = int(got[c, 0])
    if not (r[0] == BOX and r[1] == BOX and r[35] != 0) or n < 1:
      continue
    grow = abs(got[c, 1]) + 1e-5
    for i in range(n):
      for p in (got[c, 8 + 3 * i:11 + 3 * i], got[c, 20 + 3 * i:23 + 3 * i]):
        for pos, R, size in ((r[2:5], r[5:14].reshape(3, 3), r[14:17]), (r[17:20], r[20:29].reshape(3, 3), r[29:32])):
          if (np.abs(R.T @ (p - pos)) > size + grow).any():
            bad.append((c, i))
  return sorted(set(bad))


# ---- the mesh support alone -----------------------------------------------------------------------------------------
def support_cases():
  """(records (n, 8): vertadr nvert dir[3], vertices, expected index or -1, ids) for mjw_kat(3, ...): ccd_support of
  every mesh of the meshverts family along the axis directions and seeded ones.  Expected: the first vertex that attains
  the largest dot product.  Along a single axis the products are exact, so the index is pinned; along the others the
  winner must attain the maximum to fp32 rounding and be the lowest index among the vertices equal to it."""
  fam = family("meshverts")
  mv = fam.pool.verts()
  rng = np.random.default_rng(17)
  dirs = [np.array(a, float) / np.linalg.norm(a) for a in AXES] + [rand_dir(rng) for _ in range(6)]
  recs, want, ids = [], [], []
  for name, (adr, n) in fam.pool.key.items():
    v = mv[adr:adr + n].astype(np.float64)
    for k, d in enumerate(dirs):
      d32 = d.astype(np.float32)
      recs.append(np.array([adr, n, *d32, 0, 0, 0], np.float32))
      exact = np.count_nonzero(d32) == 1
      want.append(int(np.argmax(v @ d32.astype(np.float64))) if exact else -1)
      ids.append(f"{name}-d{k}")
  return np.stack(recs), mv, np.array(want), ids


def support_failures(recs, mv, want, ids, got):
  bad = []
  for c in range(len(recs)):
    adr, n = int(recs[c, 0]), int(recs[c, 1])
    v = mv[adr:adr + n].astype(np.float64)
    dots = v @ recs[c, 2:5].astype(np.float64)
    i = int(got[c, 0])
    if not 0 <= i < n:
      bad.append(f"{ids[c]}: index {i} out of range")
    elif want[c] >= 0 and i != want[c]:
      bad.append(f"{ids[c]}: vertex {i}, the first maximum is {want[c]}")
    elif dots[i] < dots.max() - 4e-7 * np.abs(v).max():
      bad.append(f"{ids[c]}: vertex {i} is not a support point ({dots[i]} < {dots.max()})")
    elif i != int(np.nonzero((v == v[i]).all(1))[0][0]):
      bad.append(f"{ids[c]}: vertex {i} has an equal vertex at a lower index")
    elif np.abs(got[c, 1:4] - v[i]).max() > 0:
      bad.append(f"{ids[c]}: point {got[c, 1:4]} is not vertex {i}")
  return bad
