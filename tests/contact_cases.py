"""Contact staging, pair compaction and row cuts at every count edge: the fixture, the checker and the case list.

The forward kernels find a world's contacts and build its constraint rows in one wave-wide loop
(csrc/mjw_step.hip collision_and_constraints): the nxn pairs are filtered in passes of 64 lanes and compacted,
the survivors' contacts (0, 1 or 2 per primitive pair, 0..8 plane-box corners, 0..4 pre-pass points) are
prefix-scanned and staged in LDS in rounds of `cmax` -- 16 on the direct and fused dense path, 32 on the generic
world-per-wave path and in every single-stage launch (make_layout) -- each round reserves its pool slots with one
atomic (the first also carries the broadphase count), assigns rows by a second scan and cuts them at njmax,
and drops the contacts past naconmax with their rows.  The sparse path (csrc/mjw_sparse.hip collision) counts,
reserves and writes per block of BLK = 256 threads.

`ladder_xml` builds a synthetic scene with an exact contact set per world: one plane, bodies on vertical slide
joints that carry spheres (1 contact when lowered), horizontal capsules (2), flat boxes (4 corners) or tilted
boxes (1 corner), and optionally one box over a static box (the convex pre-pass, 4 points under MULTICCD).
contype / conaffinity leave only the plane-geom pairs (and the one box-box pair), so nxn is the number of body
geoms and pair order is geom order.  A world's state says which bodies are `down` (every geom penetrates by
PEN), `up` (CLEAR above the plane) or `near` (capsules / boxes only: the bounding sphere reaches the plane, the
shape stays NEAR above it -- a broadphase survivor without a contact).  These bands make fp32 and fp64 decide
every contact and every survivor alike (tests/test_contact_cases.py asserts them on the oracle), so the expected
survivor count is the number of lowered or near geoms and the expected contact list is the fp64 oracle's.

`check` compares a device view (`device_view`) with the oracle: contacts in slot order per world against the
oracle's list (pairs equal, dist / pos / normal at the primitive bar of test_collision_types.py, parameters
equal), row counts, row type / id (ids through the slot order), row values at the strict bar of
test_gpu_parity_strict.py, contact.efc_address and the two pool counters.

tests/test_contact_cases.py validates the fixture and the checker on the CPU oracle,
tests/test_gpu_contact_edges.py runs CASES on the device, tools/contact_edges.py writes the report.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

PEN, NEAR, CLEAR, DEEP = 2e-3, 1e-2, 1.0, 3e-3  # the poses: q = -PEN (down), +NEAR (near), +CLEAR (up), -DEEP (deep)
POSE = {"up": CLEAR, "down": -PEN, "near": NEAR, "deep": -DEEP}
PRIM_TOL = (2e-6, 2e-6, 2e-6)  # dist, pos, normal: tests/test_collision_types.py, primitive pairs
CONVEX_TOL = (2e-5, 2e-4, 2e-4)  # the same file's bar for the box-box driver scenes
RTOL, FLOOR = 1e-5, 1e-6  # tests/test_gpu_parity_strict.py
CMAX = {"direct": 16, "fused": 16, "generic": 32, "sparse": 256}  # the staging size (sparse: the block's width)
NCON = {"S": 1, "C": 2, "F": 4, "T": 1, "B": 4}  # contacts of a lowered geom
SPACING = 0.1  # bodies along x: coordinates stay small (an fp32 coordinate near 20 is only good to 1e-6)

SPHERE_R = 0.05
CAP_R, CAP_H = 0.04, 0.08
FLAT = (0.06, 0.05, 0.03)
TILT = (0.05, 0.04, 0.03)
BOXB, BOXB_YAW = (0.05, 0.04, 0.03), np.deg2rad(25.0)
# the static box under the B geom: its top face in the plane z = 0 (it shares the world body with the plane, so the two do
# not collide); higher up, the fp32 rounding of the coordinates alone (6e-8 at z = 1) exceeds the strict row bar on a
# penetration of PEN (1e-5 * 2e-3)
STATIC, STATIC_Z = (0.15, 0.15, 0.1), -0.1


def _tilt():
  """(quat, centre height) of the tilted box: Ry(20 deg) Rx(15 deg), one lowest corner at z = 0 for q = 0 (the next
  corner is 0.019 higher)."""
  ay, ax = np.deg2rad(20.0), np.deg2rad(15.0)
  qy = np.array([np.cos(ay / 2), 0.0, np.sin(ay / 2), 0.0])
  qx = np.array([np.cos(ax / 2), np.sin(ax / 2), 0.0, 0.0])
  w1, x1, y1, z1 = qy
  w2, x2, y2, z2 = qx
  q = np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])
  w, x, y, z = q
  row2 = np.array([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)])
  return q, float(np.abs(row2) @ np.array(TILT))


TILT_QUAT, TILT_Z = _tilt()


def _f(v):
  return " ".join(repr(float(x)) for x in np.atleast_1d(v))


def ladder_xml(bodies, path, nlimit=0, cone="pyramidal", npad=0):
  """MJCF of the contact ladder.  bodies: per body a list of (kind, condim), kind in S C F T B; the first `nlimit`
  bodies' joints are limited to q >= 0 (a limit row when lowered); `npad` bodies without a colliding geom follow
  (they only raise nv).  path: direct (Newton: never the fused kernel), fused (CG, explicit Euler), generic, sparse."""
  solver = "Newton" if path == "direct" else "CG"
  jac = "sparse" if path == "sparse" else "dense"
  hasb = any(k == "B" for b in bodies for k, _ in b)
  flags = ('<flag eulerdamp="disable"' if path == "fused" else "<flag") + (' multiccd="enable"/>' if hasb else "/>")
  s = [f'<mujoco><option timestep="0.002" cone="{cone}" solver="{solver}" jacobian="{jac}">{flags}</option><worldbody>'
       '<geom type="plane" size="20 20 .1" contype="1" conaffinity="0" condim="1"/>']
  for b, geoms in enumerate(bodies):
    for i, (k, _) in enumerate(geoms):
      if k == "B":
        s.append(f'<geom type="box" size="{_f(STATIC)}" pos="{_f((b * SPACING, 0.25 * i, STATIC_Z))}" contype="2" conaffinity="0" condim="1"/>')
  for b, geoms in enumerate(bodies):
    lim = ' limited="true" range="0 3"' if b < nlimit else ""
    s.append(f'<body pos="{_f((b * SPACING, 0, 0))}"><joint type="slide" axis="0 0 1"{lim}/>')
    for i, (k, condim) in enumerate(geoms):
      y, col = 0.25 * i, f'contype="0" conaffinity="{2 if k == "B" else 1}" condim="{condim}"'
      if k == "S":
        s.append(f'<geom type="sphere" size="{SPHERE_R}" pos="0 {y} {SPHERE_R}" {col}/>')
      elif k == "C":
        s.append(f'<geom type="capsule" size="{CAP_R}" fromto="{-CAP_H} {y} {CAP_R} {CAP_H} {y} {CAP_R}" {col}/>')
      elif k == "F":
        s.append(f'<geom type="box" size="{_f(FLAT)}" pos="0 {y} {FLAT[2]}" {col}/>')
      elif k == "T":
        s.append(f'<geom type="box" size="{_f(TILT)}" pos="0 {y} {TILT_Z!r}" quat="{_f(TILT_QUAT)}" {col}/>')
      elif k == "B":
        q = (np.cos(BOXB_YAW / 2), 0.0, 0.0, np.sin(BOXB_YAW / 2))
        s.append(f'<geom type="box" size="{_f(BOXB)}" pos="0 {y} {STATIC_Z + STATIC[2] + BOXB[2]!r}" quat="{_f(q)}" {col}/>')
      else:
        raise ValueError(k)
    s.append("</body>")
  for p in range(npad):
    s.append(f'<body pos="{_f(((len(bodies) + p) * SPACING, 0, 0))}"><joint type="slide" axis="0 0 1"/>'
             f'<geom type="sphere" size="{SPHERE_R}" pos="0 0 {SPHERE_R}" contype="0" conaffinity="0"/></body>')
  s.append("</worldbody></mujoco>")
  return "".join(s)


def S(n, condim=1):
  """n bodies with one sphere each."""
  return [[("S", condim)] for _ in range(n)]


def SS(n, k=2, condim=1):
  """n bodies with k spheres each."""
  return [[("S", condim)] * k for _ in range(n)]


def body_ncon(geoms, pose="down"):
  return sum(NCON[k] for k, _ in geoms) if pose in ("down", "deep") else 0


def nrows(condim, cone):
  return 1 if condim == 1 else (condim if cone == "elliptic" else 2 * (condim - 1))


def body_nrow(geoms, cone, limited=False):
  return sum(NCON[k] * nrows(c, cone) for k, c in geoms) + int(limited)


def pick(weights, target, among=None):
  """Indices (in order) of a subset of `among` whose weights sum to `target`: greedy in order, the last items
  chosen so that the sum is exact."""
  idx = list(range(len(weights))) if among is None else list(among)
  # reach[n]: the sums the items idx[n:] can make
  reach = [set() for _ in range(len(idx) + 1)]
  reach[len(idx)] = {0}
  for n in range(len(idx) - 1, -1, -1):
    w = weights[idx[n]]
    reach[n] = reach[n + 1] | {t + w for t in reach[n + 1] if t + w <= target}
  assert target in reach[0], (target, sorted(reach[0])[-3:])
  out, rest = [], target
  for n, i in enumerate(idx):
    w = weights[i]
    if 0 < w <= rest and rest - w in reach[n + 1]:
      out.append(i)
      rest -= w
  assert rest == 0, (target, rest)
  return out


def lower(bodies, count, among=None, pose="down"):
  """A world with exactly `count` contacts: {body: pose} lowering bodies of `among` (default all) in order."""
  return {b: pose for b in pick([body_ncon(g) for g in bodies], count, among)}


class Case:
  """One forward on the worlds of `worlds` ({body: pose} each, default up).  `expect` names what the CPU test verifies about
  the construction: ("straddle", world, first index, n), ("cut", world, kind), ("pool", naconmax)."""

  def __init__(self, id, path, bodies, worlds, njmax=64, nlimit=0, cone="pyramidal", npad=0, naconmax=None, adjacent=True, expect=()):
    self.id, self.path, self.bodies, self.worlds = id, path, bodies, worlds
    self.njmax, self.nlimit, self.cone, self.npad, self.naconmax, self.adjacent = njmax, nlimit, cone, npad, naconmax, adjacent
    self.expect = tuple(expect)
    self.nworld = len(worlds)
    self.box = any(k in "FTB" for b in bodies for k, _ in b)
    self.ccd = any(k == "B" for b in bodies for k, _ in b)
    self.nv = len(bodies) + npad
    self.cmax = CMAX[path]
    assert self.nworld <= 16, id
    if path in ("direct", "fused"):
      assert njmax <= 64 and self.nv <= 32, id
    if path == "fused":
      assert 17 <= self.nv <= 28 and not self.box and cone == "pyramidal", id
    if path == "generic":
      assert (njmax > 64 or self.nv > 32) and self.nv <= 64, id

  def xml(self):
    return ladder_xml(self.bodies, self.path, self.nlimit, self.cone, self.npad)

  def model(self):
    from mujoco_warp_amd import mjcf

    return mjcf.load_model_from_string(self.xml())

  def states(self, mjm, worlds=None):
    """(qpos, qvel, ctrl): qvel ~ N(0, 0.3), seeded by the case id."""
    worlds = self.worlds if worlds is None else worlds
    rng = np.random.default_rng(sum(ord(c) for c in self.id))
    qpos = np.full((len(worlds), mjm.nq), CLEAR)
    for w, poses in enumerate(worlds):
      for b, p in poses.items():
        qpos[w, b] = POSE[p]
    return qpos, rng.normal(0, 0.3, (len(worlds), mjm.nv)), np.zeros((len(worlds), mjm.nu))

  def geom_bodies(self):
    """(body, kind, condim) per pair, in pair order: the plane-geom pairs in geom order, then the box-box pair."""
    plane = [(b, k, c) for b, g in enumerate(self.bodies) for k, c in g if k != "B"]
    return plane + [(b, k, c) for b, g in enumerate(self.bodies) for k, c in g if k == "B"]

  def geoms(self):
    """(geom id, body, kind) of the body geoms: the plane is geom 0, the static boxes follow, then the bodies' geoms."""
    first = 1 + sum(k == "B" for g in self.bodies for k, _ in g)
    out = []
    for b, g in enumerate(self.bodies):
      for k, _ in g:
        out.append((first + len(out), b, k))
    return out

  @property
  def nxn(self):
    return len(self.geom_bodies())

  def survivors(self, worlds=None):
    """Expected broadphase survivors per world: the geoms of the lowered and near bodies."""
    worlds = self.worlds if worlds is None else worlds
    return [sum(len(self.bodies[b]) for b, p in poses.items() if p != "up") for poses in worlds]

  def contacts(self, worlds=None):
    """Expected contact count per world, from the construction."""
    worlds = self.worlds if worlds is None else worlds
    return [sum(body_ncon(self.bodies[b], p) for b, p in poses.items()) for poses in worlds]

  def contact_list(self, poses):
    """(pair index, body, kind, condim) per expected contact of a world, in pair order."""
    out = []
    for p, (b, k, c) in enumerate(self.geom_bodies()):
      if poses.get(b, "up") in ("down", "deep"):
        out += [(p, b, k, c)] * NCON[k]
    return out

  def rows(self, poses):
    """(limit rows, rows per expected contact) of a world, from the construction."""
    nl = sum(1 for b, p in poses.items() if b < self.nlimit and p in ("down", "deep"))
    return nl, [nrows(c, self.cone) for _, _, _, c in self.contact_list(poses)]

  def pool_size(self):
    """naconmax of the device Data: the case's cut, or every contact of every world."""
    return self.naconmax if self.naconmax is not None else max(1, sum(self.contacts()))

  def oracle_nconmax(self):
    """The oracle's pool is per world: the device's cut when the case has one world, else room for everything."""
    if self.naconmax is not None and self.nworld == 1:
      return self.naconmax
    return max(1, max(self.contacts()))

  def oracle(self, mjm, states=None, real_bits=64):
    from tests.common import oracle_from_state

    states = self.states(mjm) if states is None else states
    od = oracle_from_state(mjm, *states, njmax=self.njmax, nconmax=self.oracle_nconmax(), real_bits=real_bits)[1]
    od.forward()
    return od


# ---- the cases ------------------------------------------------------------------------------------------
def _ladder(path):
  """Single-contact geoms, one world each at 0, 1, C-1, C, C+1, 2C-1, 2C, 2C+1 contacts; box-free and with boxes."""
  C = CMAX[path]
  counts = (0, 1, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1)
  out = []
  for box in (False, True):
    if path == "fused" and box:
      continue
    one = [("T", 1)] if box else [("S", 1)]
    two = [("S", 1), ("T", 1)] if box else [("S", 1)] * 2
    if path == "direct":  # 32 bodies, 33 contacts: one body carries two geoms
      bodies = [list(one) for _ in range(31)] + [list(two)]
    elif path == "fused":  # 28 bodies: five carry two spheres
      bodies = [list(one) for _ in range(23)] + [list(two) for _ in range(5)]
    else:  # generic: 33 bodies (nv > 32), 65 contacts, njmax 96
      bodies = [list(one)] + [list(two) for _ in range(32)]
    worlds = [lower(bodies, c) for c in counts]
    out.append(Case(f"ladder-{path}-{'box' if box else 'prim'}", path, bodies, worlds, njmax=96 if path == "generic" else 64))
  return out


def _straddle(path, kind):
  """k single contacts, then a multi-contact pair whose last contact has world-local index C-1, C, C+1, C+2, whose
  first contact has index C, and which splits evenly over the 2C boundary; one single contact follows the pair
  (plane pairs only: the box-box pair is the last pair of the list)."""
  C, n = CMAX[path], NCON[kind]
  firsts = sorted({C - 1 - (n - 1), C - (n - 1), C + 1 - (n - 1), C + 2 - (n - 1), C, 2 * C - n // 2})
  nlead = max(firsts)
  if path == "fused":  # 28 dofs at the most: pairs of spheres carry the lead
    lead = SS(nlead // 3) + S(nlead - 2 * (nlead // 3))
  else:
    lead = S(nlead)
  room = (28 if path == "fused" else 32 if path == "direct" else 64) - len(lead) - 1
  trail = S(1) if (room >= 1 and kind != "B") else []
  bodies = lead + [[(kind, 1)]] + trail
  pb = len(lead)
  worlds, expect = [], []
  for w, f in enumerate(firsts):
    poses = lower(bodies, f, among=range(len(lead)))
    poses[pb] = "down"
    if trail:
      poses[pb + 1] = "down"
    worlds.append(poses)
    expect.append(("straddle", w, f, n))
  njmax = 64 if path in ("direct", "fused") else 128
  return Case(f"straddle-{path}-{kind}", path, bodies, worlds, njmax=njmax, npad=max(0, 17 - len(bodies)) if path == "fused" else 0, expect=expect)


def _passes(path, nxn):
  """nxn pairs; worlds whose survivors are only the last pair, only pairs 63 and 64, only pairs 127 and 128, none, and
  (generic, sparse: njmax holds every row) all pairs.  The geoms of those pairs have bodies of their own."""
  special = sorted({p for p in (63, 64, 127, 128, 255, 256, nxn - 1) if 0 <= p < nxn})
  budget = {"direct": 32, "fused": 28, "generic": 40, "sparse": 40}[path]
  chunk = 0
  while True:  # the smallest bodies that fit the path's dof budget
    chunk += 1
    bodies, body_of, run = [], {}, 0
    for p in range(nxn):
      if p in special:
        body_of[p] = len(bodies)
        bodies.append([("S", 1)])
        run = 0
      else:
        if run == 0 or run == chunk:
          bodies.append([])
          run = 0
        bodies[-1].append(("S", 1))
        run += 1
    if len(bodies) <= budget:
      break
  worlds = [{body_of[nxn - 1]: "down"}]
  for a in (63, 127, 255):
    if a + 1 < nxn:
      worlds.append({body_of[a]: "down", body_of[a + 1]: "down"})
  worlds.append({})
  njmax = 64
  if path in ("generic", "sparse"):
    worlds.append({b: "down" for b in range(len(bodies))})
    njmax = max(96, 32 * (-(-(nxn + 8) // 32)))
  worlds.append({body_of[nxn - 1]: "down"})  # the last pair again, after the full world
  return Case(f"passes-{path}-nxn{nxn}", path, bodies, worlds, njmax=njmax, npad=max(0, 17 - len(bodies)) if path == "fused" else 0)


def _cuts(path):
  """njmax cuts: a world with limit rows and contacts of condim 1 and 3 (and 4, 6), between two worlds that fill
  their rows exactly."""
  C = CMAX[path]
  out = []

  def case(tag, bodies, nlimit, cut, kind, njmax, cone="pyramidal", npad=0):
    weights = [body_nrow(g, cone, b < nlimit) for b, g in enumerate(bodies)]
    full = {b: "down" for b in pick(weights, njmax)}
    full2 = {b: "down" for b in pick(weights[::-1], njmax)}
    full2 = {len(bodies) - 1 - b: p for b, p in full2.items()}
    out.append(Case(f"cut-{path}-{tag}", path, bodies, [full, cut, full2, {}], njmax=njmax, nlimit=nlimit, cone=cone, npad=npad,
                    expect=[("cut", 1, kind), ("full", 0), ("full", 2)]))

  nb = {"direct": 32, "fused": 28, "generic": 40, "sparse": 40}[path]
  # 4 limited condim-1 spheres, 6 condim-1, 6 condim-3, then condim 1: rows 4 | 4 + 6 | 6 x 4 | ...
  bodies = S(10) + S(6, 3) + S(nb - 16)
  down = {b: "down" for b in range(16)}
  # limits 0..3, contacts: rows 4..13 (condim 1), 14..37 (condim 3)
  case("after", bodies, 4, down, "after", 18)  # (i) after the first pyramid: rows 14..17
  case("pyramid", bodies, 4, down, "pyramid", 20)  # (ii) two rows into the second pyramid
  if path != "fused":
    case("elliptic", bodies, 4, down, "pyramid", 19, cone="elliptic")  # rows 14..16, 17..19: 19 is two rows into the second
    b46 = S(10) + S(2, 3) + S(1, 4) + S(1, 6) + S(nb - 14)
    # rows: 4 limits, 10, 2 x 4 = 8 (to 22), condim 4: 6 rows (22..27), condim 6: 10 rows (28..37)
    case("dim46", b46, 4, {b: "down" for b in range(14)}, "pyramid", 31)
  lim = S(nb)
  case("limits", lim, 12, {b: "down" for b in range(12)}, "limits", 8)  # (iii) 12 limit rows, njmax 8
  if path == "sparse":  # its row pass has no staging round below 256 contacts
    return out
  # (iv) inside round two: C + 1 condim-1 contacts, then condim 3
  nb2 = nb
  b4 = S(C + 1) + S(nb2 - C - 1, 3)
  k = min(nb2, C + 4)
  case("round2", b4, 0, {b: "down" for b in range(k)}, "round2", C + 1 + 4 + 2)  # two rows into the second pyramid of round two
  case("round2-after", b4, 0, {b: "down" for b in range(k)}, "round2-after", C + 1 + 4)
  return out


def _pool(path):
  """nworld 1, naconmax at C-1, C, C+1: inside the flat box's four corners (contacts C-2 .. C+1), and box-free."""
  C = CMAX[path]
  out = []
  for box in (False, True):
    if path == "fused" and box:
      continue
    bodies = (S(C - 2) + [[("F", 1)]] + S(3)) if box else S(C + 5)
    pad = max(0, 17 - len(bodies)) if path == "fused" else (max(0, 33 - len(bodies)) if path == "generic" else 0)
    for n in (C - 1, C, C + 1):
      out.append(Case(f"pool-{path}-{'box' if box else 'prim'}-{n}", path, bodies, [{b: "down" for b in range(len(bodies))}], njmax=64, npad=pad,
                      naconmax=n, expect=[("pool", n)]))
  # several worlds share a pool that is too small: the invariants of the overflow test and the exact nacon
  bodies = S(C + 5)
  pad = max(0, 17 - len(bodies)) if path == "fused" else (max(0, 33 - len(bodies)) if path == "generic" else 0)
  worlds = [{b: "down" for b in range(n)} for n in (C + 5, 3, C + 1, 0)]
  out.append(Case(f"pool-{path}-shared", path, bodies, worlds, njmax=64, npad=pad, naconmax=2 * C - 3))
  return out


def _counters(path):
  """ncollision: worlds with no survivor, survivors without a contact (the trailing count-only atomic), more than C
  contacts (the count rides on round one's reservation only); counters adjacent and apart."""
  C = CMAX[path]
  out = []
  for box in (False, True):
    if path == "fused" and box:
      continue
    nearb = [[("T", 1)] for _ in range(3)] if box else [[("C", 1)] for _ in range(3)]
    nb = {"direct": 32, "fused": 28, "generic": 40, "sparse": 40}[path]
    bodies = nearb + SS(nb - 3, 8 if path == "sparse" else 2)
    many = lower(bodies, C + 8 if path == "sparse" else 2 * C + 2, among=range(3, len(bodies)))
    worlds = [{}, {0: "near", 1: "near", 2: "near"}, many, {0: "near"}, {**many, 0: "near", 1: "down"}, {}]
    for adjacent in (True, False):
      out.append(Case(f"counters-{path}-{'box' if box else 'prim'}-{'adjacent' if adjacent else 'apart'}", path, bodies, worlds,
                      njmax={"generic": 96, "sparse": 288}.get(path, 64), adjacent=adjacent))
  return out


def _sparse():
  """The sparse collision pass counts and writes per block of 256 threads (item = pair), its scan per wave of 64:
  contact counts and nxn at 63 / 64 / 65 and 255 / 256 / 257."""
  out = []
  counts = (0, 1, 63, 64, 65, 255, 256, 257)
  for box in (False, True):
    one = [("T", 1)] if box else [("S", 1)]
    bodies = [list(one) for _ in range(8)] + [list(one) * 8 for _ in range(32)]  # 8 + 256 contacts
    worlds = [lower(bodies, c) for c in counts]
    out.append(Case(f"ladder-sparse-{'box' if box else 'prim'}", "sparse", bodies, worlds, njmax=288))
  for nxn in (63, 64, 65, 255, 256, 257):
    out.append(_passes("sparse", nxn))
  out += _counters("sparse")
  out += _cuts("sparse")
  return out


def _cases():
  out = []
  for path in ("direct", "fused", "generic"):
    out += _ladder(path)
    for kind in ("C", "F", "B"):
      if path == "fused" and kind != "C":
        continue
      out.append(_straddle(path, kind))
    for nxn in (63, 64, 65, 128, 129):
      out.append(_passes(path, nxn))
    out += _cuts(path)
    out += _pool(path)
    out += _counters(path)
  out += _sparse()
  ids = [c.id for c in out]
  assert len(set(ids)) == len(ids)
  return out


CASES = _cases()


# ---- the views ------------------------------------------------------------------------------------------
CON_REAL = ("dist", "pos", "frame", "includemargin", "friction", "solref", "solimp")
CON_INT = ("dim", "geom", "worldid", "type", "efc_address")
EFC = ("type", "id", "pos", "vel", "D", "aref", "margin")
CONTACT_ROWS = (5, 6, 7)  # ConstraintType CONTACT_*


def device_view(m, d):
  """The arrays `check` reads, as numpy, from a device Data after forward / step."""
  from tests.common import dense_efc_J, np_

  nacon = int(d.nacon[0])
  n = min(nacon, d.naconmax)
  con = {k: np_(getattr(d.contact, k))[:n] for k in CON_REAL}
  con.update({k: getattr(d.contact, k)[:n].cpu().numpy() for k in CON_INT})
  con["pos"], con["frame"], con["geom"] = con["pos"].reshape(n, 3), con["frame"].reshape(n, 9), con["geom"].reshape(n, 2)
  con["efc_address"] = con["efc_address"].reshape(n, -1)
  efc = {k: (np_(getattr(d.efc, k))[:, :d.njmax] if k not in ("type", "id") else getattr(d.efc, k)[:, :d.njmax].cpu().numpy()) for k in EFC}
  counts = {k: getattr(d, k).cpu().numpy().ravel().astype(int) for k in ("ne", "nf", "nl", "nefc")}
  return dict(nacon=nacon, ncollision=int(d.ncollision[0]), naconmax=d.naconmax, njmax=d.njmax, nworld=d.nworld, con=con, efc=efc, counts=counts,
              J=[dense_efc_J(m, d, w) for w in range(d.nworld)])


def oracle_view(od, nv, nmaxpyramid, survivors, naconmax=None, interleave=False):
  """The oracle's own arrays in the device's shape (tests of the checker): the worlds' contacts in one pool, world by
  world, or -- interleave -- alternating between the worlds as concurrent reservations would leave them."""
  nw = od.nworld
  stored = [min(int(od.ncon[w, 0]), od.nconmax) for w in range(nw)]
  order = [(w, i) for w in range(nw) for i in range(stored[w])]
  if interleave:
    order.sort(key=lambda t: (t[1] // 3, t[0], t[1]))
  if naconmax is not None:
    order = order[:naconmax]
  n = len(order)
  wid = np.array([w for w, _ in order], int)
  idx = np.array([i for _, i in order], int)
  slot = {t: s for s, t in enumerate(order)}

  def take(name, width):
    a = getattr(od, "con_" + name).reshape(nw, od.nconmax, width)
    return a[wid, idx].astype(np.float64 if a.dtype.kind == "f" else int).reshape(n, width) if n else np.zeros((0, width))

  con = dict(dist=take("dist", 1)[:, 0], pos=take("pos", 3), frame=take("frame", 9), includemargin=take("includemargin", 1)[:, 0],
             friction=take("friction", 5), solref=take("solref", 2), solimp=take("solimp", 5), dim=take("dim", 1)[:, 0], geom=take("geom", 2),
             worldid=wid, type=np.ones(n, int), efc_address=take("efc_address", 10)[:, :nmaxpyramid])
  for k in ("dist", "pos", "frame", "includemargin", "friction", "solref", "solimp"):
    con[k] = con[k].astype(np.float32).astype(np.float64)
  efc = {k: getattr(od, "efc_" + k).copy() for k in EFC}
  for w in range(nw):  # contact rows carry the pool slot
    for r in range(min(int(od.nefc[w, 0]), od.njmax)):
      if efc["type"][w, r] in CONTACT_ROWS:
        efc["id"][w, r] = slot.get((w, int(efc["id"][w, r])), -1)
  counts = {k: getattr(od, k)[:, 0].astype(int) for k in ("ne", "nf", "nl", "nefc")}
  J = [od.efc_J[w].reshape(od.njmax, nv)[:min(int(od.nefc[w, 0]), od.njmax)].copy() for w in range(nw)]
  return dict(nacon=int(od.ncon.sum()), ncollision=int(sum(survivors)), naconmax=n if naconmax is None else naconmax, njmax=od.njmax, nworld=nw,
              con=con, efc=efc, counts=counts, J=J)


# ---- the checker ----------------------------------------------------------------------------------------
def _close(name, got, want):
  """The strict bar: |got - want| <= RTOL |want| + FLOOR max |want|."""
  from tests.common import assert_close

  want = np.asarray(want, np.float64)
  if want.size:
    assert_close(name, got, want, RTOL, FLOOR * float(np.abs(want).max()))


def check(view, od, survivors, nv, geom_type=None, contact_map=None, worst=None, nacon=None, skip_pos=()):
  """Assert the view against the oracle.  contact_map[w]: per stored contact of world w (slot order) the oracle
  contact it is, or None for one the oracle does not have (a contact that lost its CONSTRAINT bit: no rows, address -1);
  default: the oracle's own order.  `worst`, a dict, collects the largest errors seen.  nacon: the expected counter when it
  is not the oracle's total (contacts without rows stay in the pool); skip_pos: (world, stored index) of contacts whose
  position the oracle state does not reproduce (an edited dist)."""
  worst = {} if worst is None else worst

  def note(k, v):
    worst[k] = max(worst.get(k, 0.0), float(v))

  con, efc, njmax = view["con"], view["efc"], view["njmax"]
  assert njmax == od.njmax
  nacon = int(od.ncon.sum()) if nacon is None else nacon
  assert view["nacon"] == nacon, ("nacon", view["nacon"], nacon)
  assert view["ncollision"] == int(sum(survivors)), ("ncollision", view["ncollision"], int(sum(survivors)))
  assert len(con["worldid"]) == min(view["nacon"], view["naconmax"])
  npyr = con["efc_address"].shape[1]
  for w in range(view["nworld"]):
    sel = np.nonzero(con["worldid"] == w)[0]
    nst = min(int(od.ncon[w, 0]), od.nconmax)
    cmap = list(range(len(sel))) if contact_map is None else contact_map[w]
    assert len(cmap) == len(sel), (w, "stored contacts", len(sel), len(cmap))
    have = [j for j in cmap if j is not None]
    assert have == list(range(nst)), (w, "contacts", have, nst)
    local = {int(s): cmap[i] for i, s in enumerate(sel)}  # slot -> oracle contact
    og = od.con_geom[w].reshape(-1, 2)
    for i, s in enumerate(sel):
      j = cmap[i]
      if j is None:
        assert (con["efc_address"][s] == -1).all(), (w, i, "address of a contact without rows", con["efc_address"][s])
        continue
      assert tuple(con["geom"][s]) == tuple(og[j]), (w, i, "geom pair", tuple(con["geom"][s]), tuple(og[j]))
      convex = geom_type is not None and geom_type[og[j][0]] == 6 and geom_type[og[j][1]] == 6
      tol = CONVEX_TOL if convex else PRIM_TOL
      ed = abs(con["dist"][s] - od.con_dist[w, j])
      ep = 0.0 if (w, i) in skip_pos else np.abs(con["pos"][s] - od.con_pos[w, 3 * j:3 * j + 3]).max()
      en = np.abs(con["frame"][s, :3] - od.con_frame[w, 9 * j:9 * j + 3]).max()
      kind = "convex" if convex else "prim"
      note(kind + "_dist", ed), note(kind + "_pos", ep), note(kind + "_normal", en)
      assert ed <= tol[0] and ep <= tol[1] and en <= tol[2], (w, i, "dist / pos / normal", ed, ep, en, tol)
      assert con["dim"][s] == od.con_dim[w, j] and con["worldid"][s] == w and con["type"][s] == 1, (w, i, "dim / worldid / type")
      for k, width in (("includemargin", 1), ("friction", 5), ("solref", 2), ("solimp", 5)):
        want = getattr(od, "con_" + k)[w, width * j:width * j + width].astype(np.float32).astype(np.float64)
        assert np.array_equal(np.atleast_1d(con[k][s]), want), (w, i, k, con[k][s], want)
      want = od.con_efc_address[w, 10 * j:10 * j + npyr]
      assert np.array_equal(con["efc_address"][s], want), (w, i, "efc_address", con["efc_address"][s], want)
    for k in ("ne", "nf", "nl", "nefc"):
      assert int(view["counts"][k][w]) == int(getattr(od, k)[w, 0]), (w, k, int(view["counts"][k][w]), int(getattr(od, k)[w, 0]))
    n = min(int(od.nefc[w, 0]), njmax)
    assert np.array_equal(efc["type"][w, :n], od.efc_type[w, :n]), (w, "efc_type", efc["type"][w, :n], od.efc_type[w, :n])
    for r in range(n):
      got = int(efc["id"][w, r])
      if od.efc_type[w, r] in CONTACT_ROWS:
        assert got in local, (w, r, "efc_id: not a slot of this world", got)
        got = local[got]
      assert got == int(od.efc_id[w, r]), (w, r, "efc_id", got, int(od.efc_id[w, r]))
    J = np.asarray(view["J"][w], np.float64)
    assert J.shape == (n, nv), (w, "J", J.shape, (n, nv))
    oJ = od.efc_J[w].reshape(njmax, nv)[:n]
    _close(f"world {w} efc_J", J, oJ)
    if n:
      note("J", np.abs(J - oJ).max() / max(np.abs(oJ).max(), 1e-300))
    for k in ("pos", "vel", "D", "aref", "margin"):
      want = getattr(od, "efc_" + k)[w, :n]
      _close(f"world {w} efc_{k}", efc[k][w, :n], want)
      if n:
        note(k, np.abs(efc[k][w, :n] - want).max() / max(np.abs(want).max(), 1e-300))
  return worst


def check_shared_pool(view, od, survivors):
  """Several worlds over a pool that is too small (which world loses its contacts depends on the order of the atomics):
  nacon counts every contact found, every stored contact is one of its world's, every contact row points into the
  pool at a contact of its own world, and a world's rows are its limit rows plus the rows of its stored contacts."""
  con, efc = view["con"], view["efc"]
  assert view["nacon"] == int(od.ncon.sum()), ("nacon", view["nacon"], int(od.ncon.sum()))
  assert view["ncollision"] == int(sum(survivors)), ("ncollision", view["ncollision"], int(sum(survivors)))
  assert len(con["worldid"]) == view["naconmax"] < view["nacon"]
  for w in range(view["nworld"]):
    sel = np.nonzero(con["worldid"] == w)[0]
    assert len(sel) <= int(od.ncon[w, 0])
    want = {tuple(g) for g in od.con_geom[w].reshape(-1, 2)[:int(od.ncon[w, 0])]}
    assert all(tuple(g) in want for g in con["geom"][sel]), (w, "stored contact of another world")
    n = min(int(view["counts"]["nefc"][w]), view["njmax"])
    typ, ids = efc["type"][w, :n], efc["id"][w, :n]
    rows = np.isin(typ, CONTACT_ROWS)
    assert (ids[rows] < view["naconmax"]).all() and np.isin(ids[rows], sel).all(), (w, "row of a contact outside the pool")
    assert int(view["counts"]["nl"][w]) == int(od.nl[w, 0])
    # condim 1: one row per stored contact (all penetrate)
    assert int(view["counts"]["nefc"][w]) == int(od.nl[w, 0]) + len(sel), (w, int(view["counts"]["nefc"][w]), len(sel))
    assert sorted(ids[rows]) == sorted(sel), (w, "rows and stored contacts differ")


# ---- the device side ------------------------------------------------------------------------------------
def expected_kernels(case):
  """(kernel names that must run in the traced step, kernel-name prefixes that must not)."""
  box = "true" if case.box else "false"
  if case.path == "fused":
    return ["mjw::step_kernel<79, false, 7, false, 28>"], ("mjw::mjw_kernel", "mjw::dense_kernel", "mjw::sp::")
  if case.path == "direct":
    must = [f"mjw::mjw_kernel<79, {box}, false>"]
    ban = ("mjw::step_kernel", "mjw::sp::", "mjw::mjw_kernel<63")
  elif case.path == "generic":
    must = [f"mjw::mjw_kernel<63, {box}, false>"]
    ban = ("mjw::step_kernel", "mjw::sp::", "mjw::dense_kernel", "mjw::mjw_kernel<79")
  else:
    must = ["mjw::sp::forward_kernel<1024>", "mjw::sp::forward_kernel<2048>"]
    ban = ("mjw::step_kernel", "mjw::mjw_kernel", "mjw::dense_kernel")
  return must, ban


def check_kernels(case, names):
  must, ban = expected_kernels(case)
  for k in must:
    assert k in names, (case.id, k, names)
  assert not [n for n in names if n.startswith(ban)], (case.id, names)
  if case.path == "direct":
    assert any(n.startswith("mjw::dense_kernel") for n in names), (case.id, names)
  assert any("ccd_kernel" in n for n in names) == (case.ccd and case.path != "sparse") or case.path == "sparse", (case.id, names)


def device_data(case, mjm, states=None):
  """(m, d) with the case's state, pool size and counter placement."""
  import torch

  import mujoco_warp_amd as mjw

  qpos, qvel, ctrl = case.states(mjm) if states is None else states
  m = mjw.put_model(mjm, device="cuda")
  d = mjw.make_data(mjm, nworld=len(qpos), njmax=case.njmax, naconmax=case.pool_size(), device="cuda", m=m)
  d.qpos[:] = torch.as_tensor(qpos, dtype=torch.float32, device="cuda")
  d.qvel[:] = torch.as_tensor(qvel, dtype=torch.float32, device="cuda")
  if case.adjacent:
    assert d.ncollision.data_ptr() == d.nacon.data_ptr() + 4
  else:
    d.ncollision = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert d.ncollision.data_ptr() != d.nacon.data_ptr() + 4
  return m, d


def run_case(case):
  """One forward and one traced step of the case on the device, each checked; returns the report entry, its `failures`
  the assertions that did not hold as (where, text) pairs (none expected).  The fused
  kernel runs only as the whole step, so the step's Data (contacts and rows of the state before it) is checked with
  the same checker on every path."""
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd.forward import StepTracer

  mjm = case.model()
  od = case.oracle(mjm)
  surv = case.survivors()
  m, d = device_data(case, mjm)
  mjw.forward(m, d)
  m2, d2 = device_data(case, mjm)
  tracer = StepTracer()
  tracer.step(m2, d2)
  torch.cuda.synchronize()
  names = [k for k, _ in tracer.durations()[0] if not k.startswith("mjw::reset_counters")]
  res = dict(id=case.id, path=case.path, cmax=case.cmax, nxn=case.nxn, kernels=names, contacts=case.contacts(), survivors=surv)
  worst, failures = {}, []
  try:
    check_kernels(case, names)
  except AssertionError as e:
    failures.append(("kernels", str(e)[:2000]))
  for tag, mm, dd in (("forward", m, d), ("step", m2, d2)):
    view = device_view(mm, dd)
    res[tag] = dict(nacon=view["nacon"], ncollision=view["ncollision"], **{k: [int(x) for x in view["counts"][k]] for k in ("nl", "nefc")})
    try:
      if case.naconmax is not None and case.nworld > 1:
        check_shared_pool(view, od, surv)
      else:
        check(view, od, surv, mjm.nv, geom_type=np.asarray(mjm.geom_type), worst=worst)
    except AssertionError as e:
      failures.append((tag, str(e)[:2000]))
  res["worst"], res["failures"] = worst, failures
  res["bars"] = dict(prim=list(PRIM_TOL), convex=list(CONVEX_TOL), rows=[RTOL, FLOOR])
  return res


# ---- pool mode ------------------------------------------------------------------------------------------
class PoolCase(Case):
  """The rows rebuilt from an edited pool (the POOL path of collision_and_constraints: a contactfilter callback, then
  mjw_contact_rows; a single-stage launch, so the staging size is 32 on every dense model).  In every world with more
  than C contacts the callback clears the CONSTRAINT bit of the contacts at world-local indices C-1 and C and lowers
  the dist of contact EDIT by DEEP - PEN.  Spheres on vertical slides: a contact's rows depend on its own body only and
  its normal row's J does not depend on the contact point, so the expected rows are the oracle's for the state with the
  two bodies raised and EDIT's body at the `deep` pose."""

  EDIT = 3

  def __init__(self, id, counts, nbody=40, njmax=64):
    bodies = S(nbody)
    Case.__init__(self, id, "generic", bodies, [lower(bodies, c) for c in counts], njmax=njmax)
    self.cmax = 32

  def edited(self, w):
    return self.contacts()[w] > self.cmax

  def edited_worlds(self):
    """The worlds whose oracle gives the edited contact set."""
    out = []
    for w, poses in enumerate(self.worlds):
      poses = dict(poses)
      if self.edited(w):
        down = sorted(poses)
        del poses[down[self.cmax - 1]], poses[down[self.cmax]]
        poses[down[self.EDIT]] = "deep"
      out.append(poses)
    return out

  def contact_map(self):
    C = self.cmax
    return [[i if i < C - 1 else (None if i <= C else i - 2) for i in range(n)] if self.edited(w) else list(range(n))
            for w, n in enumerate(self.contacts())]

  def callback(self):
    """The contactfilter callback (m, d) that makes the edit."""
    import torch

    def edit(m, d):
      n = min(int(d.nacon[0]), d.naconmax)
      wid = d.contact.worldid[:n].cpu().numpy()
      for w in range(self.nworld):
        if self.edited(w):
          sel = np.nonzero(wid == w)[0]  # slot order = pair order
          idx = torch.as_tensor(sel[[self.cmax - 1, self.cmax]], device=d.contact.type.device)
          d.contact.type[idx] = 0
          d.contact.dist[int(sel[self.EDIT])] -= DEEP - PEN

    return edit


POOL_CASES = [PoolCase("poolmode-40", (5, 38, 35, 0, 40, 33)), PoolCase("poolmode-njmax", (34, 2, 40), njmax=36)]


def run_pool_case(case):
  """forward with the editing callback (staged: the position stage, the callback, the rows from the pool), checked against
  the oracle of the edited set."""
  import torch

  import mujoco_warp_amd as mjw

  mjm = case.model()
  worlds2 = case.edited_worlds()
  od2 = case.oracle(mjm, states=case.states(mjm, worlds2))
  m, d = device_data(case, mjm)
  m.callback.contactfilter = case.callback()
  mjw.forward(m, d)
  torch.cuda.synchronize()
  view = device_view(m, d)
  ranges = d.ncon_world.cpu().numpy().reshape(-1, 2)
  res = dict(id=case.id, path="pool", cmax=case.cmax, contacts=case.contacts(), ncon_world=[[int(a), int(b)] for a, b in ranges],
             nacon=view["nacon"], ncollision=view["ncollision"], nefc=[int(x) for x in view["counts"]["nefc"]])
  skip = {(w, case.EDIT) for w in range(case.nworld) if case.edited(w)}
  res["worst"] = check(view, od2, case.survivors(), mjm.nv, contact_map=case.contact_map(), nacon=sum(case.contacts()), skip_pos=skip, worst={})
  for w in range(case.nworld):  # the cleared contacts are still in the pool, without the bit
    sel = np.nonzero(view["con"]["worldid"] == w)[0]
    typ = view["con"]["type"][sel]
    want = np.ones(len(sel), int)
    if case.edited(w):
      want[[case.cmax - 1, case.cmax]] = 0
    assert np.array_equal(typ, want), (w, typ)
  return res
