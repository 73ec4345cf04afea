"""The sparse path at every tree-shape, stride and subtree-size edge: the fixtures, the checker and the case list.

csrc/mjw_sparse.hip picks its code by counts written into it: a tree's factor solve / M product runs dense in
registers for a parent chain of <= CHAIN = 4 dofs, as a compare-select over TREE = 8 registers for any other tree of
<= 8 dofs and as read-modify-write loops in HBM above that; every per-tree / per-dof / per-body / per-joint loop
strides by BLK = 256 threads; com_pos sums a body subtree of <= BIG = 64 bodies serially in one thread and a larger
one block-wide (NBIG = 16 at a time); the J-transpose column of a dof is sorted in registers up to SORTN = 32 entries
and by insertion in HBM above; the row loops keep RU = 4 rows in flight per thread; Newton builds, factors and solves
an nv x nv Hessian with a row per thread.

The fixtures put a count on both sides of each of these:

  zoo       one tree of every shape (chains of 1..9 hinges, ball / free roots, branched trees of 3, 4, 8, 9 dofs)
  pads      single-body trees on damped vertical slides after the zoo: ntree, nv, nbody, njnt at 255 / 256 / 257
  stars     a hinged root with L leaves on slides: a subtree of 64 (serial) or 65 (block sum) bodies, one of 901
  chain70   70 hinge bodies in a row: six nested big subtrees, a depth-71 tree for the ancestor walks
            (big subtrees are counted as the kernel counts them, the world body's included: `big_bodies`)
  ladder    solver_cases.ladder_xml on the sparse path: exact row counts 255 .. 1025, njmax above and equal
  columns   bodies on a vertical slide with k condim-1 spheres each: J-transpose columns of exactly k entries
  contact   the zoo lowered into the plane: rows of 1..9 non-zeros, nv at 255 / 256 / 257 under CG and Newton

`measure` turns a view of one run (the device's `device_run`, or the fp32 oracle's `oracle_run`) into one number per check
against the fp64 oracle, all in fp64 numpy; `bars` gives the project's bar of each.  tests/test_sparse_cases.py
validates the fixtures and asserts that the fp32 build of the oracle stays within half of every bar on every case
(the inputs leave the device headroom), tests/test_gpu_sparse_edges.py runs CASES on the device,
tools/sparse_edges.py writes the report.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from tests import solver_cases as sc  # noqa: E402
from tests.parity_models import SMOOTH  # noqa: E402

CHAIN, TREE, BLK, BIG, NBIG, SORTN, RU = 4, 8, 256, 64, 16, 32, 4  # csrc/mjw_sparse.hip
SMOOTH_TOL = 1e-5  # tests/test_gpu_parity_models.py: smooth fields and qM, normwise; the backward errors
QACC_TOL = 5e-3  # qacc after the solve, normwise
TREE_FIELDS = {"subtree_com": 3, "cinert": 10, "crb": 10, "cfrc_int": 6}  # checked per tree too (width per body)
STAGES = ("fwd_position", "fwd_velocity", "fwd_actuation", "fwd_acceleration")

ELL, RS = 0.1, 0.03  # zoo: link length, sphere radius
PR = 0.03  # pad sphere radius
PEN, UP = 2e-3, 0.3  # a lowered pad / column body penetrates by PEN, a raised one sits UP above the plane
JNT = 'armature="0.01" damping="0.1"'
# the colliding zoo: CG stops on a cost improvement below tolerance * meaninertia * nv, which leaves a dof of inertia 0.01
# 0.05 rad/s^2 from the optimum at nv = 256 (the fp32 oracle missed half the qacc bar); 0.2 leaves a quarter of that
JNT_CONTACT = 'armature="0.2" damping="0.1"'


# ---- the zoo --------------------------------------------------------------------------------------------
def _tree(kinds, leaves=0):
  """A parent chain of joints `kinds` (H hinge, B ball, F free) whose last body carries `leaves` hinged leaf bodies:
  nested (kind, children)."""
  tail = [("H", []) for _ in range(leaves)]
  for k in reversed(kinds):
    tail = [(k, tail)]
  return tail[0]


ZOO = ([_tree("H" * n) for n in (1, 2, 3, 4, 5, 8, 9)]
       + [_tree("B"), _tree("BH"), _tree("BHH"), _tree("F"), _tree("FH"), _tree("F", 2), _tree("F", 3), _tree("H", 2), _tree("H", 3),
          _tree("H" * 6, 2), _tree("H" * 7, 2)])
NDOF = {"H": 1, "B": 3, "F": 6, "S": 1}


def _count(node, what):
  k, ch = node
  return (NDOF[k] if what == "dof" else 1) + sum(_count(c, what) for c in ch)


ZOO_NV, ZOO_NBODY = sum(_count(t, "dof") for t in ZOO), sum(_count(t, "body") for t in ZOO)


def _zoo_body(node, pos, depth, collide, out):
  k, ch = node
  axis = "0 1 0" if depth % 2 == 0 else "0.2 1 0"
  jnt = JNT_CONTACT if collide else JNT
  joint = {"H": f'<joint type="hinge" axis="{axis}" {jnt}/>', "B": f'<joint type="ball" {jnt}/>', "F": f'<joint type="free" {jnt}/>'}[k]
  out.append(f'<body pos="{pos[0]!r} {pos[1]!r} {pos[2]!r}">{joint}'
             f'<geom type="sphere" size="{RS}" pos="{ELL} 0 0" contype="0" conaffinity="{int(collide)}" condim="1"/>')
  for i, c in enumerate(ch):
    _zoo_body(c, (ELL, 0.06 * (i - (len(ch) - 1) / 2), 0.0), depth + 1, collide, out)
  out.append("</body>")


def pad_xy(p):
  """Pads on a 50-wide grid inside |x|, |y| <= 1.9."""
  return -1.9 + 0.075 * (p % 50), -1.9 + 0.075 * (p // 50)


def zoo_xml(npad=0, collide=False, solver="CG", integrator="Euler", zoo=True):
  """The zoo (tree t rooted at (-0.5, -1.7 + 0.2 t, zh), extending along +x), then npad pads.  collide: the zoo's spheres
  collide with the plane and the roots sit RS above it (a horizontal link touches); the pads always do."""
  zh = RS if collide else 0.5
  s = [f'<mujoco><compiler angle="radian"/><option timestep="0.002" cone="pyramidal" solver="{solver}" jacobian="sparse" integrator="{integrator}"/>'
       '<worldbody><geom type="plane" size="5 5 .1" contype="1" conaffinity="0" condim="1"/>']
  if zoo:
    for t, tree in enumerate(ZOO):
      _zoo_body(tree, (-0.5, round(-1.7 + 0.2 * t, 6), zh), 0, collide, s)
  for p in range(npad):
    x, y = pad_xy(p)
    s.append(f'<body pos="{x!r} {y!r} 0"><joint type="slide" axis="0 0 1" {JNT}/>'
             f'<geom type="sphere" size="{PR}" pos="0 0 {PR}" contype="0" conaffinity="1" condim="1"/></body>')
  s.append("</worldbody></mujoco>")
  return "".join(s)


# ---- big subtrees ---------------------------------------------------------------------------------------
def _star(pos, L, out):
  """A hinged root with L leaf bodies on slides (axes x, y, z in turn) on a 4 cm grid around it: a subtree of L + 1."""
  out.append(f'<body pos="{pos[0]!r} {pos[1]!r} {pos[2]!r}"><joint type="hinge" axis="0 1 0" {JNT}/>'
             '<geom type="sphere" size="0.03" mass="0.2" contype="0" conaffinity="0"/>')
  side = int(np.ceil(np.sqrt(L)))
  for i in range(L):
    x, y = 0.04 * (i % side - (side - 1) / 2), 0.04 * (i // side - (side - 1) / 2)
    axis = ("1 0 0", "0 1 0", "0 0 1")[i % 3]
    mass = round(0.02 * (1 + 0.5 * ((7 * i) % 11) / 11), 6)  # unequal: 900 equal addends round the same way every time
    out.append(f'<body pos="{round(x, 6)!r} {round(y, 6)!r} -0.05"><joint type="slide" axis="{axis}" {JNT}/>'
               f'<geom type="sphere" size="0.015" mass="{mass!r}" contype="0" conaffinity="0"/></body>')
  out.append("</body>")


def _chain70(pos, out, n=70):
  """n hinge bodies with 3 cm links along +x."""
  for k in range(n):
    p = pos if k == 0 else (0.03, 0.0, 0.0)
    axis = "0 1 0" if k % 2 == 0 else "0.2 1 0"
    out.append(f'<body pos="{p[0]!r} {p[1]!r} {p[2]!r}"><joint type="hinge" axis="{axis}" {JNT}/>'
               '<geom type="sphere" size="0.01" pos="0.03 0 0" mass="0.05" contype="0" conaffinity="0"/>')
  out.append("</body>" * n)


def big_xml(items):
  """items: ("star", L) / ("chain",) in body order.  Chains start at x = -1.5 on rows 0.25 apart (z = 0.3), stars sit on a
  0.4 grid (a star of more than 100 leaves takes the free area x > 0.3)."""
  s = ['<mujoco><compiler angle="radian"/><option timestep="0.002" solver="CG" jacobian="sparse"/><worldbody>']
  nchain = nstar = 0
  for it in items:
    if it[0] == "chain":
      _chain70((-1.5, round(-1.8 + 0.25 * nchain, 6), 0.3), s)
      nchain += 1
    elif it[1] > 100:
      _star((1.0, 0.0, 0.5), it[1], s)
    else:
      _star((round(-1.7 + 0.4 * (nstar % 5), 6), round(-1.6 + 0.4 * (nstar // 5), 6), 0.5), it[1], s)
      nstar += 1
  s.append("</worldbody></mujoco>")
  return "".join(s)


# ---- column lengths -------------------------------------------------------------------------------------
COLUMN_K = (1, 3, 4, 5, 31, 32, 33, 64)


def columns_xml(solver):
  """Body b on a vertical slide carries COLUMN_K[b] condim-1 spheres; one more body (one sphere) stays up."""
  s = [f'<mujoco><option timestep="0.002" cone="pyramidal" solver="{solver}" jacobian="sparse"/><worldbody>'
       '<geom type="plane" size="5 5 .1" contype="1" conaffinity="0" condim="1"/>']
  for b, k in enumerate(COLUMN_K + (1,)):
    s.append(f'<body pos="{round(-1.6 + 0.4 * b, 6)!r} 0 0"><joint type="slide" axis="0 0 1" {JNT}/>')
    # a body's k equal rows add k D to its entry of H, and D is its mass times imp / (1 - imp): with the default impedance
    # the bodies' entries of M^-1 H spread over 1 : 64 and CG (fp64 too) runs out of iterations.  k imp / (1 - imp) = 64
    # makes them equal
    imp = round(64.0 / (64.0 + k), 6)
    for i in range(k):
      s.append(f'<geom type="sphere" size="0.02" pos="{round(0.045 * (i % 8), 6)!r} {round(0.045 * (i // 8), 6)!r} 0.02" contype="0" conaffinity="1" condim="1" '
               f'priority="1" solimp="{imp!r} {imp!r} 0.001 0.5 2"/>')
    s.append("</body>")
  s.append("</worldbody></mujoco>")
  return "".join(s)


# ---- the kernel's rules, restated -----------------------------------------------------------------------
def tree_path(m, t):
  """The branch solve_trees / mul_m_trees take for tree t of the derived fields `m` (io.derive_model_fields plus
  dof_parentid): "chain", "small" or "general"."""
  a, e = int(m["tree_dofadr"][t]), int(m["tree_dofadr"][t + 1])
  if e - a <= CHAIN and all(int(m["dof_parentid"][k]) == k - 1 for k in range(a + 1, e)):
    return "chain"
  return "small" if e - a <= TREE else "general"


def tree_branched(m, t):
  a, e = int(m["tree_dofadr"][t]), int(m["tree_dofadr"][t + 1])
  return any(int(m["dof_parentid"][k]) != k - 1 for k in range(a + 1, e))


def big_bodies(m):
  """The bodies whose subtree com_pos sums block-wide (the world body included)."""
  end = np.asarray(m["body_subtree_end"])
  return [b for b in range(len(end)) if int(end[b]) - b > BIG]


def fields(mjm):
  """io.derive_model_fields and the host fields the rules read."""
  from mujoco_warp_amd import io

  f = io.derive_model_fields(mjm)
  f["dof_parentid"] = np.asarray(mjm.dof_parentid)
  f["counts"] = dict(ntree=int(f["ntree"]), nv=int(mjm.nv), nbody=int(mjm.nbody), njnt=int(mjm.njnt))
  return f


def tree_of_body(mjm, f):
  """Tree index per body (-1: the world body and bodies without dofs)."""
  starts = np.asarray(f["tree_dofadr"])
  out = np.full(mjm.nbody, -1)
  for b in range(1, mjm.nbody):
    root = int(mjm.body_rootid[b])
    if int(mjm.body_dofnum[root]):
      out[b] = int(np.searchsorted(starts, int(mjm.body_dofadr[root]), side="right")) - 1
  return out


# ---- the cases ------------------------------------------------------------------------------------------
def _seed(text):
  return sum((i + 1) * ord(c) for i, c in enumerate(text)) % (2 ** 31)


def _quat_y(a):
  return np.array([np.cos(a / 2), 0.0, np.sin(a / 2), 0.0])


def _quat_rand(rng, sd):
  v = rng.normal(0, sd, 3)
  a = np.linalg.norm(v)
  return np.concatenate(([np.cos(a / 2)], np.sin(a / 2) * v / max(a, 1e-12)))


# per case id: the first k at which the states seeded _seed(id) + 13 k leave the fp32 oracle within half of every bar
# (tests/test_sparse_cases.py asserts it); 0 where not listed
SEED_SHIFT = {"ladder-1025-njmax1040-CG": 1, "contact-nv255-CG-implicitfast": 1, "contact-nv256-Newton-implicitfast": 1}


class Case:
  """kind: zoo / big / ladder / columns / contact.  Three worlds with different seeded states and a fourth that repeats
  world 0."""

  def __init__(self, id, kind, solver="CG", integrator="Euler", npad=0, items=(), target=0, njmax=64, expect=()):
    self.id, self.kind, self.solver, self.integrator, self.npad, self.items = id, kind, solver, integrator, npad, tuple(items)
    self.target, self.njmax, self.expect = target, njmax, tuple(expect)
    self.nworld = 4
    self.nconmax = 8
    self.seed = _seed(id) + 13 * SEED_SHIFT.get(id, 0)

  def xml(self):
    if self.kind in ("zoo", "contact"):
      return zoo_xml(self.npad, self.kind == "contact", self.solver, self.integrator)
    if self.kind == "big":
      return big_xml(self.items)
    if self.kind == "ladder":
      return sc.ladder_xml(LADDER_FEET, LADDER_HINGE, self.solver, jacobian="sparse", armature=LADDER_ARMATURE, dz=LADDER_DZ)
    return columns_xml(self.solver)

  def model(self):
    from mujoco_warp_amd import mjcf

    return mjcf.load_model_from_string(self.xml())

  def _world(self, mjm, rng):
    qpos, qvel = np.array(mjm.qpos0, np.float64), rng.normal(0, 0.3, mjm.nv)
    if self.kind == "ladder":
      return sc.ladder_state(mjm, self.target, rng, self.njmax, dz=LADDER_DZ)
    if self.kind == "columns":
      qpos[:] = -PEN
      qpos[-1] = UP
      return qpos, qvel
    contact = self.kind == "contact"
    sd = 0.1 if self.kind == "big" else 0.3
    npadj = mjm.njnt - self.npad
    for j in range(mjm.njnt):
      a, t, b = int(mjm.jnt_qposadr[j]), int(mjm.jnt_type[j]), int(mjm.jnt_bodyid[j])
      root = int(mjm.body_parentid[b]) == 0
      if self.kind != "big" and j >= npadj:  # a pad: every fifth lowered
        qpos[a] = -PEN if (j - npadj) % 5 == 0 else UP
      elif t == 3:
        qpos[a] = (0.02 + rng.uniform(0, 0.01) if root else rng.uniform(0.001, 0.004)) if contact else rng.normal(0, sd)
      elif t == 2:
        qpos[a] = rng.normal(0, 0.02)
      elif t == 1:
        qpos[a:a + 4] = _quat_y(0.02 + rng.uniform(0, 0.01)) if contact else _quat_rand(rng, sd)
      else:
        qpos[a + 3:a + 7] = _quat_y(0.02 + rng.uniform(0, 0.01)) if contact else _quat_rand(rng, sd)
        if not contact:
          qpos[a:a + 3] += rng.normal(0, 0.02, 3)
    return qpos, qvel

  def states(self, mjm):
    rng = np.random.default_rng(self.seed)
    ws = [self._world(mjm, rng) for _ in range(3)]
    ws.append(ws[0])
    return np.array([q for q, _ in ws]), np.array([v for _, v in ws]), np.zeros((4, mjm.nu))

  def oracle(self, mjm, states=None, real_bits=64):
    from tests.common import oracle_from_state

    states = self.states(mjm) if states is None else states
    return oracle_from_state(mjm, *states, njmax=self.njmax, nconmax=self.nconmax, real_bits=real_bits)[1]


# the ladder as tests/solver_cases.py builds it (armature 0.01, feet 7 cm deep, nv = 200, 1000 rows) has a cost near 1e5, whose
# fp32 rounding exceeds the CG stop threshold tolerance * meaninertia * nv: the fp32 oracle stops early and its 3-step qpos
# misses the bar by itself.  Feet 7 mm deep and hinges of armature 0.1 bring its error to 1e-6 .. 4e-6.
LADDER_ARMATURE, LADDER_DZ = "0.1", 0.002
LADDER_FEET, LADDER_HINGE = 64, 8  # nv = 200: up to 1024 contact rows, one equality, two frictionloss rows, limits
LADDER_TARGETS = (255, 256, 257, 1023, 1024, 1025)
PAD_COUNTS = {"ntree": (255, 256, 257, 513), "nv": (255, 256, 257), "nbody": (255, 256, 257), "njnt": (255, 256, 257)}
ZOO_BASE = dict(ntree=len(ZOO), nv=ZOO_NV, nbody=ZOO_NBODY + 1, njnt=ZOO_NBODY)


def _cases():
  out = [Case("zoo", "zoo", njmax=8)]
  pads = sorted({c - ZOO_BASE[k] for k, cs in PAD_COUNTS.items() for c in cs})
  for n in pads:
    hit = [f"{k}={ZOO_BASE[k] + n}" for k, cs in PAD_COUNTS.items() if ZOO_BASE[k] + n in cs]
    c = Case(f"pads-{n}", "zoo", npad=n, njmax=(n + 4) // 5 + 8, expect=hit)
    c.nconmax = c.njmax
    out.append(c)
  star = lambda L: ("star", L)  # noqa: E731
  big = [("nbig1", [star(63)]), ("star64-65", [star(63), star(64)]),
         ("nbig15", [("chain",)] * 2 + [star(64)] * 2), ("nbig16", [("chain",)] * 2 + [star(64)] * 3), ("nbig17", [("chain",)] * 2 + [star(64)] * 4),
         ("chains6", [("chain",)] * 6), ("stars16-900", [star(64)] * 16 + [star(900)]), ("900-stars16", [star(900)] + [star(64)] * 16)]
  for tag, items in big:
    out.append(Case(f"big-{tag}", "big", items=items, njmax=8))
  for solver in ("CG", "Newton"):
    for t in LADDER_TARGETS:
      for njmax in (1040, t):
        c = Case(f"ladder-{t}-njmax{njmax}-{solver}", "ladder", solver=solver, target=t, njmax=njmax)
        c.nconmax = 4 * LADDER_FEET + 8
        out.append(c)
    c = Case(f"columns-{solver}", "columns", solver=solver, njmax=sum(COLUMN_K) + 8)
    c.nconmax = c.njmax
    out.append(c)
    for integ in ("Euler", "implicitfast"):
      for nv in (255, 256, 257):
        n = nv - ZOO_NV
        c = Case(f"contact-nv{nv}-{solver}-{integ}", "contact", solver=solver, integrator=integ, npad=n, njmax=ZOO_NBODY + (n + 4) // 5 + 8)
        c.nconmax = c.njmax
        out.append(c)
  ids = [c.id for c in out]
  assert len(set(ids)) == len(ids)
  return out


CASES = _cases()


# ---- views ----------------------------------------------------------------------------------------------
def _solver_world(M, J, d):
  return dict(M=M, J=J, **d)


def oracle_run(case, mjm, states, real_bits):
  """The oracle's view of a case: every stage, the solve, one step and a 3-step rollout (`measure` reads it)."""
  nv, nj = mjm.nv, case.njmax
  od = case.oracle(mjm, states, real_bits)
  v = dict(fields={}, nworld=od.nworld)
  for st in STAGES:
    getattr(od, st)()
    for f in SMOOTH[st] + (("cfrc_int",) if st == "fwd_velocity" else ()):
      a = getattr(od, f, None)
      if a is not None and a.size:
        v["fields"][f] = np.array(a, np.float64)
  v["qM"] = [np.array(od.qM[w], np.float64).reshape(nv, nv) for w in range(od.nworld)]
  v["qacc_smooth"], v["qfrc_smooth"] = np.array(od.qacc_smooth, np.float64), np.array(od.qfrc_smooth, np.float64)
  od.solve()
  v["solver"] = sc.oracle_worlds(od, nv)
  v["qacc"], v["Ma"] = np.array(od.qacc, np.float64), np.array(od.efc_Ma, np.float64)
  v["niter"] = [int(x) for x in od.solver_niter[:, 0]]
  v["counts"] = {k: [int(x) for x in getattr(od, k)[:, 0]] for k in ("ne", "nf", "nl", "nefc")}
  v["od"] = od
  o2 = case.oracle(mjm, states, real_bits)
  o2.step()
  v["step1"] = (np.array(o2.qpos, np.float64), np.array(o2.qvel, np.float64))
  o2.step()
  o2.step()
  v["step3"] = (np.array(o2.qpos, np.float64), np.array(o2.qvel, np.float64))
  return v


def rebuild_LDL(mjm, f, qLD, t):
  """L' D L of tree t in fp64 from a sparse qLD (ancestor rows, diagonal last: L[k][j] for the ancestors j, D[k])."""
  a, e = int(f["tree_dofadr"][t]), int(f["tree_dofadr"][t + 1])
  n = e - a
  L, D = np.eye(n), np.zeros(n)
  for k in range(a, e):
    adr, nnz = int(mjm.M_rowadr[k]), int(mjm.M_rownnz[k])
    D[k - a] = qLD[adr + nnz - 1]
    for p in range(nnz - 1):
      L[k - a, int(mjm.M_colind[adr + p]) - a] = qLD[adr + p]
  return L.T @ np.diag(D) @ L


def _norm(got, want):
  """Worst world of max |got - want| / max |want| (tests/parity_models.err "norm")."""
  got, want = np.asarray(got, np.float64).reshape(len(want), -1), np.asarray(want, np.float64).reshape(len(want), -1)
  if want.size == 0:
    return 0.0
  return float((np.abs(got - want).max(axis=1) / (np.abs(want).max(axis=1) + 1e-30)).max())


def measure(case, mjm, f, view, ref):
  """{check: value} of `view` (a device or fp32-oracle run) against `ref` (the fp64 oracle run); BARS has the bars."""
  nv, nw = mjm.nv, ref["nworld"]
  out = {}
  for k, want in ref["fields"].items():
    if k in view["fields"]:
      out[k] = _norm(view["fields"][k], want)
  tb = tree_of_body(mjm, f)
  ntree = int(f["ntree"])
  starts = np.asarray(f["tree_dofadr"])
  for k, width in TREE_FIELDS.items():
    if k not in view["fields"] or k not in ref["fields"]:
      continue
    got, want = view["fields"][k].reshape(nw, mjm.nbody, width), ref["fields"][k].reshape(nw, mjm.nbody, width)
    worst = 0.0
    for t in range(ntree):
      sel = tb == t
      scale = np.abs(want[:, sel]).max(axis=(1, 2))
      e = np.abs(got[:, sel] - want[:, sel]).max(axis=(1, 2))
      ok = scale > 0
      if ok.any():
        worst = max(worst, float((e[ok] / scale[ok]).max()))
      if (~ok).any() and e[~ok].max() > 0:  # exactly zero in fp64: nothing to scale by
        worst = float(np.inf)
    out[k + "_tree"] = worst
  qM_t = ldl_t = bw_t = ma_t = 0.0
  out["qM"] = max(_norm(view["qM"][w][None], ref["qM"][w][None]) for w in range(nw))
  for w in range(nw):
    Mv, Mr = view["qM"][w], ref["qM"][w]
    for t in range(ntree):
      s = slice(int(starts[t]), int(starts[t + 1]))
      qM_t = max(qM_t, float(np.abs(Mv[s, s] - Mr[s, s]).max() / np.abs(Mr[s, s]).max()))
      if "qLD" in view:
        ldl_t = max(ldl_t, float(np.abs(rebuild_LDL(mjm, f, view["qLD"][w], t) - Mv[s, s]).max() / np.abs(Mv[s, s]).max()))
      x, b = view["qacc_smooth"][w, s], view["qfrc_smooth"][w, s]  # the run's own M and right-hand side: this is solve_trees
      bw_t = max(bw_t, float(np.abs(Mv[s, s] @ x - b).max() / max((np.abs(Mv[s, s]) @ np.abs(x)).max(), np.abs(b).max(), 1e-300)))
      q = view["qacc"][w, s]
      ma_t = max(ma_t, float(np.abs(view["Ma"][w, s] - Mv[s, s] @ q).max() / max((np.abs(Mv[s, s]) @ np.abs(q)).max(), 1e-300)))
  out["qM_tree"], out["solve_trees_backward"], out["mul_m_trees"] = qM_t, bw_t, ma_t
  if "qLD" in view:
    out["factor_trees"] = ldl_t
  inv = sc.solver_invariants(view["solver"], case.njmax, sentinel=view.get("sentinel", False))
  for k in sc.VALUES:
    out[k] = inv[k]
  out["qfrc_abs"], out["state_bad"], out["boundary_share"], out["nonfinite"], out["touched"] = (inv[k] for k in ("qfrc_abs", "state_bad", "boundary_share", "nonfinite", "touched"))
  od = ref["od"]
  truncated = [w for w in range(nw) if int(od.nefc[w, 0]) > case.njmax]
  out["cost_excess"] = sc.cost_excess(od, view["qacc"], skip=truncated)
  out["qacc"] = _norm(view["qacc"], ref["qacc"])
  out["counts_equal"] = view["counts"] == ref["counts"]
  out["niter_zero"] = sum(1 for w in range(nw) if ref["counts"]["nefc"][w] > 0 and view["niter"][w] <= 0)
  for tag in ("step1", "step3"):
    out[tag + "_qpos"], out[tag + "_qvel"] = _norm(view[tag][0], ref[tag][0]), _norm(view[tag][1], ref[tag][1])
  return out


def bars(values):
  """The bar of every measured value (the project's own: SMOOTH_TOL, solver_cases.TOL / COST_TOL / QPOS_TOL / QVEL_TOL)."""
  out = {}
  for k in values:
    if k in sc.VALUES:
      out[k] = sc.TOL
    elif k == "cost_excess":
      out[k] = sc.COST_TOL
    elif k == "qacc":
      out[k] = QACC_TOL
    elif k.endswith("_qpos"):
      out[k] = sc.QPOS_TOL
    elif k.endswith("_qvel"):
      out[k] = sc.QVEL_TOL
    elif k == "boundary_share":
      out[k] = sc.BOUNDARY_CAP
    elif k in ("qfrc_abs", "state_bad", "nonfinite", "touched", "niter_zero"):
      out[k] = 0
    elif k != "counts_equal":
      out[k] = SMOOTH_TOL
  return out


def failures(values, scale=1.0):
  """(check, value, bar) of every value over scale * its bar (the counting checks are never scaled)."""
  bad = []
  for k, b in bars(values).items():
    lim = b if (b == 0 or k == "boundary_share") else scale * b
    if not values[k] <= lim:
      bad.append((k, values[k], lim))
  if not values["counts_equal"]:
    bad.append(("counts", False, True))
  return bad


# ---- the device side ------------------------------------------------------------------------------------
COMPARED = ("xpos", "xquat", "xipos", "subtree_com", "cinert", "cdof", "crb", "cvel", "cdof_dot", "qfrc_bias", "qfrc_passive", "qfrc_smooth", "qacc_smooth",
            "qM", "qLD", "qacc", "qfrc_constraint", "qpos", "qvel")


def _bits(t):
  import torch

  return t.view(torch.int32) if t.dtype == torch.float32 else t


def _bitwise(d, tag, store):
  """World 3 against world 0 now, and the whole array against the earlier run's under `tag`."""
  import torch

  bad = []
  for k in COMPARED:
    t = getattr(d, k, None)
    if t is None or t.numel() == 0:
      continue
    b = _bits(t)
    if not torch.equal(b[3], b[0]):
      bad.append((tag, k, "world 3 differs from world 0"))
    key = (tag, k)
    if key in store:
      if not torch.equal(store[key], b):
        bad.append((tag, k, "second run differs"))
    else:
      store[key] = b.clone()
  return bad


def device_run(case, mjm, f, states, store, trace=False):
  """The device's view of a case (as oracle_run), plus qLD, the bitwise findings and the traced step's kernel names."""
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd.forward import StepTracer
  from tests.cloth_common import dense_qM
  from tests.common import dense_efc_J, gpu_from_state, np_

  nv, nw = mjm.nv, 4
  fresh = lambda: gpu_from_state(mjm, *states, njmax=case.njmax, nconmax=case.nconmax)  # noqa: E731
  m, d = fresh()
  assert m.is_sparse
  d.efc.force.fill_(float("nan"))
  v = dict(fields={}, nworld=nw, sentinel=True, bitwise=[])
  for st in STAGES:
    getattr(mjw, st)(m, d)
    for k in SMOOTH[st] + (("cfrc_int",) if st == "fwd_velocity" else ()):
      g = getattr(d, k, None)
      if g is not None and g.numel():
        v["fields"][k] = np_(g).reshape(nw, -1)
  v["qM"] = [dense_qM(mjm, np_(d.qM[w])) for w in range(nw)]
  v["qLD"] = [np_(d.qLD[w]) for w in range(nw)]
  v["qacc_smooth"], v["qfrc_smooth"] = np_(d.qacc_smooth), np_(d.qfrc_smooth)
  mjw.solve(m, d)
  torch.cuda.synchronize()
  v["bitwise"] += _bitwise(d, "forward", store)
  worlds = []
  for w in range(nw):
    n = min(int(d.nefc[w]), d.njmax)
    J = np.zeros((d.njmax, nv))
    J[:n] = dense_efc_J(m, d, w)
    worlds.append(dict(M=v["qM"][w], J=J, D=np_(d.efc.D[w, :d.njmax]), aref=np_(d.efc.aref[w]), fl=np_(d.efc.frictionloss[w]), ne=int(d.ne[w]), nf=int(d.nf[w]),
                       nefc=int(d.nefc[w]), qacc=np_(d.qacc[w]), qfrc_constraint=np_(d.qfrc_constraint[w]), Ma=np_(d.efc.Ma[w]), force=np_(d.efc.force[w]),
                       state=d.efc.state[w, :d.njmax].cpu().numpy()))
  v["solver"] = worlds
  v["qacc"], v["Ma"] = np_(d.qacc), np_(d.efc.Ma)
  v["niter"] = [int(x) for x in d.solver_niter.cpu().ravel()]
  v["counts"] = {k: [int(x) for x in getattr(d, k).cpu().ravel()] for k in ("ne", "nf", "nl", "nefc")}
  m2, d2 = fresh()
  if trace:
    tracer = StepTracer()
    tracer.step(m2, d2)
    torch.cuda.synchronize()
    v["kernels"] = [k for k, _ in tracer.durations()[0] if not k.startswith("mjw::reset_counters")]
  else:
    mjw.step(m2, d2)
  v["step1"] = (np_(d2.qpos), np_(d2.qvel))
  mjw.step(m2, d2)
  mjw.step(m2, d2)
  torch.cuda.synchronize()
  v["step3"] = (np_(d2.qpos), np_(d2.qvel))
  v["bitwise"] += _bitwise(d2, "step3", store)
  return v


SP_KERNELS = ("mjw::sp::forward_kernel<1024>", "mjw::sp::forward_kernel<2048>", "mjw::sp::euler_kernel")


def check_kernels(names):
  for k in SP_KERNELS:
    assert k in names, (k, names)
  assert len(sc.solve_kernels(names)) == 1 and sc.solve_kernels(names)[0] == "mjw::sp::solve_kernel<1>", names
  assert not [n for n in names if n.startswith(("mjw::step_kernel", "mjw::mjw_kernel", "mjw::dense_kernel"))], names


def describe(case, mjm, f):
  """The counts and the path of every tree in tree order, runs of equal trees as [dofs, path, count], for the report."""
  starts = np.asarray(f["tree_dofadr"])
  trees = []
  for t in range(int(f["ntree"])):
    key = [int(starts[t + 1] - starts[t]), tree_path(f, t)]
    if trees and trees[-1][:2] == key:
      trees[-1][2] += 1
    else:
      trees.append(key + [1])
  return dict(counts=f["counts"], nbig=len(big_bodies(f)), njmax=case.njmax, trees=trees)


def run_case(case):
  """The case on the device, twice from fresh Data, measured against the fp64 oracle; the fp32 oracle's values go next to
  the device's.  Returns the report entry; `failures` lists what did not hold (none expected)."""
  mjm = case.model()
  f = fields(mjm)
  states = case.states(mjm)
  ref = oracle_run(case, mjm, states, 64)
  v32 = oracle_run(case, mjm, states, 32)
  store = {}
  dev = device_run(case, mjm, f, states, store, trace=True)
  again = device_run(case, mjm, f, states, store)
  values = measure(case, mjm, f, dev, ref)
  fp32 = measure(case, mjm, f, v32, ref)
  res = dict(id=case.id, **describe(case, mjm, f), nefc=dev["counts"]["nefc"], kernels=dev["kernels"],
             niter=dict(device=dev["niter"], fp32_oracle=v32["niter"], fp64_oracle=ref["niter"]))
  bad = [list(x) for x in failures(values)]
  try:
    check_kernels(dev["kernels"])
  except AssertionError as e:
    bad.append(["kernels", str(e)[:1000]])
  bad += [list(x) for x in dev["bitwise"] + again["bitwise"]]
  b = bars(values)
  res["values"] = {k: dict(device=values[k], bar=b.get(k), fp32_oracle=fp32.get(k)) for k in values}
  res["failures"] = bad
  return res
