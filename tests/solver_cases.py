"""Solver-output invariants on a row-count ladder: the fixture, the checker and the case list.

The constraint solve exists in five forms that `run()` / `dense_launch()` pick by nv, njmax, solver and
entry point (csrc/mjw_dense.hip, csrc/mjw_step.hip, csrc/mjw_sparse.hip): dense_kernel with the factor
bound NB = 16 / 28 / 32, the fused step_kernel (CG, 17 <= nv <= 28, lean model, explicit Euler), the
generic LDS solver (nv 33..64 or njmax > 64) and the sparse solve.  Inside them the row count chooses the
unrolled J'f width (8/9, 16/17 rows), the Newton Hessian's row pairs (odd nefc), the half a row lives in
(31/32/33), the rows dropped past njmax and the 64-row stride of the generic solver (63/64/65).

`ladder_xml` builds a small synthetic model whose nv is free and `ladder_state` a state with an exact
row count: feet of four stacked spheres over a plane (0..4 contacts each, 4 pyramidal rows per contact),
limited hinges in chains (one limit row each when outside the range), two frictionloss dofs and one joint
equality.  `solver_invariants` then checks, in fp64 numpy and from the arrays the solver itself consumed
(M, J, D, aref, frictionloss, ne, nf) and wrote (qacc, efc_force, efc_state, qfrc_constraint, efc_Ma):

  force      efc_force against the row law of jar = J qacc - aref (equality -D jar; friction +-fl outside
             +-fl / D; one-sided 0 for jar >= 0), as max |diff| / max (D s), s = |J| |qacc| + |aref|
  state      efc_state is the branch taken (0 satisfied, 1 quadratic, 2 linear-, 3 linear+)
  qfrc       qfrc_constraint against J' efc_force, as max |diff| / max (|J|' |f|)
  Ma         efc_Ma against M qacc, as max |diff| / max (|M| |qacc|)
  force_row  the force error of each row against that row's own D s, qfrc_dof the qfrc error of each dof
             against that dof's own (|J|' |f|): the world-wide maxima above hide a wrong entry of a row or dof
             far below the largest (a frictionloss row next to contact rows); rounding stays at 1e-7 of the
             row's / dof's own scale, so the same bar applies
             (a world without rows: qfrc_constraint is exactly zero, `qfrc_abs`)
  untouched  efc_force rows >= n = min(nefc, njmax) still hold the NaN sentinel, rows < n are finite

A row whose jar lies within BAND * s of a branch point may match either side (force and state); at most
BOUNDARY_CAP of a case's rows may be such rows.  `cost_excess` (fp64 primal cost from the oracle's rows,
tests/parity_models.efc_cost) and `niter_margin` (Newton iteration totals) need the oracle.

tests/test_solver_cases.py validates the fixture and the checker on the CPU oracle,
tests/test_gpu_solver_outputs.py runs CASES on the device, tools/solver_invariants.py writes the report.
"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

R, DZ = 0.05, 0.02  # sphere radius, z offset between the spheres of a foot
BAND = 1e-4  # a row within BAND * s of a branch point is a boundary row
BOUNDARY_CAP = 0.05
VALUES = ("force", "force_row", "qfrc", "qfrc_dof", "Ma")  # the invariants with a bar
TOL = 1e-5  # the floor of the force / qfrc / Ma bars (tests/test_gpu_parity_models.py SMOOTH_TOL)
TOL_CAP = 1e-4
COST_TOL = 1e-5  # relative cost excess over the fp64 oracle's optimum (the project's bar)
QPOS_TOL, QVEL_TOL = 1e-5, 5e-3  # one step against the fp64 oracle (test_solve_and_step)

LADDER = (3, 4, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65)


def ladder_xml(nfeet, nhinge, solver, bare=False, eulerdamp=True, jacobian="dense", armature="0.01", dz=DZ):
  """MJCF of the ladder model: nv = 3 nfeet + nhinge, no tendons / actuators / sensors / boxes; `armature` of the hinges,
  `dz` between the spheres of a foot."""
  flag = "" if eulerdamp else '<flag eulerdamp="disable"/>'
  s = [f'<mujoco><compiler angle="radian"/><option timestep="0.002" cone="pyramidal" solver="{solver}" jacobian="{jacobian}">{flag}</option>'
       '<worldbody><geom type="plane" size="20 20 .1"/>']
  for b in range(nfeet):
    s.append(f'<body pos="{b * 0.6} 0 0"><joint name="fx{b}" type="slide" axis="1 0 0"/><joint name="fy{b}" type="slide" axis="0 1 0"/>'
             f'<joint name="fz{b}" type="slide" axis="0 0 1"/>')
    for k in (3, 2, 1, 0):  # the lowest sphere last: a foot's last contact is its deepest, the one that carries the load
      s.append(f'<geom type="sphere" size="{R}" pos="{0.12 * (k % 2)} {0.12 * (k // 2)} {k * dz}" condim="3" mass="0.3"/>')
    s.append("</body>")
  h = chain = 0
  while h < nhinge:
    n = min(4, nhinge - h)
    s.append(f'<body pos="{chain * 0.5} 3 1">')
    for k in range(n):
      fl = ' frictionloss="0.3"' if (h < 2 and not bare) else ""
      if k:
        s.append('<body pos="0.2 0 0">')
      s.append(f'<joint name="h{h}" type="hinge" axis="0 1 0" limited="true" range="-0.5 0.5" armature="{armature}" damping="0.1"{fl}/>'
               '<geom type="capsule" size="0.02" fromto="0 0 0 0.2 0 0" contype="0" conaffinity="0"/>')
      h += 1
    s.append("</body>" * n)
    chain += 1
  s.append("</worldbody>")
  if not bare:
    s.append(f'<equality><joint joint1="h{nhinge - 1}" joint2="h{nhinge - 2}" polycoef="0 1 0 0 0"/></equality>')
  s.append("</mujoco>")
  return "".join(s)


def ladder_counts(mjm):
  """(nfeet, nhinge, ne, nf) of a ladder model."""
  nhinge = int((np.asarray(mjm.jnt_type) == 3).sum())
  return (mjm.nv - nhinge) // 3, nhinge, int(mjm.neq), int((np.asarray(mjm.dof_frictionloss) > 0).sum())


def ladder_state(mjm, target_nefc, rng, njmax=None, dz=DZ):
  """qpos, qvel with ne + nf + 4 contacts + limits = target_nefc rows: as many contacts as fit, limits make
  up the remainder.  The frictionloss hinges and the equality's second joint take a limit row only when no
  other hinge is left (the (4, 4) model).  qvel ~ N(0, 0.3), except that the foot whose contact owns the last
  row the solver keeps (row min(target_nefc, njmax) - 1) moves straight down: its four pyramid rows then all
  carry a force, so a kernel that drops the last row of a world (a row-count edge) changes its outputs.  Rows
  are ordered equality, friction, limits, contacts (feet in order), so any other last row carries one anyway."""
  nfeet, nhinge, ne, nf = ladder_counts(mjm)
  rest = target_nefc - ne - nf
  assert rest >= 0, (target_nefc, ne, nf)
  ncon = min(rest // 4, 4 * nfeet)
  nlim = rest - 4 * ncon
  qpos = np.zeros(mjm.nq)
  qpos[3 * nfeet:] = rng.uniform(-0.3, 0.3, nhinge)
  qpos[0:3 * nfeet:3] = rng.uniform(-0.05, 0.05, nfeet)
  qpos[1:3 * nfeet:3] = rng.uniform(-0.05, 0.05, nfeet)
  qpos[2:3 * nfeet:3] = 1.0  # feet in the air
  c = ncon
  for b in range(nfeet):
    k = min(4, c)
    c -= k
    if k:  # spheres 0 .. k-1 penetrate, the topmost of them by DZ / 2; sphere k clears the plane by DZ / 2
      qpos[3 * b + 2] = R - (k - 0.5) * dz
  if ne or nf:
    first = [h for h in range(nhinge) if h >= nf and h != nhinge - 2]
    last = [nhinge - 2] + list(range(nf))
  else:
    first, last = list(range(nhinge)), []
  cand = [first[i] for i in rng.permutation(len(first))] + last
  assert nlim <= len(cand), (target_nefc, nlim, len(cand))
  for h in cand[:nlim]:
    qpos[3 * nfeet + h] = rng.choice([-1.0, 1.0]) * rng.uniform(0.55, 0.7)
  qvel = rng.normal(0, 0.3, mjm.nv)
  last = min(target_nefc, target_nefc if njmax is None else njmax) - 1 - ne - nf - nlim
  if last >= 0:
    b = (last // 4) // 4  # feet fill up in order, four contacts each
    qvel[3 * b:3 * b + 3] = 0.0, 0.0, -abs(qvel[3 * b + 2])
  return qpos, qvel


# per case number: the first seed of 1000 + num + 13 k at which, on the fp64, fp32 and fp32-FMA oracle builds and
# for both solvers, no row of any world lies within 1e-3 s (ten times BAND) of a branch point and the last row
# the solver keeps carries a force in every world (tests/test_solver_cases.py asserts both)
SEEDS = {1: 1001, 2: 1041, 3: 1003, 4: 1004, 5: 1005, 6: 1006, 7: 1020, 8: 1008, 9: 1009, 10: 1010, 11: 1011, 12: 1012, 13: 1013}
# (case number, target) whose last row is force-free whatever the seed: in the (4, 4) model the only hinge left
# for a single limit row is the equality's first joint, and the equality pulls it back inside its range
LAST_ROW_FREE = {(1, 4)}


class Case:
  def __init__(self, num, nfeet, nhinge, njmax, solver, kernel, targets=LADDER, bare=False, eulerdamp=True, jacobian="dense"):
    self.num, self.nfeet, self.nhinge, self.njmax, self.solver, self.kernel = num, nfeet, nhinge, njmax, solver, kernel
    self.targets, self.bare, self.eulerdamp, self.jacobian = tuple(targets), bare, eulerdamp, jacobian
    self.nconmax = 32
    self.seed = SEEDS[num]
    self.id = f"{num:02d}-nv{3 * nfeet + nhinge}-njmax{njmax}-{solver}"

  def model(self):
    from mujoco_warp_amd import mjcf

    return mjcf.load_model_from_string(ladder_xml(self.nfeet, self.nhinge, self.solver, self.bare, self.eulerdamp, self.jacobian))

  def states(self, mjm):
    """(qpos, qvel, ctrl) of the case's worlds, one per ladder target."""
    rng = np.random.default_rng(self.seed)
    qs = [ladder_state(mjm, t, rng, self.njmax) for t in self.targets]
    return np.array([q for q, _ in qs]), np.array([v for _, v in qs]), np.zeros((len(qs), mjm.nu))

  def oracle(self, mjm, states, real_bits=64):
    from tests.common import oracle_from_state

    return oracle_from_state(mjm, *states, njmax=self.njmax, nconmax=self.nconmax, real_bits=real_bits)[1]


def _cases():
  out = []
  both = ("CG", "Newton")
  for s in both:
    out.append(Case(1, 4, 4, 64, s, "dense16"))
  out.append(Case(2, 4, 5, 64, "CG", "fused", eulerdamp=False))
  out.append(Case(3, 4, 5, 64, "Newton", "dense28"))
  out.append(Case(4, 4, 16, 64, "CG", "fused", targets=LADDER + (48,), eulerdamp=False))
  for s in both:
    out.append(Case(5, 4, 16, 64, s, "dense28"))
  for s in both:
    out.append(Case(6, 4, 17, 64, s, "dense32", eulerdamp=False))
  for s in both:
    out.append(Case(7, 4, 20, 64, s, "dense32"))
  for s in both:
    out.append(Case(8, 4, 21, 64, s, "generic"))
  for s in both:
    out.append(Case(9, 6, 10, 96, s, "generic", targets=(63, 64, 65, 95, 96, 97, 99)))
  for s in both:
    out.append(Case(10, 4, 16, 20, s, "dense28", targets=(3, 19, 20, 21, 33)))
  for s in both:
    out.append(Case(11, 4, 16, 64, s, "dense28", targets=(0, 1, 2, 3, 4, 5), bare=True))
  out.append(Case(12, 4, 21, 64, "CG", "generic", targets=(0, 1, 2, 3), bare=True))
  for s in both:
    out.append(Case(13, 4, 16, 64, s, "sparse", targets=(3, 16, 33, 64), jacobian="sparse"))
  return out


CASES = _cases()


# ---- the invariants -------------------------------------------------------------------------------------
def row_law(jar, D, fl, ne, nf):
  """(force, state, distance of jar to the row's nearest branch point) per row."""
  n = len(jar)
  f, st, dist = np.zeros(n), np.zeros(n, int), np.full(n, np.inf)
  for r in range(n):
    if r < ne:
      f[r], st[r] = -D[r] * jar[r], 1
    elif r < ne + nf:
      rf = fl[r] / D[r]
      dist[r] = min(abs(jar[r] - rf), abs(jar[r] + rf))
      if jar[r] <= -rf:
        f[r], st[r] = fl[r], 2
      elif jar[r] >= rf:
        f[r], st[r] = -fl[r], 3
      else:
        f[r], st[r] = -D[r] * jar[r], 1
    else:
      dist[r] = abs(jar[r])
      if jar[r] < 0:
        f[r], st[r] = -D[r] * jar[r], 1
  return f, st, dist


def _other_side(jar, D, fl, ne, nf, r):
  """(force, state) of boundary row r on the other side of its nearest branch point."""
  if r >= ne + nf:
    return (-D[r] * jar[r], 1) if jar[r] >= 0 else (0.0, 0)
  rf = fl[r] / D[r]
  if abs(jar[r] + rf) <= abs(jar[r] - rf):
    return (-D[r] * jar[r], 1) if jar[r] <= -rf else (fl[r], 2)
  return (-D[r] * jar[r], 1) if jar[r] >= rf else (-fl[r], 3)


def world_invariants(a, njmax, sentinel=False):
  """The invariants of one world from its arrays `a` (see oracle_world / device_world): M (nv, nv), J (n, nv),
  D, aref, fl (n), ne, nf, nefc, qacc, qfrc_constraint, Ma (nv), force, state (njmax: the whole row array)."""
  n = min(int(a["nefc"]), njmax)
  f64 = lambda x: np.asarray(x, np.float64)  # noqa: E731
  M, J, D, aref, fl, q = f64(a["M"]), f64(a["J"])[:n], f64(a["D"])[:n], f64(a["aref"])[:n], f64(a["fl"])[:n], f64(a["qacc"])
  force_all, state = f64(a["force"]), np.asarray(a["state"])[:n].astype(int)
  f = force_all[:n]
  out = dict(rows=n, boundary=0, state_bad=0, force=0.0, force_row=0.0, qfrc=0.0, qfrc_dof=0.0, qfrc_abs=0.0, Ma=0.0,
             nonfinite=int((~np.isfinite(f)).sum()), touched=0)
  if sentinel:
    out["touched"] = int((~np.isnan(force_all[n:])).sum())
  out["Ma"] = float(np.abs(f64(a["Ma"]) - M @ q).max() / max((np.abs(M) @ np.abs(q)).max(), 1e-300))
  if n == 0:
    out["qfrc_abs"] = float(np.abs(f64(a["qfrc_constraint"])).max())
    return out
  jar = J @ q - aref
  s = np.abs(J) @ np.abs(q) + np.abs(aref)
  want, st, dist = row_law(jar, D, fl, int(a["ne"]), int(a["nf"]))
  near = dist < BAND * s
  out["boundary"] = int(near.sum())
  df = np.abs(np.where(np.isfinite(f), f, np.inf) - want)
  bad = state != st
  for r in np.nonzero(near)[0]:  # either side of the branch point, the force on the side the state names
    wf, ws = _other_side(jar, D, fl, int(a["ne"]), int(a["nf"]), r)
    if state[r] == ws:
      df[r], bad[r] = abs(f[r] - wf), False
  out["force"] = float(df.max() / (D * s).max())
  out["force_row"] = float((df / np.maximum(D * s, 1e-300)).max())
  out["state_bad"] = int(bad.sum())
  fz = np.where(np.isfinite(f), f, 0.0)
  dq, sq = np.abs(f64(a["qfrc_constraint"]) - J.T @ fz), np.abs(J).T @ np.abs(fz)
  out["qfrc"] = float(dq.max() / max(sq.max(), 1e-300))
  out["qfrc_dof"] = float((dq / np.maximum(sq, 1e-300)).max())
  return out


def solver_invariants(worlds, njmax, sentinel=False):
  """Worst value of each invariant over the worlds of a case, the counts summed; `per_world` keeps the detail."""
  per = [world_invariants(a, njmax, sentinel) for a in worlds]
  out = {k: max(p[k] for p in per) for k in VALUES + ("qfrc_abs",)}
  out.update({k: sum(p[k] for p in per) for k in ("rows", "boundary", "state_bad", "nonfinite", "touched")})
  out["boundary_share"] = out["boundary"] / max(out["rows"], 1)
  out["per_world"] = per
  return out


def oracle_world(od, w, nv):
  """The arrays of world w of an oracle run (any real type)."""
  nj = od.njmax
  return dict(M=od.qM[w].reshape(nv, nv), J=od.efc_J[w].reshape(nj, nv), D=od.efc_D[w], aref=od.efc_aref[w], fl=od.efc_frictionloss[w],
              ne=od.ne[w, 0], nf=od.nf[w, 0], nefc=od.nefc[w, 0], qacc=od.qacc[w], qfrc_constraint=od.qfrc_constraint[w], Ma=od.efc_Ma[w],
              force=od.efc_force[w], state=od.efc_state[w])


def oracle_worlds(od, nv):
  return [oracle_world(od, w, nv) for w in range(od.nworld)]


def cost_excess(od, qacc, skip=()):
  """Worst (c(qacc) - c(oracle qacc)) / |c(oracle qacc)| over the worlds with rows: the fp64 primal cost from the
  fp64 oracle's own rows."""
  from tests.parity_models import efc_cost

  nv = od.qacc.shape[1]
  worst = -np.inf
  for w in range(od.nworld):
    n = min(int(od.nefc[w, 0]), od.njmax)
    if n == 0 or w in skip:
      continue
    args = (od.efc_J[w].reshape(od.njmax, nv)[:n], od.efc_D[w, :n], od.efc_aref[w, :n], od.efc_type[w, :n], od.qM[w].reshape(nv, nv),
            od.qacc_smooth[w])
    c_or = efc_cost(*args, od.qacc[w], fl=od.efc_frictionloss[w, :n])
    c = efc_cost(*args, np.asarray(qacc[w], np.float64), fl=od.efc_frictionloss[w, :n])
    worst = max(worst, (c - c_or) / abs(c_or))
  return float(worst) if np.isfinite(worst) else 0.0


def niter_margin(o32, o64):
  """(fp32 oracle total, fp64 oracle total, allowed excess over the fp32 total): one iteration per world or the
  two builds' own difference, whichever is larger (counts are discrete, the stop test sits at rounding level)."""
  t32, t64 = int(o32.solver_niter.sum()), int(o64.solver_niter.sum())
  return t32, t64, max(o32.nworld, abs(t32 - t64))


def bar(v32):
  """tests/test_gpu_parity_models.py fp32_bar: 1e-5 or twice the fp32 oracle's own residual, never above 1e-4."""
  b = max(TOL, 2.0 * v32)
  assert b <= TOL_CAP, v32
  return b


# ---- the device side ------------------------------------------------------------------------------------
def solve_kernels(names):
  """The kernels of a traced step that run the constraint solve."""
  out = []
  for n in names:
    m = re.match(r"mjw::(step_kernel|dense_kernel|mjw_kernel|sp::solve_kernel)<(\d+)", n)
    if not m:
      continue
    kind, k = m.group(1), int(m.group(2))
    if kind == "step_kernel" or (kind == "dense_kernel" and k & 2) or (kind == "mjw_kernel" and k & 16) or (kind == "sp::solve_kernel" and k):
      out.append(n)
  return out


def expected_kernels(case):
  """(solve kernel names allowed, the launch that must follow it or None, kernel-name prefixes that must not run)."""
  nt = "true" if case.solver == "Newton" else "false"
  if case.kernel == "fused":
    return ["mjw::step_kernel<79, false, 7, false, 28>"], None, ("mjw::dense_kernel", "mjw::mjw_kernel", "mjw::sp::")
  if case.kernel.startswith("dense"):
    nb = case.kernel[5:]
    if case.eulerdamp:  # implicit damping: factor + solve, then the Euler-only kernel
      return [f"mjw::dense_kernel<3, {nt}, false, {nb}>"], f"mjw::dense_kernel<4, {nt}, false, {nb}>", ("mjw::step_kernel", "mjw::sp::")
    return [f"mjw::dense_kernel<7, {nt}, false, {nb}>"], None, ("mjw::step_kernel", "mjw::sp::")
  if case.kernel == "generic":
    return ["mjw::mjw_kernel<63, false, false>"], None, ("mjw::step_kernel", "mjw::dense_kernel", "mjw::sp::")
  return ["mjw::sp::solve_kernel<1>", "mjw::sp::solve_kernel<2>"], "mjw::sp::euler_kernel", ("mjw::step_kernel", "mjw::dense_kernel", "mjw::mjw_kernel")


def check_kernels(case, names):
  allowed, follow, banned = expected_kernels(case)
  sk = solve_kernels(names)
  assert len(sk) == 1 and sk[0] in allowed, (case.id, names)
  if follow is not None:
    assert names[names.index(sk[0]) + 1:][:1] == [follow], (case.id, names)
  assert not [n for n in names if n.startswith(banned)], (case.id, names)


INPUTS = ("qM", "efc_J", "efc_D", "efc_aref", "efc_frictionloss", "qfrc_smooth", "qacc_smooth", "ne", "nf", "nefc")


def _field(d, name):
  return getattr(d.efc, name[4:]) if name.startswith("efc_") else getattr(d, name)


def _bits(t):
  import torch

  return t.view(torch.int32) if t.dtype == torch.float32 else t


def device_worlds(mjm, m, d, od, src):
  """Per-world arrays of the device: the solver's outputs from `d`, each input from src[name] (the stepped Data,
  or the twin's where the step did not leave the array)."""
  from tests.common import dense_efc_J, np_
  from tests.parity_models import dense_M

  out = []
  for w in range(d.nworld):
    n = min(int(d.nefc[w]), d.njmax)
    J = np.zeros((d.njmax, mjm.nv))
    J[:n] = dense_efc_J(m, src["efc_J"], w)
    out.append(dict(M=dense_M(mjm, src["qM"], od, w)[0], J=J, D=np_(src["efc_D"].efc.D[w, :d.njmax]), aref=np_(src["efc_aref"].efc.aref[w]),
                    fl=np_(src["efc_frictionloss"].efc.frictionloss[w]), ne=int(d.ne[w]), nf=int(d.nf[w]), nefc=int(d.nefc[w]),
                    qacc=np_(d.qacc[w]), qfrc_constraint=np_(d.qfrc_constraint[w]), Ma=np_(d.efc.Ma[w]), force=np_(d.efc.force[w]),
                    state=d.efc.state[w, :d.njmax].cpu().numpy()))
  return out


def run_case(case):
  """One traced step of the case on the device and everything the tests assert, as a dict (no assertion here
  besides the row counts, which the comparison needs)."""
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd.forward import StepTracer
  from tests.common import gpu_from_state, np_

  mjm = case.model()
  nv = mjm.nv
  states = case.states(mjm)
  nworld = len(case.targets)
  o64, o32 = case.oracle(mjm, states, 64), case.oracle(mjm, states, 32)
  o64.forward()
  o32.forward()
  ostep = case.oracle(mjm, states, 64)
  ostep.step()

  def fresh():
    m_, d_ = gpu_from_state(mjm, *states, njmax=case.njmax, nconmax=case.nconmax)
    d_.efc.force.fill_(float("nan"))
    return m_, d_

  m, d = fresh()
  tracer = StepTracer()
  tracer.step(m, d)
  m2, d2 = fresh()  # the twin: the same state through `forward`
  mjw.forward(m2, d2)
  if case.kernel == "fused":
    m3, d3 = fresh()
    for f in (mjw.fwd_position, mjw.fwd_velocity, mjw.fwd_actuation, mjw.fwd_acceleration, mjw.solve, mjw.euler):
      f(m3, d3)
  torch.cuda.synchronize()
  names = [k for k, _ in tracer.durations()[0] if not k.startswith("mjw::reset_counters")]
  res = dict(id=case.id, kernels=names, targets=list(case.targets), nefc=[int(x) for x in d.nefc.cpu()])
  counts = {k: [int(x) for x in getattr(d, k).cpu().ravel()] for k in ("nefc", "ne", "nf", "nl")}
  res["counts_equal"] = all(counts[k] == [int(x) for x in getattr(o64, k)[:, 0]] for k in counts)
  res["counts"] = counts
  # the twin is the stepped solve: bitwise the same qacc and efc_force (sentinel rows included)
  res["twin_bitwise"] = bool(torch.equal(_bits(d.qacc), _bits(d2.qacc)) and torch.equal(_bits(d.efc.force), _bits(d2.efc.force)))
  src, from_twin = {}, []
  for name in INPUTS:
    same = torch.equal(_bits(_field(d, name)), _bits(_field(d2, name)))
    src[name] = d if same else d2
    if not same:
      from_twin.append(name)
  if m.is_sparse:  # the sparse J goes with its index arrays
    src["efc_J"] = d if "efc_J" not in from_twin and all(torch.equal(getattr(d.efc, f), getattr(d2.efc, f)) for f in ("J_colind", "J_rownnz")) else d2
  res["from_twin"] = from_twin
  if case.kernel == "fused":
    res["staged_bitwise"] = {f: bool(torch.equal(_bits(_field(d, f)), _bits(_field(d3, f)))) for f in ("qacc", "efc_force", "efc_state", "qpos", "qvel")}
  dev = solver_invariants(device_worlds(mjm, m, d, o64, src), case.njmax, sentinel=True)
  ref = solver_invariants(oracle_worlds(o32, nv), case.njmax)
  res["device"] = {k: v for k, v in dev.items() if k != "per_world"}
  res["fp32"] = {k: ref[k] for k in VALUES + ("state_bad", "boundary_share")}
  res["worst_world"] = {k: int(np.argmax([p[k] for p in dev["per_world"]])) for k in VALUES}
  truncated = [w for w in range(nworld) if int(o64.nefc[w, 0]) > case.njmax] if m.is_sparse else ()
  res["cost_excess"] = cost_excess(o64, np_(d.qacc), skip=truncated)
  res["cost_excess_fp32"] = cost_excess(o64, o32.qacc, skip=truncated)
  t32, t64, margin = niter_margin(o32, o64)
  res["niter"] = dict(device=int(d.solver_niter.sum()), fp32=t32, fp64=t64, margin=margin,
                      per_world=[int(x) for x in d.solver_niter.cpu().ravel()], per_world_fp32=[int(x) for x in o32.solver_niter[:, 0]])
  # normwise per world, worst world (tests/parity_models.err "norm")
  res["step_qpos"] = float((np.abs(np_(d.qpos) - ostep.qpos).max(axis=1) / np.abs(ostep.qpos).max(axis=1)).max())
  res["step_qvel"] = float((np.abs(np_(d.qvel) - ostep.qvel).max(axis=1) / np.abs(ostep.qvel).max(axis=1)).max())
  return res


def failures(case, res):
  """Every assertion of the GPU test as (name, detail) pairs; empty when the case passes."""
  bad = []
  dev, ref = res["device"], res["fp32"]
  try:
    check_kernels(case, res["kernels"])
  except AssertionError as e:
    bad.append(("kernels", str(e)))
  if not res["counts_equal"]:
    bad.append(("counts", res["counts"]))
  if not res["twin_bitwise"]:
    bad.append(("twin", "qacc / efc_force of the forward twin differ from the step's"))
  if case.kernel == "fused" and not all(res["staged_bitwise"].values()):
    bad.append(("staged", res["staged_bitwise"]))
  for k in VALUES:
    if not dev[k] <= bar(ref[k]):
      bad.append((k, (dev[k], bar(ref[k]), "world", res["worst_world"][k])))
  if dev["qfrc_abs"] != 0.0:
    bad.append(("qfrc", ("qfrc_constraint of a world without rows", dev["qfrc_abs"])))
  if dev["state_bad"]:
    bad.append(("state", dev["state_bad"]))
  if dev["boundary_share"] > BOUNDARY_CAP:
    bad.append(("boundary", dev["boundary_share"]))
  if dev["nonfinite"] or dev["touched"]:
    bad.append(("untouched", dict(nonfinite=dev["nonfinite"], touched=dev["touched"])))
  if not res["cost_excess"] <= COST_TOL:
    bad.append(("cost", res["cost_excess"]))
  ni = res["niter"]
  if case.solver == "Newton" and ni["device"] > ni["fp32"] + ni["margin"]:
    bad.append(("niter", ni))
  if not res["step_qpos"] <= QPOS_TOL:
    bad.append(("step_qpos", res["step_qpos"]))
  if not res["step_qvel"] <= QVEL_TOL:
    bad.append(("step_qvel", res["step_qvel"]))
  return bad
