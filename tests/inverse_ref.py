"""Inverse dynamics in fp64 numpy: the yardstick of tests/test_inverse.py and tests/test_gpu_inverse.py.

A restatement of the reference's inverse.py / solver.py init_context(grad=False) from the arrays of one world
(the same dict tests/solver_cases.world_invariants reads: M, J, D, aref, fl, ne, nf, nefc, qacc, plus qfrc_bias
and qfrc_passive):

  Jaref = J qacc - aref over the rows r < n = min(nefc, njmax)
  efc_force, efc_state   the row law: tests/solver_cases.row_law for equality / friction-loss / one-sided rows,
                         `cone_law` (solver.py:1886-1942) for the rows of an elliptic contact
  qfrc_constraint = J' efc_force,  Ma = M qacc
  qfrc_inverse = qfrc_bias + Ma - qfrc_passive - qfrc_constraint

and `discrete_acc` (inverse.py:70-113) for Euler and implicitfast.  tests/test_inverse.py pins it on the fp64
oracle's forward dynamics: at the oracle's qacc it must return qfrc_applied + qfrc_actuator.
"""
import numpy as np

from tests.solver_cases import BAND, row_law

SATISFIED, QUADRATIC, LINEARNEG, LINEARPOS, CONE = 0, 1, 2, 3, 4
ELLIPTIC = 7  # ConstraintType.CONTACT_ELLIPTIC
ZONES = ("top", "middle", "bottom")


def cone_law(jar, D, mu, fr, zone=None):
  """(force (dim,), state, zone) of one elliptic contact from its rows' Jaref and D, mu = friction[0] *
  impratio_invsqrt and the friction coefficients fr (solver.py:1886-1942): top zone N >= mu T (no force), bottom
  zone mu N + T <= 0 (every row quadratic), else the middle zone (the cone's surface).  `zone` forces a zone's
  formula (the other side of a boundary, for a contact that sits on one)."""
  dim = len(jar)
  u = np.array([jar[0] * mu] + [jar[j] * fr[j - 1] for j in range(1, dim)])
  N, T = u[0], float(np.sqrt((u[1:] ** 2).sum()))
  if zone is None:
    zone = "top" if (N >= mu * T or (T <= 0.0 and N >= 0.0)) else ("bottom" if (mu * N + T <= 0.0 or (T <= 0.0 and N < 0.0)) else "middle")
  if zone == "top":
    return np.zeros(dim), SATISFIED, "top"
  if zone == "bottom":
    return -D * jar, QUADRATIC, "bottom"
  dm = D[0] / (mu * mu * (1.0 + mu * mu))
  f0 = -dm * (N - mu * T) * mu
  f = np.empty(dim)
  f[0] = f0
  for j in range(1, dim):
    f[j] = -(f0 / T) * u[j] * fr[j - 1]
  return f, CONE, "middle"


def cones_of(etype, eid, con_adr0, con_dim, con_friction, impratio_invsqrt, n):
  """The elliptic contacts with a row below n, as (r0, dim, mu, fr, whole): from the rows' type / id and the
  contacts' first row, dim and friction.  whole = False when njmax cuts the contact's rows (it contributes nothing)."""
  out, seen = [], set()
  for r in range(n):
    if int(etype[r]) != ELLIPTIC or int(eid[r]) in seen:
      continue
    c = int(eid[r])
    seen.add(c)
    r0, dim = int(con_adr0[c]), int(con_dim[c])
    assert r0 == r, (r0, r)
    fr = np.asarray(con_friction[c], np.float64)
    out.append((r0, dim, float(fr[0]) * float(impratio_invsqrt), fr, r0 + dim <= n))
  return out


def cone_near(jar, s, mu, fr):
  """Whether the contact lies within BAND of a zone boundary (N = mu T or mu N + T = 0), on the scale of its
  rows' s = |J| |qacc| + |aref|."""
  dim = len(jar)
  N = jar[0] * mu
  T = float(np.sqrt(sum((jar[j] * fr[j - 1]) ** 2 for j in range(1, dim))))
  sN = s[0] * mu
  sT = float(np.sqrt(sum((s[j] * fr[j - 1]) ** 2 for j in range(1, dim))))
  return abs(N - mu * T) < BAND * (sN + mu * sT) or abs(mu * N + T) < BAND * (mu * sN + sT)


def inverse_world(a, njmax, cones=()):
  """The inverse dynamics of one world; `cones` from cones_of for elliptic models.  Returns a dict: n, jar, s,
  force, state (n rows each), dist (row_law's branch distance, inf on cone rows), zones (one per whole cone),
  qfrc_constraint, Ma, qfrc_inverse."""
  f64 = lambda x: np.asarray(x, np.float64)  # noqa: E731
  n = min(int(a["nefc"]), njmax)
  M, q = f64(a["M"]), f64(a["qacc"])
  nv = len(q)
  J, D, aref, fl = f64(a["J"])[:n].reshape(n, nv), f64(a["D"])[:n], f64(a["aref"])[:n], f64(a["fl"])[:n]
  jar = J @ q - aref
  s = np.abs(J) @ np.abs(q) + np.abs(aref)
  force, state, dist = row_law(jar, D, fl, int(a["ne"]), int(a["nf"]))
  zones = []
  for r0, dim, mu, fr, whole in cones:
    hi = min(r0 + dim, n)
    dist[r0:hi] = np.inf
    if not whole:
      force[r0:hi], state[r0:hi] = 0.0, SATISFIED
      continue
    force[r0:hi], st, zone = cone_law(jar[r0:hi], D[r0:hi], mu, fr)
    state[r0:hi] = st
    zones.append(zone)
  qc = J.T @ force
  Ma = M @ q
  out = dict(n=n, jar=jar, s=s, force=force, state=state, dist=dist, zones=zones, qfrc_constraint=qc, Ma=Ma)
  if "qfrc_bias" in a:
    out["qfrc_inverse"] = f64(a["qfrc_bias"]) + Ma - f64(a["qfrc_passive"]) - qc
  return out


def gpu_cases():
  """The ladder cases of tests/solver_cases.CASES the device test runs: the Newton variant where a case has
  one (1, 3, 5-11, 13), the CG-only cases 2, 4 and 12 as they are."""
  from tests.solver_cases import CASES

  cg_only = (2, 4, 12)
  return [c for c in CASES if (c.solver == "CG") == (c.num in cg_only)]


def perturb_qacc(qacc, seed):
  """qacc + N(0, 0.1 max(max |qacc|, 1)) per world, worlds in order from default_rng(seed), as float32: an
  acceleration away from the solver's, so that the result does not depend on its convergence."""
  rng = np.random.default_rng(seed)
  qacc = np.asarray(qacc, np.float64)
  out = np.empty(qacc.shape, np.float32)
  for w in range(qacc.shape[0]):
    sd = 0.1 * max(float(np.abs(qacc[w]).max()), 1.0)
    out[w] = (qacc[w] + rng.normal(0.0, sd, qacc.shape[1])).astype(np.float32)
  return out


def discrete_acc(M, qacc, dt, integrator, dof_damping=None, qDeriv=None, eulerdamp=True):
  """Continuous-time acceleration of one world from the discrete-time one (inverse.py:70-113): Euler
  M^-1 (M + dt diag(damping)) qacc (a copy without eulerdamp), implicitfast M^-1 (M - dt qDeriv) qacc."""
  M, qacc = np.asarray(M, np.float64), np.asarray(qacc, np.float64)
  if integrator == "Euler":
    if not eulerdamp:
      return qacc.copy()
    return np.linalg.solve(M, (M + dt * np.diag(np.asarray(dof_damping, np.float64))) @ qacc)
  if integrator == "implicitfast":
    return np.linalg.solve(M, (M - dt * np.asarray(qDeriv, np.float64)) @ qacc)
  raise NotImplementedError(integrator)
