"""The yardstick of the finite-difference linearisation (transition_fd): a numpy restatement of MuJoCo's mjd_stepFD
semantics, written from their description, not from the device code.

A state is a dict of 1-D arrays: qpos (nq), qvel (nv), act (na), ctrl (nu), and after a step sensordata.  `perturb`
and `difference` run in float64 on whatever they are given (float32 inputs included).  The tangent-space order of inputs
and outputs is [dq (nv), dv (nv), dact (na)], ndx = 2 nv + na; the K = ndx + nu columns are those, then ctrl.

  perturb(mjm, state, k, sign, eps)   the state with column k nudged by sign * eps (ctrl: a plain add; whether the
                                      nudge is made at all is `ctrl_nudges`)
  difference(mjm, y1, y2, h)          (y2 - y1) / h in the tangent space: ndx entries, then sensordata's if present
  ctrl_nudges / column_plan           MuJoCo's ctrl range rule and what a column then is (centred, one-sided, zero)
  pass_layout / slot_map              the slot bookkeeping: slot c of world w is scratch world c * nworld + w
  transition(mjm, stepfn, x, ...)     the whole linearisation around one state over any batched step function
"""

import numpy as np

# free box, ball-joint child, hinge, slide; a ctrl-limited motor and a position actuator with filter dynamics (the
# <position> shortcut has no dyntype: written out as <general>); jointpos, framepos
# and gyro sensors; one mocap body; one joint equality, inactive unless a test switches it on (so that eq_active has a
# row to copy); contacts off.  nq 13, nv 11, na 1, nu 2, nsensordata 7: ndx 23, K 25
FD_SMALL = """<mujoco><option timestep="0.005"/>
<default><geom contype="0" conaffinity="0"/></default>
<worldbody>
<body name="target" mocap="true" pos=".5 0 1"><geom type="sphere" size=".02"/></body>
<body name="box" pos="0 0 1"><freejoint/><geom type="box" size=".1 .08 .06"/>
  <body name="arm" pos="0 0 .15"><joint name="ball" type="ball" damping=".05"/><geom type="capsule" size=".03" fromto="0 0 0 .05 0 .2"/>
    <site name="tip" pos=".05 0 .2"/></body></body>
<body name="pend" pos="1 0 1"><joint name="hinge" type="hinge" axis="0 1 0" damping=".1"/><geom type="capsule" size=".03" fromto="0 0 0 .3 0 0"/>
  <body name="slider" pos=".3 0 0"><joint name="slide" type="slide" axis="1 0 0" stiffness="5"/><geom type="sphere" size=".05"/></body></body>
</worldbody>
<actuator>
<motor joint="hinge" ctrllimited="true" ctrlrange="-1 1"/>
<general joint="slide" dyntype="filter" dynprm=".05" gainprm="20" biastype="affine" biasprm="0 -20 0"/>
</actuator>
<equality><joint joint1="slide" active="false"/></equality>
<sensor><jointpos joint="hinge"/><framepos objtype="site" objname="tip"/><gyro site="tip"/></sensor>
</mujoco>"""
FD_SMALL_CTRL0 = (0.0, 1.0, -1.0)  # the motor's ctrl per world: the centred, backward-only and forward-only branches

# 1-dof slide: mass 2, stiffness 3, damping 0.7, motor gear 5, timestep 0.01, no gravity, Euler: a linear system
SLIDE_XML = """<mujoco><option timestep="0.01" gravity="0 0 0" integrator="Euler"{jacobian}/>
<worldbody><body><joint name="s" type="slide" axis="1 0 0" stiffness="3" damping="0.7"/>
<geom type="sphere" size=".1" mass="2" contype="0" conaffinity="0"/></body></worldbody>
<actuator><motor joint="s" gear="5"/></actuator></mujoco>"""


def slide_closed_form(m=2.0, k=3.0, b=0.7, g=5.0, h=0.01):
  """A, B of the slide model's Euler step with implicit damping: (m + h b) a = -k q - b v + g u, v' = v + h a, q' = q + h v'."""
  s = h / (m + h * b)
  return np.array([[1 - h * s * k, h * (1 - s * b)], [-s * k, 1 - s * b]]), np.array([[h * s * g], [s * g]])


FREE, BALL, SLIDE, HINGE = 0, 1, 2, 3
CLAMPCTRL = 256  # DisableBit


def sizes(mjm):
  nv, na, nu = int(mjm.nv), int(mjm.na), int(mjm.nu)
  return dict(nq=int(mjm.nq), nv=nv, na=na, nu=nu, ndx=2 * nv + na, ncol=2 * nv + na + nu, nsensordata=int(mjm.nsensordata))


def quat_mul(a, b):
  aw, ax, ay, az = a
  bw, bx, by, bz = b
  return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                   aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], dtype=np.float64)


def quat_exp(v):
  """exp(v) = (cos(|v| / 2), sin(|v| / 2) v / |v|)."""
  v = np.asarray(v, dtype=np.float64)
  n = np.linalg.norm(v)
  if n == 0.0:
    return np.array([1.0, 0, 0, 0])
  return np.concatenate([[np.cos(n / 2)], np.sin(n / 2) * v / n])


def quat_log(q):
  """angle * axis with angle = 2 atan2(|q_xyz|, q_w) wrapped into (-pi, pi]."""
  q = np.asarray(q, dtype=np.float64)
  n = np.linalg.norm(q[1:])
  if n == 0.0:
    return np.zeros(3)
  angle = 2.0 * np.arctan2(n, q[0])
  if angle > np.pi:
    angle -= 2.0 * np.pi
  return q[1:] / n * angle


def dof_target(mjm, v):
  """(is quaternion, qpos address, local axis) of dof v."""
  j = int(mjm.dof_jntid[v])
  t, qa, off = int(mjm.jnt_type[j]), int(mjm.jnt_qposadr[j]), v - int(mjm.jnt_dofadr[j])
  if t == FREE:
    return (False, qa + off, 0) if off < 3 else (True, qa + 3, off - 3)
  if t == BALL:
    return True, qa, off
  return False, qa, 0


def perturb(mjm, state, k, sign, eps):
  s = sizes(mjm)
  out = {n: np.array(state[n], dtype=np.float64) for n in ("qpos", "qvel", "act", "ctrl")}
  nv, na = s["nv"], s["na"]
  step = float(sign) * float(eps)
  if k < nv:
    isq, adr, axis = dof_target(mjm, k)
    if not isq:
      out["qpos"][adr] += step
    else:
      e = np.zeros(3)
      e[axis] = step
      q = quat_mul(out["qpos"][adr:adr + 4], quat_exp(e))
      out["qpos"][adr:adr + 4] = q / np.linalg.norm(q)
  elif k < 2 * nv:
    out["qvel"][k - nv] += step
  elif k < 2 * nv + na:
    out["act"][k - 2 * nv] += step
  else:
    out["ctrl"][k - 2 * nv - na] += step
  return out


def difference(mjm, y1, y2, h):
  s = sizes(mjm)
  nv = s["nv"]
  q1, q2 = np.asarray(y1["qpos"], dtype=np.float64), np.asarray(y2["qpos"], dtype=np.float64)
  dq = np.zeros(nv)
  for v in range(nv):
    isq, adr, axis = dof_target(mjm, v)
    if not isq:
      dq[v] = (q2[adr] - q1[adr]) / h
    elif axis == 0:
      conj = q1[adr:adr + 4] * np.array([1.0, -1, -1, -1])
      dq[v:v + 3] = quat_log(quat_mul(conj, q2[adr:adr + 4])) / h
  parts = [dq] + [(np.asarray(y2[n], dtype=np.float64) - np.asarray(y1[n], dtype=np.float64)) / h for n in ("qvel", "act")]
  if "sensordata" in y1 and "sensordata" in y2:
    parts.append((np.asarray(y2["sensordata"], dtype=np.float64) - np.asarray(y1["sensordata"], dtype=np.float64)) / h)
  return np.concatenate(parts)


def ctrl_nudges(mjm, ctrl, i, eps, centered):
  """(plus, minus): which nudges of ctrl i MuJoCo makes.  The sums are float32: the rule is stated on the stored
  values, and ctrl + eps is what the slot would hold."""
  plus, minus = True, bool(centered)
  if bool(mjm.actuator_ctrllimited[i]) and not (int(mjm.opt.disableflags) & CLAMPCTRL):
    lo, hi = (np.float32(x) for x in np.asarray(mjm.actuator_ctrlrange).reshape(-1, 2)[i])
    c, e = np.float32(ctrl[i]), np.float32(eps)
    inside = lambda x: bool(lo <= x <= hi)  # noqa: E731
    plus = inside(c) and inside(np.float32(c + e))
    minus = (bool(centered) or not plus) and inside(c) and inside(np.float32(c - e))
  return plus, minus


def column_plan(plus, minus):
  """(from, to, steps of eps between them) with '+', '-', '0' naming the perturbed and nominal results; None: zero."""
  if plus and minus:
    return "-", "+", 2
  if plus:
    return "0", "+", 1
  if minus:
    return "-", "0", 1
  return None


def pass_layout(ncol, nworld, centered, max_worlds=None):
  """(ncp columns per pass, ncol_pass slots per world, npass)."""
  per = 2 if centered else 1
  ncp = ncol if max_worlds is None else min(ncol, (max_worlds // nworld - 1) // per)
  return ncp, 1 + per * ncp, -(-ncol // ncp)


def slot_map(ncol, ncp, centered, pass_index):
  """(ncol_pass, 2): column and sign of every slot; (-1, 0): nominal (slot 0 and the last pass's spare slots)."""
  col0 = pass_index * ncp
  ncols = min(ncp, ncol - col0)
  out = np.full((1 + (2 if centered else 1) * ncp, 2), (-1, 0), dtype=np.int32)
  for j in range(ncols):
    out[1 + j] = (col0 + j, 1)
    if centered:
      out[1 + ncp + j] = (col0 + j, -1)
  return out


def slot_state(mjm, state, col, sign, eps, centered):
  """What the slot of (col, sign) holds: the nudged state, or the nominal one where the ctrl rule refuses the nudge
  (a forward context's one slot of a ctrl column takes the - nudge when only that one is possible)."""
  s = sizes(mjm)
  nominal = {n: np.array(state[n], dtype=np.float64) for n in ("qpos", "qvel", "act", "ctrl")}
  if col < 0:
    return nominal
  if col >= s["ndx"]:
    plus, minus = ctrl_nudges(mjm, state["ctrl"], col - s["ndx"], eps, centered)
    if not centered and not plus and minus:
      sign = -1
    elif not (plus if sign > 0 else minus):
      return nominal
  return perturb(mjm, state, col, sign, eps)


def transition(mjm, stepfn, state, eps, centered=True):
  """A (ndx, ndx), B (ndx, nu), C (nsd, ndx), D (nsd, nu) around `state`.  stepfn(list of states) -> list of next
  states (dicts with qpos, qvel, act and sensordata), one call for all 1 + 2 K (1 + K) of them."""
  s = sizes(mjm)
  K, ndx, nu = s["ncol"], s["ndx"], s["nu"]
  smap = slot_map(K, K, centered, 0)
  nxt = stepfn([slot_state(mjm, state, int(c), int(sg), eps, centered) for c, sg in smap])
  M = np.zeros((ndx + s["nsensordata"], K))
  for k in range(K):
    plan = ("-", "+", 2) if centered else ("0", "+", 1)
    if k >= ndx:
      plan = column_plan(*ctrl_nudges(mjm, state["ctrl"], k - ndx, eps, centered))
      if plan is None:
        continue
    slot = {"0": 0, "+": 1 + k, "-": 1 + K + k if centered else 1 + k}
    M[:, k] = difference(mjm, nxt[slot[plan[0]]], nxt[slot[plan[1]]], plan[2] * eps)
  return M[:ndx, :ndx], M[:ndx, ndx:ndx + nu], M[ndx:, :ndx], M[ndx:, ndx:ndx + nu]


def oracle_stepfn(mjm, njmax=64, nconmax=64, base=None, nefc_out=None, nthread=1):
  """stepfn over the fp64 CPU oracle: all states in one batched oracle step.  `base`: extra oracle fields held fixed
  (e.g. qacc_warmstart), name -> 1-D array, read at every call (the caller may change it between calls).  `nefc_out`:
  a list that receives the constraint rows of the first state of every call."""
  from oracle import orc

  om = orc.OracleModel(mjm)

  def stepfn(states):
    od = orc.OracleData(om, len(states), njmax, nconmax)
    for n in ("qpos", "qvel", "act", "ctrl"):
      if getattr(od, n).shape[1]:
        getattr(od, n)[:] = np.stack([st[n] for st in states])
    for n, v in ({} if base is None else base).items():
      getattr(od, n)[:] = v
    od.step(nthread)
    if nefc_out is not None:
      nefc_out.append(int(od.nefc[0, 0]))
    return [dict(qpos=od.qpos[i].copy(), qvel=od.qvel[i].copy(), act=od.act[i].copy(), sensordata=od.sensordata[i].copy()) for i in range(len(states))]

  return stepfn
