"""Inverse dynamics (mirror mujoco_warp/_src/inverse.py).

`inverse(m, d)` computes the generalized force `d.qfrc_inverse` that produces the acceleration `d.qacc` at the
state `qpos`, `qvel`, `act` in `d`: the position and velocity stages through their usual entry points, then one
HIP launch (`mjw_inverse`: csrc/mjw_inverse.hip on the dense path, `sp::inverse_kernel` in csrc/mjw_sparse.hip
on the sparse path) that evaluates the constraint row law once at `qacc` and combines

  qfrc_inverse = qfrc_bias + M qacc - qfrc_passive - qfrc_constraint,

then the acceleration sensors.  `d.qacc` is an input and is left unchanged.
"""

from __future__ import annotations

import torch

from . import _lib
from .forward import _stream, fwd_position, fwd_velocity, sensor_acc, sensor_pos, sensor_vel
from .io import cdata, cmodel
from .stages import _per_world, deriv_smooth_vel, factor_m, solve_m
from .support import mul_m
from .types import Data, DisableBit, EnableBit, IntegratorType, Model


def _check_discrete(m: Model):
  if m.opt.integrator == IntegratorType.RK4:
    raise NotImplementedError("discrete inverse dynamics is not supported by RK4 integrator")
  if m.opt.integrator not in (IntegratorType.EULER, IntegratorType.IMPLICITFAST):
    raise NotImplementedError(f"integrator {m.opt.integrator} not implemented.")


def discrete_acc(m: Model, d: Data, qacc: torch.Tensor):
  """Continuous-time acceleration into `qacc` (nworld, nv) from the discrete-time one in `d.qacc`
  (inverse.py:70-113); `qacc` may be `d.qacc` itself.

  Euler with EULERDAMP disabled: a copy.  Euler: qacc = M^-1 (M + dt diag(dof_damping)) d.qacc.  implicitfast:
  qacc = M^-1 (M - dt qDeriv) d.qacc with the matrix of `deriv_smooth_vel`.  RK4 raises NotImplementedError
  before any launch.  The solve needs the factor of the current qM: `factor_m` refreshes `d.qLD` here, and with
  it rewrites `d.qfrc_smooth` and `d.qacc_smooth` (the acceleration-stage launch).  Not a hot path: torch ops."""
  _check_discrete(m)
  src = d.qacc
  if m.opt.integrator == IntegratorType.EULER and (m.opt.disableflags & DisableBit.EULERDAMP):
    if qacc is not src:
      qacc.copy_(src)
    return
  nw, nv = d.nworld, m.nv
  qfrc = torch.empty((nw, nv), dtype=src.dtype, device=src.device)
  if m.opt.integrator == IntegratorType.EULER:
    mul_m(m, d, qfrc, src)
    dt = _per_world(m.opt.timestep, nw, 1)
    qfrc += dt * _per_world(m.dof_damping, nw, nv) * src
  else:
    qderiv = torch.empty_like(d.qM)
    deriv_smooth_vel(m, d, qderiv)
    mul_m(m, d, qfrc, src, M=qderiv)
  factor_m(m, d)
  solve_m(m, d, qacc, qfrc)


def inv_constraint(m: Model, d: Data):
  """The inverse constraint solve and the combine, one launch (mjw_inverse): over the rows r < min(nefc, njmax)
  Jaref = J qacc - aref, efc.force / efc.state from the row law, qfrc_constraint = J' efc.force, efc.Ma = M qacc,
  and qfrc_inverse = qfrc_bias + efc.Ma - qfrc_passive - qfrc_constraint.  Expects the position and velocity
  stages of the current state in `d`."""
  _lib.check(_lib.lib().mjw_inverse(cmodel(m), cdata(d), _stream(d)), "mjw_inverse")


def inverse(m: Model, d: Data):
  """Inverse dynamics (inverse.py:127-161): `d.qfrc_inverse` from `d.qpos`, `d.qvel`, `d.act`, `d.qacc` and
  `d.eq_active`; also writes efc.force, efc.state, qfrc_constraint, efc.Ma and the sensors.  `d.qacc` is left
  unchanged (bitwise).  With EnableBit.INVDISCRETE, `d.qacc` is taken as the discrete-time acceleration
  (qvel_next - qvel) / dt and converted first (`discrete_acc`, which also refreshes qLD / qfrc_smooth /
  qacc_smooth)."""
  invdiscrete = bool(m.opt.enableflags & EnableBit.INVDISCRETE)
  if invdiscrete:
    _check_discrete(m)  # before any launch
  fwd_position(m, d)
  sensor_pos(m, d)
  fwd_velocity(m, d)  # includes rne and the tendon bias (qfrc_bias)
  sensor_vel(m, d)
  if invdiscrete:
    qacc_discrete = d.qacc.clone()
    discrete_acc(m, d, d.qacc)
  inv_constraint(m, d)
  sensor_acc(m, d)
  if invdiscrete:
    d.qacc.copy_(qacc_discrete)
