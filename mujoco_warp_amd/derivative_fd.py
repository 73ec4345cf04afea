"""Finite-difference linearisation of `step` (MuJoCo's mjd_transitionFD; the reference has no counterpart).

`transition_fd(m, d, eps, centered, A, B, C, D, ctx=ctx)` gives, for every world of `d`, the matrices of
`x' ~ A dx + B du` and `sensordata ~ C dx + D du` around the world's state, in the tangent space
`dx = [dq (nv), dv (nv), dact (na)]`.  Every perturbed copy of a world is one more world of the context's scratch Data
(`ctx.data`, an ordinary Data): `fd_perturb` fills its slots (csrc/mjw_fd.hip, one wave per scratch world), one `step`
advances all of them, `fd_difference` transposes the differences of the stepped slots into A..D.  Slot `c` of world
`w` is scratch world `c * nworld + w`; slot 0 of every pass holds the nominal state.  `d` is only read, nothing is
allocated on the device after `make_fd_context`, and all launches go to the Data's stream.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .forward import _stream, step
from .io import _model_attr, cdata, cmodel, make_data
from .types import Data, Model


class FdContext:
  """What `make_fd_context` returns: the scratch Data and the slot bookkeeping of a linearisation.

  ndx = 2 nv + na, ncol = ndx + nu (the columns: dq, dv, dact, dctrl); ncp columns per pass, ncol_pass = 1 + 2 ncp
  (centred) or 1 + ncp (forward) slots per world, npass passes; data: the scratch Data of ncol_pass * nworld worlds."""

  def __init__(self):
    self.nworld = self.ndx = self.ncol = self.ncp = self.ncol_pass = self.npass = 0
    self.centered = True
    self.sizes = ()
    self.data: Data = None
    self._cfd = {}

  def pass_columns(self, pass_index: int):
    """(first column, number of columns) of a pass."""
    if not 0 <= int(pass_index) < self.npass:
      raise ValueError(f"pass_index {pass_index} outside 0 .. {self.npass - 1}")
    col0 = int(pass_index) * self.ncp
    return col0, min(self.ncp, self.ncol - col0)

  def slot_map(self, pass_index: int = 0) -> np.ndarray:
    """Host array (ncol_pass, 2) int32: the column and the sign (+1 / -1) of every slot of a pass; (-1, 0) for the
    nominal slot 0 and for the last pass's spare slots, which hold the nominal state too.  (A forward context's slot
    of a ctrl column whose + nudge the range rule refuses holds the - nudge: see transition_fd.)"""
    col0, ncols = self.pass_columns(pass_index)
    out = np.full((self.ncol_pass, 2), (-1, 0), dtype=np.int32)
    for j in range(ncols):
      out[1 + j] = (col0 + j, 1)
      if self.centered:
        out[1 + self.ncp + j] = (col0 + j, -1)
    return out


def _model_sizes(m: Model):
  return tuple(int(getattr(m, n)) for n in ("nq", "nv", "na", "nu", "nbody", "nmocap", "neq", "nsensordata"))


def make_fd_context(mjm, m: Model, nworld: int, centered: bool = True, nconmax=None, njmax=None, max_worlds=None, device=None) -> FdContext:
  """Allocates everything `transition_fd` needs for `nworld` worlds of model `m` (made from `mjm`).

  One pass holds all ncol = 2 nv + na + nu columns by default: the scratch Data has (1 + 2 ncol) nworld worlds centred,
  (1 + ncol) nworld forward.  `max_worlds` caps the scratch Data's worlds; `transition_fd` then loops over
  `ctx.npass` passes of `ctx.ncp` columns.  nconmax / njmax are per scratch world, as in make_data.  ValueError if a
  batched field of `m` has a batch size that does not divide nworld (slot c of world w must read the row world w
  reads: (c nworld + w) % nb == w % nb), or if max_worlds cannot hold the nominal slot and one column."""
  nworld = int(nworld)
  if nworld < 1:
    raise ValueError("make_fd_context: nworld must be >= 1")
  if m.nv == 0:
    raise NotImplementedError("make_fd_context: a model without dofs (nv == 0) has no state to linearise")
  for name, _ in _lib.MODEL_REAL_ARRAYS:
    grp, attr = _model_attr(name)
    t = getattr(getattr(m, grp), attr) if grp else getattr(m, attr)
    nb = int(t.shape[0]) if isinstance(t, torch.Tensor) and t.dim() > 0 else 1
    if nb > 1 and nworld % nb:
      raise ValueError(f"make_fd_context: model field {name} is batched over {nb} worlds, which does not divide nworld = {nworld}")
  ctx = FdContext()
  ctx.nworld, ctx.centered = nworld, bool(centered)
  ctx.sizes = _model_sizes(m)
  ctx.ndx = 2 * m.nv + m.na
  ctx.ncol = ctx.ndx + m.nu
  per = 2 if ctx.centered else 1
  ctx.ncp = ctx.ncol
  if max_worlds is not None:
    ctx.ncp = min(ctx.ncol, (int(max_worlds) // nworld - 1) // per)
    if ctx.ncp < 1:
      raise ValueError(f"make_fd_context: max_worlds = {max_worlds} cannot hold the nominal slot and one column of {nworld} worlds "
                       f"({(1 + per) * nworld} scratch worlds)")
  ctx.ncol_pass = 1 + per * ctx.ncp
  ctx.npass = -(-ctx.ncol // ctx.ncp)
  ctx.data = make_data(mjm, nworld=ctx.ncol_pass * nworld, nconmax=nconmax, njmax=njmax, device=device if device is not None else m.device, m=m)
  return ctx


def _check_ctx(who: str, m: Model, d: Data, ctx: FdContext, centered=None):
  if m.nv == 0:
    raise NotImplementedError(f"{who}: a model without dofs (nv == 0) has no state to linearise")
  if not isinstance(ctx, FdContext):
    raise ValueError(f"{who}: ctx must come from make_fd_context")
  if ctx.nworld != d.nworld:
    raise ValueError(f"{who}: ctx was made for nworld = {ctx.nworld}, the Data has {d.nworld}")
  if centered is not None and bool(centered) != ctx.centered:
    raise ValueError(f"{who}: ctx was made with centered = {ctx.centered}")
  if ctx.sizes != _model_sizes(m):
    raise ValueError(f"{who}: ctx was made for another model size")


def _check_eps(who: str, eps) -> float:
  eps = float(eps)
  if not (eps > 0.0 and np.isfinite(eps)):
    raise ValueError(f"{who}: eps must be positive and finite (there is no default: MuJoCo's 1e-6 is an fp64 value)")
  return eps


def _check_out(who: str, m: Model, d: Data, ctx: FdContext, A, B, C, D):
  if (C is None) != (D is None):
    raise ValueError(f"{who}: C and D are both given or both None")
  dev = d.qpos.device
  _lib.check_tensor(who, "A", A, torch.float32, dev, (d.nworld, ctx.ndx, ctx.ndx))
  _lib.check_tensor(who, "B", B, torch.float32, dev, (d.nworld, ctx.ndx, m.nu))
  if C is not None:
    _lib.check_tensor(who, "C", C, torch.float32, dev, (d.nworld, m.nsensordata, ctx.ndx))
    _lib.check_tensor(who, "D", D, torch.float32, dev, (d.nworld, m.nsensordata, m.nu))


def _cfd(d: Data, ctx: FdContext, pass_index: int, A=None, B=None, C=None, D=None) -> _lib.CFd:
  """The C view of a pass (cached on the context per pass and nominal Data; the outputs are set on every call)."""
  key = (int(pass_index), id(d))
  tensors = [getattr(d, n) for n in _lib.FD_STATE_FIELDS] + [getattr(ctx.data, n) for n in _lib.FD_STATE_FIELDS] + [ctx.data.sensordata]
  cache = ctx._cfd.get(key)
  if cache is None or not all(a is b for a, b in zip(cache[1], tensors)):
    c = _lib.CFd()
    c.nworld, c.ncol, c.ncol_pass, c.centered = ctx.nworld, ctx.ncol, ctx.ncol_pass, int(ctx.centered)
    c.col0, c.ncols = ctx.pass_columns(pass_index)
    for n, t in zip(["n_" + n for n in _lib.FD_STATE_FIELDS] + ["s_" + n for n in _lib.FD_STATE_FIELDS] + ["s_sensordata"], tensors):
      if not t.is_contiguous():
        raise TypeError(f"fd field {n} must be contiguous")
      setattr(c, n, t.data_ptr() if t.numel() else None)
    ctx._cfd = {k: v for k, v in ctx._cfd.items() if k[1] == id(d)}  # one nominal Data at a time
    ctx._cfd[key] = cache = (c, tensors)
  c = cache[0]
  for n, t in (("A", A), ("B", B), ("C", C), ("D", D)):
    setattr(c, n, t.data_ptr() if t is not None and t.numel() else None)
    setattr(c, "ld" + n.lower(), int(t.shape[-1]) if t is not None else 0)
  return c


def fd_perturb(m: Model, d: Data, ctx: FdContext, eps: float, pass_index: int = 0):
  """Fills the slots of pass `pass_index` in ctx.data from the worlds of `d` (mjw_fd_perturb): every slot receives,
  bitwise, the world's time, qpos, qvel, act, ctrl, qacc_warmstart, qfrc_applied, xfrc_applied, eq_active, mocap_pos
  and mocap_quat, and on top of that the nudge of its column (`ctx.slot_map`).  Reads `d`, allocates nothing."""
  _check_ctx("fd_perturb", m, d, ctx)
  eps = _check_eps("fd_perturb", eps)
  c = _cfd(d, ctx, pass_index)
  _lib.check(_lib.lib().mjw_fd_perturb(cmodel(m), cdata(d), c, eps, _stream(d)), "mjw_fd_perturb")


def fd_difference(m: Model, d: Data, ctx: FdContext, eps: float, A, B, C=None, D=None, pass_index: int = 0):
  """Writes the columns of pass `pass_index` of A, B (C, D) from the stepped slots in ctx.data (mjw_fd_difference);
  the other columns are left alone.  Reads `d` (the ctrl range rule), allocates nothing."""
  _check_ctx("fd_difference", m, d, ctx)
  eps = _check_eps("fd_difference", eps)
  _check_out("fd_difference", m, d, ctx, A, B, C, D)
  c = _cfd(d, ctx, pass_index, A, B, C, D)
  _lib.check(_lib.lib().mjw_fd_difference(cmodel(m), cdata(d), c, eps, _stream(d)), "mjw_fd_difference")


def transition_fd(m: Model, d: Data, eps: float, centered: bool, A, B, C=None, D=None, *, ctx: FdContext):
  """Finite-differenced discrete-time transition matrices of `step` at the state of every world of `d`
  (MuJoCo's mjd_transitionFD): x' ~ A dx + B du, sensordata ~ C dx + D du.

  A (nworld, ndx, ndx), B (nworld, ndx, nu), C (nworld, nsensordata, ndx), D (nworld, nsensordata, nu): float32,
  contiguous, caller-allocated, on the Data's device; rows are outputs, columns inputs, both ordered
  [dq (nv), dv (nv), dact (na)] with ndx = 2 nv + na.  C and D are both given or both None; with nu == 0, B and D
  have a zero-sized last dimension and are not touched.  Positions are perturbed and differenced in the tangent
  space (mj_integratePos / mj_differentiatePos).  ctrl columns follow MuJoCo's range rule for ctrl-limited
  actuators: per world the column is centred, forward, backward or zero.  Sensors are `sensordata` as `step` leaves
  it.  `ctx` comes from `make_fd_context(mjm, m, d.nworld, centered)`; per pass this is `fd_perturb`, `step` on
  ctx.data, `fd_difference`.  `d` is only read; nothing is allocated on the device; every launch goes to the Data's
  stream, so the call can be captured in a graph.

  `eps` is required: MuJoCo's 1e-6 is an fp64 value; in float32 every entry carries a rounding error of about
  2^-24 |y| / eps.  Recommended: eps = 2^-7 (about 0.008).  That is a measurement on one model, not a guarantee
  (tools/fd_bench.py): the humanoid, 64 worlds, centred, against the same finite difference over the
  fp64 oracle at eps = 1e-6.  Before ground contact the 99th percentile of the error of A and B is smallest at 2^-7
  to 2^-8 (4e-4; truncation takes over above 2^-6, rounding below 2^-9).  Settled in contact the error does not depend
  on eps between 2^-4 and 2^-9 (median 1e-2 in A, where the fp64 reference disagrees with itself at eps = 1e-5 by
  3e-3: a nudge switches contact rows) and grows below 2^-10."""
  _check_ctx("transition_fd", m, d, ctx, centered)
  eps = _check_eps("transition_fd", eps)
  _check_out("transition_fd", m, d, ctx, A, B, C, D)
  for p in range(ctx.npass):
    fd_perturb(m, d, ctx, eps, p)
    step(m, ctx.data)
    fd_difference(m, d, ctx, eps, A, B, C, D, p)
