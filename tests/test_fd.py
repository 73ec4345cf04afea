"""Finite-difference linearisation, host side: the public surface (make_fd_context, transition_fd, fd_perturb,
fd_difference, the mjw_fd_t mirror and the two C entries' argument checks) and the yardstick tests/fd_ref.py pinned on
a closed form over the fp64 CPU oracle.  The kernels are tested in tests/test_gpu_fd.py.
"""

import ctypes

import numpy as np
import pytest

from tests import fd_ref as fr

NO_DOF_XML = '<mujoco><worldbody><geom type="plane" size="1 1 .1"/></worldbody></mujoco>'


def _small(nworld=3, **kw):
  import mujoco_warp_amd as mjw

  mjm = mjw.load_model_from_string(fr.FD_SMALL)
  m = mjw.put_model(mjm, device="cpu")
  d = mjw.make_data(mjm, nworld=nworld, device="cpu", m=m)
  ctx = mjw.make_fd_context(mjm, m, nworld, device="cpu", **kw)
  return mjw, mjm, m, d, ctx


def _outputs(nworld, ndx, nu, ns):
  import torch

  return [torch.zeros(s) for s in ((nworld, ndx, ndx), (nworld, ndx, nu), (nworld, ns, ndx), (nworld, ns, nu))]


# ---- 1: names, argument validation, context sizes ------------------------------------------------------------
def test_names_validation_and_context_sizes():
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import _lib

  for name in ("make_fd_context", "transition_fd", "fd_perturb", "fd_difference"):
    assert callable(getattr(mjw, name)), name
  assert {"mjw_fd_perturb", "mjw_fd_difference", "mjw_sizeof_fd"} <= set(_lib.ENTRY_POINTS) and "mjw_fd_t" in _lib._H

  mjw, mjm, m, d, ctx = _small()
  assert (mjm.nq, mjm.nv, mjm.na, mjm.nu, mjm.nsensordata, mjm.nmocap) == (13, 11, 1, 2, 7, 1)
  assert (ctx.ncol, ctx.ncol_pass, ctx.npass, ctx.centered) == (25, 51, 1, True)
  assert isinstance(ctx.data, mjw.Data) and ctx.data.nworld == 51 * 3 and tuple(ctx.data.qpos.shape) == (153, 13)
  fwd = mjw.make_fd_context(mjm, m, 3, centered=False, device="cpu")
  assert (fwd.ncol, fwd.ncol_pass, fwd.npass, fwd.centered) == (25, 26, 1, False)
  for centered, npass in ((True, 13), (False, 7)):  # 2 (4) columns per pass: a remainder pass of 1 column
    part = mjw.make_fd_context(mjm, m, 3, centered=centered, max_worlds=3 * 5, device="cpu")
    assert part.ncol_pass == 5 and part.data.nworld == 15 and part.npass == npass
    cols = [part.pass_columns(p) for p in range(part.npass)]
    assert cols[0][0] == 0 and cols[-1] == (24, 1) and sum(n for _, n in cols) == 25
    assert all(a[0] + a[1] == b[0] for a, b in zip(cols, cols[1:]))
    for p in range(part.npass):  # the context's slot map is the yardstick's
      assert np.array_equal(part.slot_map(p), fr.slot_map(25, part.ncp, centered, p))
    assert part.slot_map(npass - 1)[2:].tolist() == ([[-1, 0], [24, -1], [-1, 0]] if centered else [[-1, 0]] * 3)
  assert fr.pass_layout(25, 3, True, 15) == (2, 5, 13) and fr.pass_layout(25, 3, False) == (25, 26, 1)
  assert mjw.make_fd_context(mjm, m, 3, max_worlds=3 * 4, device="cpu").ncol_pass == 3  # an even count is rounded down
  assert np.array_equal(ctx.slot_map(0), fr.slot_map(25, 25, True, 0)) and ctx.slot_map(0)[[0, 1, 26]].tolist() == [[-1, 0], [0, 1], [0, -1]]

  # refusals
  with pytest.raises(ValueError, match="max_worlds"):
    mjw.make_fd_context(mjm, m, 3, max_worlds=3 * 2, device="cpu")
  mjm0 = mjw.load_model_from_string(NO_DOF_XML)
  m0 = mjw.put_model(mjm0, device="cpu")
  with pytest.raises(NotImplementedError, match="nv == 0"):
    mjw.make_fd_context(mjm0, m0, 2, device="cpu")
  A, B, C, D = _outputs(3, 23, 2, 7)
  eps = 2.0**-7
  with pytest.raises(NotImplementedError, match="nv == 0"):
    mjw.transition_fd(m0, mjw.make_data(mjm0, nworld=3, device="cpu", m=m0), eps, True, A, B, ctx=ctx)
  with pytest.raises(ValueError, match="nworld"):
    mjw.transition_fd(m, mjw.make_data(mjm, nworld=2, device="cpu", m=m), eps, True, A, B, ctx=ctx)
  with pytest.raises(ValueError, match="centered"):
    mjw.transition_fd(m, d, eps, False, A, B, ctx=ctx)
  mjm1 = mjw.load_model_from_string(fr.SLIDE_XML.format(jacobian=""))
  m1 = mjw.put_model(mjm1, device="cpu")
  with pytest.raises(ValueError, match="model size"):
    mjw.transition_fd(m1, mjw.make_data(mjm1, nworld=3, device="cpu", m=m1), eps, True, A, B, ctx=ctx)
  with pytest.raises(ValueError, match="ctx"):
    mjw.transition_fd(m, d, eps, True, A, B, ctx=None)
  for bad_eps in (0.0, -1.0, float("nan")):
    with pytest.raises(ValueError, match="eps"):
      mjw.transition_fd(m, d, bad_eps, True, A, B, ctx=ctx)
  with pytest.raises(TypeError):
    mjw.transition_fd(m, d, True, A, B, ctx=ctx)  # eps has no default
  with pytest.raises(ValueError, match="C and D"):
    mjw.transition_fd(m, d, eps, True, A, B, C, None, ctx=ctx)
  bad = dict(A=torch.zeros(3, 23, 22), B=torch.zeros(3, 23, 2, dtype=torch.float64), C=torch.zeros(3, 23, 7).transpose(1, 2), D=torch.zeros(2, 7, 2))
  for name, t in bad.items():
    args = dict(A=A, B=B, C=C, D=D)
    args[name] = t
    with pytest.raises(ValueError, match=f"{name} must be"):
      mjw.transition_fd(m, d, eps, True, args["A"], args["B"], args["C"], args["D"], ctx=ctx)
    with pytest.raises(ValueError, match=f"{name} must be"):
      mjw.fd_difference(m, d, ctx, eps, args["A"], args["B"], args["C"], args["D"])
  with pytest.raises(ValueError, match="pass_index"):
    mjw.fd_perturb(m, d, ctx, eps, pass_index=1)
  # valid arguments reach the launch, which a host Data refuses like every other entry
  with pytest.raises(RuntimeError, match="ROCm device only"):
    mjw.transition_fd(m, d, eps, True, A, B, C, D, ctx=ctx)


def test_batched_model_fields_must_divide_nworld():
  import torch

  import mujoco_warp_amd as mjw

  mjm = mjw.load_model_from_string(fr.FD_SMALL)
  m = mjw.put_model(mjm, device="cpu")
  m.dof_damping = m.dof_damping.reshape(1, -1).repeat(2, 1).contiguous()
  assert mjw.make_fd_context(mjm, m, 4, device="cpu").data.nworld == 4 * 51
  with pytest.raises(ValueError, match="dof_damping"):
    mjw.make_fd_context(mjm, m, 3, device="cpu")
  assert isinstance(m.dof_damping, torch.Tensor)


def test_struct_mirror_and_abi():
  from mujoco_warp_amd import _lib

  assert ctypes.sizeof(_lib.CFd) == 6 * 4 + (2 * 11 + 5) * 8 + 4 * 8
  L = _lib.lib()
  assert L.mjw_sizeof_fd() == ctypes.sizeof(_lib.CFd)
  assert _lib.ABI_VERSION == 36 and L.mjw_abi_version() == 36


def test_c_entries_check_their_arguments_without_a_launch():
  import torch

  from mujoco_warp_amd import _lib
  from mujoco_warp_amd.derivative_fd import _cfd
  from mujoco_warp_amd.io import cdata, cmodel

  mjw, mjm, m, d, ctx = _small()
  L = _lib.lib()
  A, B, C, D = _outputs(3, 23, 2, 7)
  good = _cfd(d, ctx, 0, A, B, C, D)
  eps = ctypes.c_float(2.0**-7)

  def variant(**kw):
    c = _lib.CFd()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(good), ctypes.sizeof(good))
    for k, v in kw.items():
      setattr(c, k, v)
    return c

  for fn in (L.mjw_fd_perturb, L.mjw_fd_difference):
    assert fn(None, cdata(d), good, eps, None) == -1 and b"null" in L.mjw_last_error()
    assert fn(cmodel(m), None, good, eps, None) == -1
    assert fn(cmodel(m), cdata(d), None, eps, None) == -1
    assert fn(cmodel(m), _lib.CData(), good, eps, None) == 0  # nworld = 0: nothing to do
    assert fn(cmodel(m), cdata(d), good, ctypes.c_float(0.0), None) == -4 and b"eps" in L.mjw_last_error()
    for kw, word in ((dict(nworld=2), b"nworld"), (dict(ncol=24), b"ncol"), (dict(ncol_pass=50), b"ncol_pass"), (dict(ncol_pass=1), b"ncol_pass"),
                     (dict(col0=-1), b"column range"), (dict(ncols=0), b"column range"), (dict(ncols=26), b"column range"),
                     (dict(col0=1), b"column range"), (dict(n_qpos=ctx.data.qpos.data_ptr()), b"nominal")):
      assert fn(cmodel(m), cdata(d), variant(**kw), eps, None) == -4, kw
      assert word in L.mjw_last_error(), (kw, L.mjw_last_error())
    assert fn(cmodel(m), cdata(d), variant(s_mocap_quat=None), eps, None) == -1 and b"null" in L.mjw_last_error()
  assert L.mjw_fd_difference(cmodel(m), cdata(d), variant(A=None), eps, None) == -1
  assert L.mjw_fd_difference(cmodel(m), cdata(d), variant(D=None), eps, None) == -1
  assert L.mjw_fd_difference(cmodel(m), cdata(d), variant(lda=22), eps, None) == -4 and b"leading" in L.mjw_last_error()
  mjm0 = mjw.load_model_from_string(NO_DOF_XML)
  m0 = mjw.put_model(mjm0, device="cpu")
  d0 = mjw.make_data(mjm0, nworld=3, device="cpu", m=m0)
  assert L.mjw_fd_perturb(cmodel(m0), cdata(d0), good, eps, None) == -4 and b"nv == 0" in L.mjw_last_error()
  assert isinstance(A, torch.Tensor)


# ---- the yardstick on its own ---------------------------------------------------------------------------------
def _random_state(mjm, rng):
  qpos = rng.normal(size=mjm.nq)
  for adr in (3, 7):
    qpos[adr:adr + 4] /= np.linalg.norm(qpos[adr:adr + 4])
  return dict(qpos=qpos, qvel=rng.normal(size=mjm.nv), act=rng.normal(size=mjm.na), ctrl=rng.uniform(-0.5, 0.5, mjm.nu))


def test_reference_difference_inverts_perturb():
  """difference(x, x + eps e_k) / eps = e_k for every state column, quaternion ones included, and the centred pair gives
  the same; the quaternion nudge is a local-frame rotation (conj(q) q' = exp(eps e)) and the log wraps into (-pi, pi]."""
  import mujoco_warp_amd as mjw

  mjm = mjw.load_model_from_string(fr.FD_SMALL)
  rng = np.random.default_rng(0)
  x = _random_state(mjm, rng)
  eps = 2.0**-7
  for k in range(23):
    e = np.zeros(23)
    e[k] = 1.0
    p, n = fr.perturb(mjm, x, k, +1, eps), fr.perturb(mjm, x, k, -1, eps)
    assert np.allclose(fr.difference(mjm, x, p, eps), e, atol=1e-12), k
    assert np.allclose(fr.difference(mjm, n, p, 2 * eps), e, atol=1e-12), k
    assert np.array_equal(p["ctrl"], x["ctrl"])
  q = x["qpos"][3:7]
  p = fr.perturb(mjm, x, 4, +1, eps)["qpos"][3:7]  # free joint, local y
  assert np.allclose(fr.quat_mul(q * [1, -1, -1, -1], p), [np.cos(eps / 2), 0, np.sin(eps / 2), 0], atol=1e-15)
  assert abs(np.linalg.norm(p) - 1) < 1e-15
  assert np.allclose(fr.perturb(mjm, x, 24, -1, eps)["ctrl"], x["ctrl"] - [0, eps])
  assert np.allclose(fr.quat_log(fr.quat_exp([0, 0, 3.0])), [0, 0, 3.0]) and np.allclose(fr.quat_log(-fr.quat_exp([0, 0, 3.0])), [0, 0, 3.0])
  assert np.allclose(fr.quat_log(fr.quat_exp([0, 0, 4.0])), [0, 0, 4.0 - 2 * np.pi])  # past pi: the short way round
  assert np.allclose(fr.quat_log([0, 1.0, 0, 0]), [np.pi, 0, 0])


def test_reference_ctrl_rule():
  import mujoco_warp_amd as mjw

  mjm = mjw.load_model_from_string(fr.FD_SMALL)
  eps = 2.0**-7
  want = {0.0: {True: (True, True), False: (True, False)}, 1.0: {True: (False, True), False: (False, True)},
          -1.0: {True: (True, False), False: (True, False)}, 2.0: {True: (False, False), False: (False, False)}}
  for c, by_mode in want.items():
    for centered, pm in by_mode.items():
      assert fr.ctrl_nudges(mjm, [c, 0.0], 0, eps, centered) == pm, (c, centered)
      assert fr.ctrl_nudges(mjm, [c, 9.0], 1, eps, centered) == (True, centered)  # not ctrl-limited
  assert fr.ctrl_nudges(mjm, [1.0 - eps, 0.0], 0, eps, True) == (True, True)  # the bounds belong to the range
  assert [fr.column_plan(*pm) for pm in ((True, True), (True, False), (False, True), (False, False))] == [("-", "+", 2), ("0", "+", 1), ("-", "0", 1), None]
  mjm.opt.disableflags |= fr.CLAMPCTRL
  assert fr.ctrl_nudges(mjm, [1.0, 0.0], 0, eps, True) == (True, True)
  # a forward context's slot takes the - nudge when only that is possible; a refused nudge leaves the nominal state
  mjm.opt.disableflags &= ~fr.CLAMPCTRL
  x = dict(qpos=np.zeros(13), qvel=np.zeros(11), act=np.zeros(1), ctrl=np.array([1.0, 0.0]))
  assert fr.slot_state(mjm, x, 23, +1, eps, False)["ctrl"][0] == 1.0 - eps
  assert fr.slot_state(mjm, x, 23, +1, eps, True)["ctrl"][0] == 1.0 and fr.slot_state(mjm, x, 23, -1, eps, True)["ctrl"][0] == 1.0 - eps


# ---- 2: the yardstick over the fp64 oracle against a closed form ----------------------------------------------
@pytest.mark.parametrize("centered", [True, False])
def test_reference_matches_the_slide_closed_form(centered):
  """A linear system: FD is exact up to fp64 rounding over eps."""
  import mujoco_warp_amd as mjw

  mjm = mjw.load_model_from_string(fr.SLIDE_XML.format(jacobian=""))
  assert (mjm.nq, mjm.nv, mjm.na, mjm.nu) == (1, 1, 0, 1)
  x = dict(qpos=np.array([0.3]), qvel=np.array([-0.2]), act=np.zeros(0), ctrl=np.array([0.4]))
  A, B, C, D = fr.transition(mjm, fr.oracle_stepfn(mjm), x, 1e-6, centered)
  Aw, Bw = fr.slide_closed_form()
  print("A", A, "B", B, "err", np.abs(A - Aw).max(), np.abs(B - Bw).max())
  assert np.abs(A - Aw).max() < 1e-9 and np.abs(B - Bw).max() < 1e-9
  assert C.shape == (0, 2) and D.shape == (0, 1)
