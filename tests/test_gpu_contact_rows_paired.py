"""Contact rows built two staged contacts per pass (csrc/mjw_step.hip collision_and_constraints, nv <= 32).

Lane 32 h + i works on contact 2 p + h, dof i; the rows of a pass are taken in chunks of four and each row's J.qvel is one
half of a two-sum reduction.  The smallest shapes at which that can go wrong, each run through `contact_cases.run_case`:
one forward and one traced step, both checked by `contact_cases.check` at its own bars against the fp64 oracle of a
`ladder_xml` scene, the traced step naming the kernel that ran:

  unequal halves      1, 2 and 3 contacts, neighbours of condim (1, 3) and (3, 1): halves with 1 and 4 rows, a pass
                      without a partner; direct path at nv = 32 (the largest paired nv), fused path at nv = 17
  several chunks      a condim-4 (6 rows) and a condim-6 (10 rows) contact in one pass, njmax inside the first contact,
                      between the two, inside the second, and holding all 16 rows
  pool end in a pair  nworld 1, naconmax 1 of 2 contacts and 3 of 4: the kept contacts end inside a pass

and, bitwise, that a contact's rows do not depend on the half that builds them: a tree's contact staged at index 0 in one
world and at index 1 in the other gives the same row bits.
"""

import numpy as np
import pytest

from tests import contact_cases as cc
from tests.contact_cases import Case, S, run_case


def _pad(path, n):
  """npad: direct cases at nv = 32, fused cases at nv = 17."""
  return (32 if path == "direct" else 17) - n


def _unequal(path):
  bodies = S(1, 1) + S(1, 3) + S(1, 1) + S(1, 3)
  worlds = [{0: "down"}, {1: "down"}, {0: "down", 1: "down"}, {1: "down", 2: "down"}, {0: "down", 1: "down", 2: "down"},
            {1: "down", 2: "down", 3: "down"}]
  return Case(f"unequal-{path}", path, bodies, worlds, njmax=64, npad=_pad(path, 4))


def _chunks(path, njmax, tag):
  # rows 0..5: the condim-4 contact, rows 6..15: the condim-6 contact
  return Case(f"chunks-{path}-{tag}", path, S(1, 4) + S(1, 6), [{0: "down", 1: "down"}], njmax=njmax, npad=_pad(path, 2))


def _pool(path, naconmax, ncon):
  return Case(f"poolpair-{path}-{naconmax}of{ncon}", path, S(4, 3), [{b: "down" for b in range(ncon)}], njmax=64, npad=_pad(path, 4),
              naconmax=naconmax)


CASES = []
for _path in ("fused", "direct"):
  CASES.append(_unequal(_path))
  CASES += [_chunks(_path, 4, "first"), _chunks(_path, 6, "between"), _chunks(_path, 9, "second"), _chunks(_path, 16, "all")]
  CASES += [_pool(_path, 1, 2), _pool(_path, 3, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gpu_contact_rows_paired(case):
  res = run_case(case)
  print(case.id, res["kernels"], res["worst"], res["forward"])
  assert not res["failures"], res["failures"]


# ---- even / odd slot symmetry ---------------------------------------------------------------------------
NPAD = 8  # nv = 1 + 9 + 8 = 18: the fused step kernel runs (nv 17..28)


def _symmetry_xml():
  """A plane; body P, a condim-1 sphere on a vertical slide, first in geom order; tree Q, a free base with a chain of three
  hinges that ends in a condim-3 sphere, the only geom of Q that collides; NPAD slide bodies without a colliding geom."""
  col = 'contype="0" conaffinity="1"'
  off = 'contype="0" conaffinity="0"'
  s = ['<mujoco><option timestep="0.002" cone="pyramidal" solver="CG" jacobian="dense"><flag eulerdamp="disable"/></option><worldbody>',
       '<geom type="plane" size="20 20 .1" contype="1" conaffinity="0" condim="1"/>',
       f'<body pos="0 0 0"><joint type="slide" axis="0 0 1"/><geom type="sphere" size="0.05" pos="0 0 0.05" {col} condim="1"/></body>',
       f'<body pos="0.5 0 0.48"><freejoint/><geom type="sphere" size="0.06" {off}/>',
       f'<body pos="0 0 -0.15"><joint type="hinge" axis="0 1 0"/><geom type="capsule" size="0.02" fromto="0 0 0 0 0 0.15" {off}/>',
       f'<body pos="0.05 0 -0.15"><joint type="hinge" axis="1 0 0"/><geom type="capsule" size="0.02" fromto="0 0 0 -0.05 0 0.15" {off}/>',
       f'<body pos="0 0.05 -0.15"><joint type="hinge" axis="0 0 1"/><geom type="capsule" size="0.02" fromto="0 0 0 0 -0.05 0.15" {off}/>',
       f'<geom type="sphere" size="0.05" {col} condim="3"/>',
       '</body></body></body></body>']
  for p in range(NPAD):
    s.append(f'<body pos="{1.0 + 0.1 * p} 0 0"><joint type="slide" axis="0 0 1"/><geom type="sphere" size="0.05" pos="0 0 0.05" {off}/></body>')
  s.append("</worldbody></mujoco>")
  return "".join(s)


def _bits(t):
  return t.detach().cpu().numpy().astype(np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["step", "forward"])
def test_gpu_contact_rows_same_bits_in_either_half(entry):
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf
  from mujoco_warp_amd.forward import StepTracer

  mjm = mjcf.load_model_from_string(_symmetry_xml())
  nv = mjm.nv
  assert nv == 1 + 9 + NPAD and mjm.nq == nv + 1
  rng = np.random.default_rng(9)
  qpos = np.tile(mjm.qpos0, (2, 1))
  qpos[:, 8:11] = (0.1, -0.08, 0.3)  # Q's hinges, the same in both worlds
  qpos[0, 0], qpos[1, 0] = cc.CLEAR, -cc.PEN  # world A: P up, Q's contact is staged at index 0; world B: P down, at index 1
  qvel = np.tile(rng.normal(0, 0.3, nv), (2, 1))
  m = mjw.put_model(mjm, device="cuda")
  d = mjw.make_data(mjm, nworld=2, njmax=64, naconmax=8, device="cuda", m=m)
  d.qpos[:] = torch.as_tensor(qpos, dtype=torch.float32, device="cuda")
  d.qvel[:] = torch.as_tensor(qvel, dtype=torch.float32, device="cuda")
  if entry == "step":
    tracer = StepTracer()
    tracer.step(m, d)
    torch.cuda.synchronize()
    names = [k for k, _ in tracer.durations()[0]]
    assert "mjw::step_kernel<79, false, 7, false, 28>" in names, names
  else:
    mjw.forward(m, d)
    torch.cuda.synchronize()
  assert d.nefc.cpu().numpy().ravel().tolist() == [4, 5], d.nefc  # Q's pyramid; P's row, then Q's pyramid
  assert int(d.nacon[0]) == 3
  J = _bits(d.efc.J)
  a, b = slice(0, 4), slice(1, 5)
  assert np.array_equal(J[0, a, 1:nv], J[1, b, 1:nv]), (J[0, a, 1:nv], J[1, b, 1:nv])
  assert np.any(J[0, a, 1:10] & 0x7fffffff) and not np.any(J[0, a, 10:nv] & 0x7fffffff)
  assert not np.any(J[0, a, 0] & 0x7fffffff) and not np.any(J[1, b, 0] & 0x7fffffff)  # P's column
  for k in ("vel", "D", "aref", "pos"):
    x = _bits(getattr(d.efc, k))
    assert np.array_equal(x[0, a], x[1, b]), (k, x[0, a], x[1, b])
  assert np.all(np.abs(d.efc.vel[0, a].cpu().numpy()) > 0)  # the reduction had something to add
