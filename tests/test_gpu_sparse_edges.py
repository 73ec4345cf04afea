"""The sparse path at every tree-shape, stride and subtree-size edge, on the device (tests/sparse_cases.py).

Per case: the four smooth stages one at a time, the solve, one traced step and a 3-step rollout, twice from fresh Data.
`sparse_cases.measure` compares every smooth field (normwise; subtree_com, cinert, crb, cfrc_int per tree too), qM per tree,
L' D L rebuilt from the device's qLD (factor_trees), the backward error of qacc_smooth (solve_trees), efc_Ma against M qacc
(mul_m_trees), the solver invariants, the cost excess, qacc and the stepped qpos / qvel with the fp64 oracle; world 3 must
equal world 0 and the second run the first, bitwise; the traced step must run the sp:: kernels."""

import pytest

from tests import sparse_cases as sp


@pytest.mark.gpu
@pytest.mark.parametrize("case", sp.CASES, ids=[c.id for c in sp.CASES])
def test_gpu_sparse_edges(case):
  res = sp.run_case(case)
  print(case.id, res["counts"], res["nefc"], {k: v["device"] for k, v in res["values"].items()})
  assert not res["failures"], res["failures"]
