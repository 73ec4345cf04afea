"""Contact staging, pair compaction and row cuts at every count edge, on the device (tests/contact_cases.py).

One forward and one traced step per case, both checked by `contact_cases.check` against the fp64 oracle of the same
states: the contacts in slot order, the rows, contact.efc_address, nacon and ncollision; the traced step must run the
kernels the case names (direct mjw_kernel + dense_kernel, fused step_kernel, generic mjw_kernel, sparse
forward_kernel).  The pool-mode cases rebuild the rows from a pool a contactfilter callback edited."""

import pytest

from tests import contact_cases as cc


@pytest.mark.gpu
@pytest.mark.parametrize("case", cc.CASES, ids=[c.id for c in cc.CASES])
def test_gpu_contact_edges(case):
  res = cc.run_case(case)
  print(case.id, res["kernels"], res["worst"], res["forward"])
  assert not res["failures"], res["failures"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", cc.POOL_CASES, ids=[c.id for c in cc.POOL_CASES])
def test_gpu_contact_rows_from_an_edited_pool(case):
  res = cc.run_pool_case(case)
  assert any(k0 > 0 for k0, _ in res["ncon_world"])  # a world's pool range starts mid-pool
  print(case.id, res["worst"], res["ncon_world"])
