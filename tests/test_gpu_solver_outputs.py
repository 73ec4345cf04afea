"""What the constraint solve writes, at every dense / fused / generic / sparse dispatch edge and row-count edge.

One traced `step` per case of tests/solver_cases.py CASES (pyramidal cones, a synthetic ladder model, one
world per target row count).  The trace must name the solve kernel the dispatch table gives for the case's
nv, njmax, solver and integrator; the invariants of tests/solver_cases.py (efc_force and efc_state against
the row law, qfrc_constraint = J' f, efc_Ma = M qacc, rows past min(nefc, njmax) untouched, the fp64 cost
excess, the Newton iteration total) are evaluated on the arrays the device itself wrote, and qpos / qvel
are compared with the fp64 oracle's step.

Bars: force / force_row / qfrc / qfrc_dof / Ma at max(1e-5, 2 x the fp32 oracle's own residual on that invariant in that case),
never above 1e-4 (tests/test_gpu_parity_models.py fp32_bar); no state mismatch; at most 5 % boundary rows;
cost excess <= 1e-5 relative; Newton's device iteration total <= the fp32 oracle's plus the larger of one
per world and the fp32 / fp64 oracle builds' own difference; qpos 1e-5 and qvel 5e-3 normwise.

The step's inputs that the entry point does not leave in Data are taken from a twin Data run through
`forward` on the same state, whose qacc and efc_force must be bitwise the stepped ones.  The fused cases
also run the chained stage functions and require bitwise equal qacc, efc_force, efc_state, qpos and qvel.
"""

import pytest

from tests import solver_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sc.CASES, ids=[c.id for c in sc.CASES])
def test_solver_outputs(case):
  res = sc.run_case(case)
  dev, ref, ni = res["device"], res["fp32"], res["niter"]
  print(f"{case.id}: kernels {res['kernels']}")
  print(f"  nefc {res['nefc']} from_twin {res['from_twin']} boundary {dev['boundary']} / {dev['rows']} state_bad {dev['state_bad']} "
        f"nonfinite {dev['nonfinite']} touched {dev['touched']}")
  for k in sc.VALUES:
    print(f"  {k}: device {dev[k]:.3g} fp32 oracle {ref[k]:.3g} bar {sc.bar(ref[k]):.3g} (worst world {res['worst_world'][k]})")
  print(f"  cost excess {res['cost_excess']:.3g} (fp32 oracle {res['cost_excess_fp32']:.3g}); niter device {ni['device']} fp32 {ni['fp32']} "
        f"fp64 {ni['fp64']} margin {ni['margin']}; step qpos {res['step_qpos']:.3g} qvel {res['step_qvel']:.3g}")
  bad = sc.failures(case, res)
  assert not bad, (case.id, bad)
