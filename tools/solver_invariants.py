"""Solver-output invariants of the HIP path on the row-count ladder (GPU box): one record per case of
tests/solver_cases.py CASES -- the kernel names of the traced step, nefc per world, each invariant's device
value with the fp32 oracle's value and the bar, the boundary share, the Newton iteration totals (device,
fp32, fp64) and which assertions of tests/test_gpu_solver_outputs.py the case fails (none expected).
usage: python tools/solver_invariants.py [out.json]      (default profiles/solver_invariants.json)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import solver_cases as sc  # noqa: E402


def record(case):
  res = sc.run_case(case)
  dev, ref = res["device"], res["fp32"]
  rec = dict(kernels=res["kernels"], targets=res["targets"], nefc=res["nefc"], njmax=case.njmax, from_twin=res["from_twin"])
  for k in sc.VALUES:
    rec[k] = dict(device=dev[k], fp32=ref[k], bar=sc.bar(ref[k]), worst_world=res["worst_world"][k])
  rec["state_mismatches"] = dev["state_bad"]
  rec["untouched"] = dict(nonfinite=dev["nonfinite"], touched=dev["touched"])
  rec["boundary_share"] = dict(device=dev["boundary_share"], fp32=ref["boundary_share"], cap=sc.BOUNDARY_CAP)
  rec["cost_excess"] = dict(device=res["cost_excess"], fp32=res["cost_excess_fp32"], bar=sc.COST_TOL)
  rec["niter"] = res["niter"]
  rec["step"] = dict(qpos=res["step_qpos"], qvel=res["step_qvel"], bars=[sc.QPOS_TOL, sc.QVEL_TOL])
  if "staged_bitwise" in res:
    rec["staged_bitwise"] = res["staged_bitwise"]
  rec["twin_bitwise"] = res["twin_bitwise"]
  rec["failures"] = [name for name, _ in sc.failures(case, res)]
  return rec


def main():
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "solver_invariants.json")
  out = {}
  for case in sc.CASES:
    out[case.id] = record(case)
    print(case.id, json.dumps(out[case.id])[:300], flush=True)
  with open(path, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
  nbad = sum(bool(r["failures"]) for r in out.values())
  print(f"{len(out)} cases, {nbad} with failures -> {path}")
  return 1 if nbad else 0


if __name__ == "__main__":
  sys.exit(main())
