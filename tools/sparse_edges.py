"""Tree-shape, stride and subtree-size edges of the sparse path (GPU box): one line per case of tests/sparse_cases.py
CASES -- ntree / nv / nbody / njnt, the number of block-summed subtrees, the path (chain / small / general) of every tree
as runs of [dofs, path, count], the row counts, the solver iterations, every measured value as [device, fp32 oracle on the
same states] (three significant digits; the bars stand once, under "bars"), and the assertions of
tests/test_gpu_sparse_edges.py the case fails (none expected).  "kernels" holds the traced step's kernel names, which are
the same for every case (a case whose names differ carries its own).
usage: python tools/sparse_edges.py [out.json] [case id substring ...]      (default profiles/sparse_edges.json)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import sparse_cases as sp  # noqa: E402


def _sig(x):
  return float(f"{x:.3g}") if isinstance(x, float) else x


def main():
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_edges.json")
  sel = sys.argv[2:]
  cases, bars, kernels = {}, {}, None
  for case in sp.CASES:
    if sel and not any(s in case.id for s in sel):
      continue
    res = sp.run_case(case)
    worst = max(((v["device"] / v["bar"], k) for k, v in res["values"].items() if v["bar"]), default=None)
    print(case.id, res["counts"], "worst value / bar", worst, "failures", res["failures"], flush=True)
    bars.update({k: v["bar"] for k, v in res["values"].items()})
    kernels = res["kernels"] if kernels is None else kernels
    rec = {k: res[k] for k in ("counts", "nbig", "njmax", "trees", "nefc", "niter")}
    if res["kernels"] != kernels:
      rec["kernels"] = res["kernels"]
    rec["values"] = {k: [_sig(v["device"]), _sig(v["fp32_oracle"])] for k, v in res["values"].items()}
    rec["failures"] = res["failures"]
    cases[case.id] = rec
  with open(path, "w") as f:
    f.write('{"bars": ' + json.dumps(bars) + ',\n "kernels": ' + json.dumps(kernels) + ',\n "cases": {\n')
    f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in cases.items()))
    f.write("\n }}\n")
  nbad = sum(bool(r["failures"]) for r in cases.values())
  print(f"{len(cases)} cases, {nbad} with failures -> {path}")
  return 1 if nbad else 0


if __name__ == "__main__":
  sys.exit(main())
