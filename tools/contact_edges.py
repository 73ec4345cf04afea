"""Contact staging / pair compaction / row-cut edges of the HIP path (GPU box): one record per case of
tests/contact_cases.py CASES and POOL_CASES -- the kernel names of the traced step, the staging size of the path,
the expected contacts and survivors per world, the counters and row counts after forward and after step, the worst
contact errors (dist / pos / normal, primitive and convex) and row errors (relative to the largest entry of the
array in its world) next to their bars, and the assertions of tests/test_gpu_contact_edges.py the case fails (none
expected).
usage: python tools/contact_edges.py [out.json]      (default profiles/contact_edges.json)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import contact_cases as cc  # noqa: E402


def main():
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "contact_edges.json")
  out = {}
  for case in cc.CASES:
    out[case.id] = {k: v for k, v in cc.run_case(case).items() if k != "id"}
    print(case.id, json.dumps(out[case.id])[:300], flush=True)
  for case in cc.POOL_CASES:
    try:
      rec = cc.run_pool_case(case)
      rec["failures"] = []
    except AssertionError as e:
      rec = dict(path="pool", cmax=case.cmax, contacts=case.contacts(), failures=[("pool", str(e)[:2000])])
    out[case.id] = {k: v for k, v in rec.items() if k != "id"}
    print(case.id, json.dumps(out[case.id])[:300], flush=True)
  with open(path, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
  nbad = sum(bool(r["failures"]) for r in out.values())
  print(f"{len(out)} cases, {nbad} with failures -> {path}")
  return 1 if nbad else 0


if __name__ == "__main__":
  sys.exit(main())
