"""Capacity and degeneracy edges of the convex collision code: per family of tests/ccd_cases.py the case count, the
polytope routes and EPA exits the fp64 oracle's trace shows, the peak face-array fill / vertex count / horizon, the pass /
tie / unmatched shares of the acceptance rule for liborc32, liborc32f and (on a GPU box) the device, the worst distance
error among the passes, and the size and yield of the capacity search.
usage: python tools/ccd_edges.py [out.json]      (default profiles/ccd_edges.json)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import orc  # noqa: E402
from tests import ccd_cases as cc  # noqa: E402


def _shares(res, fam):
  out = {k: round(res[k], 5) for k in ("passed", "tie", "un")}
  out["worst_dist_err"] = float(f"{res['worst_dist']:.3g}")
  out["unmatched_failing_property"] = [fam.ids[i] for i in res["unmatched"][~res["property"]]]
  return out


def main():
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ccd_edges.json")
  try:
    import torch

    gpu = torch.cuda.is_available()
  except ImportError:
    gpu = False
  report = {"exits": {str(k): v for k, v in orc.CCD_EPA_EXITS.items()}, "caps": cc.CAPS, "families": {}}
  nbad = 0
  for name in cc.FAMILIES:
    fam, ref = cc.family(name), cc.references(name)
    bad, reach = cc.check_predicates(name)
    rec = {"cases": len(fam.recs), "iteration_counts": sorted({int(v) for v in np.stack(fam.recs)[:, 34]}), "reached": reach,
           "predicate_failures": bad}
    rec["liborc32"] = _shares(cc.classify(name, ref["o32"], [ref["o32f"]]), fam)
    rec["liborc32f"] = _shares(cc.classify(name, ref["o32f"], [ref["o32"]]), fam)
    if gpu:
      res = cc.classify(name, cc.run_device(name), [ref["o32"], ref["o32f"]])
      rec["device"] = _shares(res, fam)
      rec["device"]["failures"] = cc.verdict(name, res)
      rec["device"]["ties"] = [fam.ids[i] for i in np.nonzero(res["cls"] == 1)[0]]
      rec["device"]["unmatched"] = [fam.ids[i] for i in res["unmatched"]]
      nbad += bool(rec["device"]["failures"])
    else:
      rec["device"] = None
    nbad += bool(bad)
    report["families"][name] = rec
    print(name, {k: rec[k] for k in ("cases", "liborc32", "liborc32f", "device")}, flush=True)
  found, ids, _ = cc.capacity_search()
  report["capacity_search"] = {
    "candidates": len(ids), "iteration_counts": list(cc.CAP_ITS), "runs": len(ids) * len(cc.CAP_ITS),
    "well_conditioned_hits": {str(it): {e: len(v) for e, v in found[it][3].items()} for it in cc.CAP_ITS},
    "peak_horizon": {str(it): int(found[it][2][:, cc.T["horizon"]].max()) for it in cc.CAP_ITS},
    "not_reached": sorted(e for e in cc.CAP_EDGES if not any(found[it][3][e] for it in cc.CAP_ITS)),
  }
  with open(path, "w") as f:
    json.dump(report, f, indent=1)
    f.write("\n")
  print(f"{nbad} families with failures -> {path}")
  return 1 if nbad else 0


if __name__ == "__main__":
  sys.exit(main())
