"""Body, sensor, stage and row-source edges of the sensor kernel (GPU box): one line per case of tests/sensor_cases.py
CASES -- nbody / nv / nsensor, the rows per world, the sensor kernel the traced step launched, and per field
(sensordata, cacc, cfrc_int, cfrc_ext) [device error, fp32-oracle error, bar], all in units of the strict bar
(1e-5 |want| + 1e-6 max|want| per world; three significant digits), bar = max(1, 4 x the fp32 oracle's error), and
the checks of tests/test_gpu_sensor_edges.py the case fails (none expected).
usage: python tools/sensor_edges.py [out.json] [case id substring ...]      (default profiles/sensor_edges.json)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import sensor_cases as sc  # noqa: E402


def _sig(x):
  return float(f"{x:.3g}")


def main():
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sensor_edges.json")
  sel = sys.argv[2:]
  cases = {}
  for case in sc.CASES:
    if sel and not any(s in case.id for s in sel):
      continue
    res = sc.run_case(case)
    worst = max(((v["device"] / v["bar"], k) for k, v in res["values"].items()), default=None)
    print(case.id, "worst device / bar", worst, "failures", res["failures"], flush=True)
    rec = {k: res[k] for k in ("edge", "nbody", "nv", "nsensor", "nefc", "kernels")}
    rec["values"] = {k: [_sig(v["device"]), _sig(v["fp32_oracle"]), _sig(v["bar"])] for k, v in res["values"].items()}
    rec["failures"] = res["failures"]
    cases[case.id] = rec
  with open(path, "w") as f:
    f.write('{"unit": "strict bar: 1e-5 |want| + 1e-6 max|want| per world", "values": "[device, fp32 oracle, bar]",\n "cases": {\n')
    f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in cases.items()))
    f.write("\n }}\n")
  nbad = sum(bool(r["failures"]) for r in cases.values())
  print(f"{len(cases)} cases, {nbad} with failures -> {path}")
  return 1 if nbad else 0


if __name__ == "__main__":
  sys.exit(main())
