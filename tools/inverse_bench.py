"""Times mjw.inverse on the device and prints one JSON line per configuration.

  python tools/inverse_bench.py [humanoid] [franka]      (default: both)

Each configuration puts the model's keyframe 0 (qpos0 for franka, which has none) in every world, advances it 10 steps (so that contacts exist), runs
one forward, then times with HIP events on the stream the kernels run on, one event pair per launch, 30 launches
after 5 warm-up launches each:

  constraint   the inverse constraint launch alone (mjw_inverse: row law at d.qacc, J'f, M qacc, the combine)
  inverse      the whole mjw.inverse call (position and velocity stages, their sensors, the launch above, sensor_acc)
  solve        mjw.solve on the same state, the launch the constraint launch is expected to stay below

Reported per item: median, minimum and maximum ms.  `floor_ms` is the constraint launch's bytes moved (the live J
rows twice, qM once, the per-row and per-dof vectors) over 8 TB/s.  There is no CPU fallback: without a GPU this
fails.
"""

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
  "humanoid": dict(path="models/humanoid.xml", nworld=8192, nconmax=24, njmax=64, solver="CG", key=0),
  "franka": dict(path="models/franka_emika_panda/scene.xml", nworld=16384, nconmax=16, njmax=64, solver=None, key=None),  # no keyframe: qpos0
}
WARMUP, CALLS, SETTLE = 5, 30, 10
HBM_BYTES_PER_S = 8e12


def timed(fn, torch):
  """ms of each of CALLS launches of fn, one event pair per launch."""
  for _ in range(WARMUP):
    fn()
  pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
  torch.cuda.synchronize()
  for beg, end in pairs:
    beg.record()
    fn()
    end.record()
  torch.cuda.synchronize()
  ms = np.array([beg.elapsed_time(end) for beg, end in pairs])
  return dict(median=round(float(np.median(ms)), 5), min=round(float(ms.min()), 5), max=round(float(ms.max()), 5))


def run(name):
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf
  from mujoco_warp_amd.inverse import inv_constraint

  cfg = CONFIGS[name]
  mjm = mjcf.load_model(os.path.join(ROOT, cfg["path"]))
  if cfg["solver"]:
    mjw.override_model(mjm, [f"opt.solver={cfg['solver']}"])
  mjd = mjcf.MjData(mjm)
  if cfg["key"] is not None:
    mjcf.reset_data_keyframe(mjm, mjd, cfg["key"])
  m = mjw.put_model(mjm, device="cuda")
  nworld = cfg["nworld"]
  d = mjw.put_data(mjm, mjd, nworld=nworld, nconmax=cfg["nconmax"], njmax=cfg["njmax"], device="cuda", m=m)
  for _ in range(SETTLE):
    mjw.step(m, d)
  mjw.forward(m, d)
  torch.cuda.synchronize()
  nefc = torch.clamp(d.nefc.reshape(-1), max=d.njmax).double()
  row_bytes = 4 * (m.njrow if m.is_sparse else m.nv_pad)
  qm_bytes = 4 * (m.nM if m.is_sparse else m.nv_pad * m.nv_pad)
  # J rows twice; aref, D, force, state per row; qM; qacc, bias, passive in and qfrc_constraint, Ma, qfrc_inverse out per dof
  moved = float(nefc.sum()) * (2 * row_bytes + 16) + nworld * (qm_bytes + 6 * 4 * mjm.nv)
  out = dict(config=name, nworld=nworld, nv=int(mjm.nv), njmax=cfg["njmax"], nefc_mean=round(float(nefc.mean()), 2), sparse=bool(m.is_sparse),
             bytes_moved=int(moved), floor_ms=round(moved / HBM_BYTES_PER_S * 1e3, 5))
  out["constraint_ms"] = timed(lambda: inv_constraint(m, d), torch)
  out["inverse_ms"] = timed(lambda: mjw.inverse(m, d), torch)
  out["solve_ms"] = timed(lambda: mjw.solve(m, d), torch)
  out.update(warmup=WARMUP, calls=CALLS, device=torch.cuda.get_device_name(0))
  return out


if __name__ == "__main__":
  names = sys.argv[1:] or list(CONFIGS)
  for n in names:
    if n not in CONFIGS:
      sys.exit(f"unknown configuration {n}: one of {', '.join(CONFIGS)}")
  for n in names:
    print(json.dumps(run(n)), flush=True)
