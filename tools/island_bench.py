"""Times mjw.island on the device and prints one JSON line per configuration.

  python tools/island_bench.py [humanoid] [aloha_cloth]      (default: both)

Each configuration runs in a child process of its own under a time limit, and the tool ends at the first one that
fails or runs out of time (nothing more is started on the device after a failure).  A configuration puts the
model's keyframe in every world, advances it `settle` steps (humanoid: 100 from the squat key; aloha_cloth: 20), then
times with HIP events on the stream the kernels run on, one event pair per launch, 30 launches after 5 warm-up
launches each:

  island        the mjw_island launch (union-find over the trees, tree / dof / row maps)
  fwd_position  the position stage on the same state, whose rows the launch reads
  step          one mjw.step of the same model, timed last (it advances the state)

Reported per item: median, minimum and maximum ms; `island_over_step` and `fwd_position_over_step` are ratios of the
medians; `nisland_min` / `nisland_max` are over the worlds.  There is no CPU fallback: without a GPU this fails.
"""

import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
  "humanoid": dict(path="models/humanoid.xml", nworld=8192, nconmax=24, njmax=64, solver="CG", key=0, settle=100, limit_s=240),
  "aloha_cloth": dict(path="models/aloha_cloth/scene.xml", nworld=1024, nconmax=4096, njmax=16384, solver=None, key=0, settle=20, limit_s=420),
}
WARMUP, CALLS = 5, 30


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

  cfg = CONFIGS[name]
  mjm = mjcf.load_model(os.path.join(ROOT, cfg["path"]))
  if cfg["solver"]:
    mjw.override_model(mjm, [f"opt.solver={cfg['solver']}"])
  mjd = mjcf.MjData(mjm)
  mjcf.reset_data_keyframe(mjm, mjd, cfg["key"])
  m = mjw.put_model(mjm, device="cuda")
  nworld = cfg["nworld"]
  d = mjw.put_data(mjm, mjd, nworld=nworld, nconmax=cfg["nconmax"], njmax=cfg["njmax"], device="cuda", m=m)
  for _ in range(cfg["settle"]):
    mjw.step(m, d)
  mjw.fwd_position(m, d)
  torch.cuda.synchronize()
  nefc = torch.clamp(d.nefc.reshape(-1), max=d.njmax).double()
  out = dict(config=name, nworld=nworld, nv=int(mjm.nv), ntree=int(m.ntree), njmax=cfg["njmax"], settle=cfg["settle"], sparse=bool(m.is_sparse),
             nefc_mean=round(float(nefc.mean()), 2), nefc_max=int(nefc.max()))
  out["island_ms"] = timed(lambda: mjw.island(m, d), torch)
  out["nisland_min"], out["nisland_max"] = int(d.nisland.min()), int(d.nisland.max())
  out["fwd_position_ms"] = timed(lambda: mjw.fwd_position(m, d), torch)
  out["step_ms"] = timed(lambda: mjw.step(m, d), torch)
  out["island_over_step"] = round(out["island_ms"]["median"] / out["step_ms"]["median"], 5)
  out["fwd_position_over_step"] = round(out["fwd_position_ms"]["median"] / out["step_ms"]["median"], 5)
  out.update(warmup=WARMUP, calls=CALLS, device=torch.cuda.get_device_name(0))
  return out


if __name__ == "__main__":
  if len(sys.argv) == 3 and sys.argv[1] == "--one":
    print(json.dumps(run(sys.argv[2])), flush=True)
    sys.exit(0)
  names = sys.argv[1:] or list(CONFIGS)
  for n in names:
    if n not in CONFIGS:
      sys.exit(f"unknown configuration {n}: one of {', '.join(CONFIGS)}")
  for n in names:
    try:
      rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", n], timeout=CONFIGS[n]["limit_s"]).returncode
    except subprocess.TimeoutExpired:
      sys.exit(f"{n}: no result within {CONFIGS[n]['limit_s']} s; stopping")
    if rc != 0:
      sys.exit(f"{n}: failed with exit status {rc}; stopping")
