"""Times mjw.rays on the device and prints one JSON line per configuration.

  python tools/ray_bench.py [humanoid64] [humanoid1] [apollo256]      (default: all three)

Each configuration puts the model's keyframe 0 in every world, runs one forward, then times `rays` with HIP
events around 20 calls after 5 warm-up calls (one event pair around the whole window, on the stream the
kernels run on), and one `step` at the same nworld the same way.  The rays start at a body's frame origin with
that body excluded: a horizontal fan (humanoid) or a 16 x 16 fan over azimuth and elevation (apollo).
Reported: ms per call, rays per second, ray x geom tests per second (rays x ngeom, the brute-force work the
kernel is asked for, not what the bounding tests let through) and ms per step.  There is no CPU fallback: without
a GPU this fails.
"""

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
  "humanoid64": dict(path="models/humanoid.xml", nworld=8192, nray=64, nconmax=24, njmax=64, solver="CG", body="torso", fan="flat"),
  "humanoid1": dict(path="models/humanoid.xml", nworld=8192, nray=1, nconmax=24, njmax=64, solver="CG", body="torso", fan="flat"),
  "apollo256": dict(path="models/apptronik_apollo/scene_flat.xml", nworld=4096, nray=256, nconmax=16, njmax=64, solver=None, body=1, fan="dome"),
}
WARMUP, CALLS = 5, 20


def fan(kind, nray):
  """Unit directions: `flat` = nray azimuths in the horizontal plane; `dome` = 16 azimuths x nray / 16 elevations
  between -60 and +30 degrees."""
  if kind == "flat":
    az = 2 * np.pi * (np.arange(nray) + 0.5) / nray
    return np.stack([np.cos(az), np.sin(az), np.zeros(nray)], axis=1)
  nel = max(nray // 16, 1)
  az, el = np.meshgrid(2 * np.pi * (np.arange(16) + 0.5) / 16, np.deg2rad(np.linspace(-60, 30, nel)), indexing="ij")
  return np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=-1).reshape(-1, 3)[:nray]


def timed(fn, torch):
  for _ in range(WARMUP):
    fn()
  beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  beg.record()
  for _ in range(CALLS):
    fn()
  end.record()
  torch.cuda.synchronize()
  return beg.elapsed_time(end) / CALLS


def run(name):
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf

  cfg = CONFIGS[name]
  mjm = mjcf.load_model(os.path.join(ROOT, cfg["path"]))
  if cfg["solver"]:
    mjw.override_model(mjm, [f"opt.solver={cfg['solver']}"])
  mjd = mjcf.MjData(mjm)
  mjcf.reset_data_keyframe(mjm, mjd, 0)
  m = mjw.put_model(mjm, device="cuda")
  nworld, nray = cfg["nworld"], cfg["nray"]
  d = mjw.put_data(mjm, mjd, nworld=nworld, nconmax=cfg["nconmax"], njmax=cfg["njmax"], device="cuda", m=m)
  mjw.forward(m, d)
  torch.cuda.synchronize()
  body = mjm.body_names.index(cfg["body"]) if isinstance(cfg["body"], str) else int(cfg["body"])
  origin = d.xpos.reshape(nworld, mjm.nbody, 3)[:, body].clone()  # (nworld, 3)
  pnt = origin[:, None, :].expand(nworld, nray, 3).contiguous()
  vec = torch.as_tensor(fan(cfg["fan"], nray)[None], dtype=torch.float32, device="cuda").contiguous()
  excl = torch.full((nray,), body, dtype=torch.int32, device="cuda")
  dist = torch.empty(nworld, nray, device="cuda")
  geomid = torch.empty(nworld, nray, dtype=torch.int32, device="cuda")
  normal = torch.empty(nworld, nray, 3, device="cuda")
  ms_rays = timed(lambda: mjw.rays(m, d, pnt, vec, None, True, excl, dist, geomid, normal), torch)
  hit = float((geomid >= 0).float().mean())
  ms_step = timed(lambda: mjw.step(m, d), torch)
  rays_per_s = nworld * nray / (ms_rays * 1e-3)
  return dict(config=name, nworld=nworld, nray=nray, ngeom=int(mjm.ngeom), ms_per_rays_call=round(ms_rays, 5),
              rays_per_s=round(rays_per_s), ray_geom_tests_per_s=round(rays_per_s * mjm.ngeom), hit_share=round(hit, 4),
              ms_per_step=round(ms_step, 5), warmup=WARMUP, calls=CALLS, device=torch.cuda.get_device_name(0))


if __name__ == "__main__":
  names = sys.argv[1:] or list(CONFIGS)
  for n in names:
    if n not in CONFIGS:
      sys.exit(f"unknown configuration {n}: one of {', '.join(CONFIGS)}")
  for n in names:
    print(json.dumps(run(n)), flush=True)
