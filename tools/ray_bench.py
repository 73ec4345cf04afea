"""Times mjw.rays on the device and prints one JSON line per configuration.

  python tools/ray_bench.py [humanoid64] [humanoid1] [apollo256] [aloha_pot] [aloha_pot_random]      (default: all five)

Each configuration puts the model's keyframe 0 in every world, runs one forward, then times `rays` with HIP
events around 20 calls after 5 warm-up calls (one event pair around the whole window, on the stream the
kernels run on), and one `step` at the same nworld the same way.  The rays start at a body's frame origin with
that body excluded: a horizontal fan (humanoid) or a 16 x 16 fan over azimuth and elevation (apollo).
Reported: ms per call, rays per second, ray x geom tests per second (rays x ngeom, the brute-force work the
kernel is asked for, not what the bounding tests let through) and ms per step.  There is no CPU fallback: without
a GPU this fails.

aloha_pot (the reference's vision scene: 204 geoms, 190 of them mesh geoms, 64,609 mesh faces) casts the 64 x 64
pixel fan of its overhead camera, from the camera's position, and aloha_pot_random the same number of rays from
there with one random direction per lane of the lower half space, so that a wave's rays share no direction.  Both
are timed without a render context (the loop over every mesh face) and with one (`ms_per_rays_call_rc`: the walk
through its mesh BVHs), and report whether the two agree bit for bit; `--no-rc` leaves the second out.
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
  "aloha_pot": dict(path="models/aloha_pot/scene.xml", nworld=64, nray=4096, nconmax=64, njmax=256, solver=None, camera="overhead_cam", fan="pixels"),
  "aloha_pot_random": dict(path="models/aloha_pot/scene.xml", nworld=64, nray=4096, nconmax=64, njmax=256, solver=None, camera="overhead_cam",
                           fan="random"),
}
WARMUP, CALLS = 5, 20
USE_RC = True  # --no-rc


def fan(kind, nray):
  """Unit directions: `flat` = nray azimuths in the horizontal plane; `dome` = 16 azimuths x nray / 16 elevations
  between -60 and +30 degrees."""
  if kind == "flat":
    az = 2 * np.pi * (np.arange(nray) + 0.5) / nray
    return np.stack([np.cos(az), np.sin(az), np.zeros(nray)], axis=1)
  nel = max(nray // 16, 1)
  az, el = np.meshgrid(2 * np.pi * (np.arange(16) + 0.5) / 16, np.deg2rad(np.linspace(-60, 30, nel)), indexing="ij")
  return np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=-1).reshape(-1, 3)[:nray]


def camera_fan(kind, mjm, cam, xmat, nray):
  """World-frame unit directions from camera cam (xmat: its frame): `pixels` = the centres of a square image's
  pixels (fovy path), `random` = seeded directions of the lower half space."""
  if kind == "random":
    v = np.random.default_rng(0).normal(0, 1, (nray, 3))
    v[:, 2] = -np.abs(v[:, 2])
    return v / np.linalg.norm(v, axis=1, keepdims=True)
  side = int(round(np.sqrt(nray)))
  assert side * side == nray
  half = np.tan(0.5 * np.deg2rad(float(mjm.cam_fovy[cam])))
  py, px = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
  v = np.stack([-half + 2 * half * (px.ravel() + 0.5) / side, half - 2 * half * (py.ravel() + 0.5) / side, -np.ones(nray)], axis=1)
  v /= np.linalg.norm(v, axis=1, keepdims=True)
  return v @ np.asarray(xmat, dtype=np.float64).reshape(3, 3).T


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
  if "camera" in cfg:
    cam, body = mjm.cam_names.index(cfg["camera"]), -1
    origin = d.cam_xpos.reshape(nworld, mjm.ncam, 3)[:, cam].clone()
    dirs = camera_fan(cfg["fan"], mjm, cam, d.cam_xmat.reshape(nworld, mjm.ncam, 9)[0, cam].cpu().numpy(), nray)
  else:
    body = mjm.body_names.index(cfg["body"]) if isinstance(cfg["body"], str) else int(cfg["body"])
    origin = d.xpos.reshape(nworld, mjm.nbody, 3)[:, body].clone()  # (nworld, 3)
    dirs = fan(cfg["fan"], nray)
  pnt = origin[:, None, :].expand(nworld, nray, 3).contiguous()
  vec = torch.as_tensor(dirs[None], dtype=torch.float32, device="cuda").contiguous()
  excl = torch.full((nray,), body, dtype=torch.int32, device="cuda")
  dist = torch.empty(nworld, nray, device="cuda")
  geomid = torch.empty(nworld, nray, dtype=torch.int32, device="cuda")
  normal = torch.empty(nworld, nray, 3, device="cuda")
  ms_rays = timed(lambda: mjw.rays(m, d, pnt, vec, None, True, excl, dist, geomid, normal), torch)
  hit = float((geomid >= 0).float().mean())
  extra = {}
  if "camera" in cfg and USE_RC:
    rc = mjw.create_render_context(mjm, nworld=nworld, cam_res=(1, 1), device="cuda")
    loop = (dist.clone(), geomid.clone(), normal.clone())
    ms_rc = timed(lambda: mjw.rays(m, d, pnt, vec, None, True, excl, dist, geomid, normal, rc=rc), torch)
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(loop, (dist, geomid, normal)))
    extra = dict(ms_per_rays_call_rc=round(ms_rc, 5), rays_per_s_rc=round(nworld * nray / (ms_rc * 1e-3)), rc_bitwise_equal=same,
                 speedup_rc=round(ms_rays / ms_rc, 3))
  ms_step = timed(lambda: mjw.step(m, d), torch)
  rays_per_s = nworld * nray / (ms_rays * 1e-3)
  return dict(config=name, nworld=nworld, nray=nray, ngeom=int(mjm.ngeom), ms_per_rays_call=round(ms_rays, 5),
              rays_per_s=round(rays_per_s), ray_geom_tests_per_s=round(rays_per_s * mjm.ngeom), hit_share=round(hit, 4), **extra,
              ms_per_step=round(ms_step, 5), warmup=WARMUP, calls=CALLS, device=torch.cuda.get_device_name(0))


if __name__ == "__main__":
  USE_RC = "--no-rc" not in sys.argv[1:]
  names = [a for a in sys.argv[1:] if a != "--no-rc"] or list(CONFIGS)
  for n in names:
    if n not in CONFIGS:
      sys.exit(f"unknown configuration {n}: one of {', '.join(CONFIGS)}")
  for n in names:
    print(json.dumps(run(n)), flush=True)
