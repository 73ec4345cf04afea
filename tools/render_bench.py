"""Times mjw.render on the device and prints one JSON line per configuration.

  python tools/render_bench.py [humanoid] [apollo] [aloha_pot]      (default: all three)

Each configuration puts the model's keyframe 0 in every world, runs one forward, and renders one body-mounted
camera of the model at 64 x 64 in three ways: depth + segmentation, RGB without shadows, RGB with shadows.  Each is
timed with HIP events around 20 `render` calls after 5 warm-up calls (one event pair around the whole window, on
the stream the kernels run on).  For depth + segmentation the route without `render` is timed the same way at
the same build (not for aloha_pot): the same pixel rays made in torch from d.cam_xpos / d.cam_xmat (origins and directions as
(nworld, pixels, 3) tensors), one `mjw.rays` call, and the depth multiply and background fill in torch.
Reported: ms per call and pixels per second.  There is no CPU fallback: without a GPU this fails.

aloha_pot is the reference's vision scene (204 geoms, 190 of them mesh geoms, 64,609 mesh faces): its overhead
camera at a small nworld, so that a build that loops over every mesh face finishes too.  `render` walks the mesh
BVHs of its context; `--face-loop` times the loop over every face instead (a per-world batched mesh_vert of
identical rows), for the comparison at one build.  The line also reports the host time of create_render_context,
which builds the trees.
"""

import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
  "humanoid": dict(path="models/humanoid.xml", nworld=8192, nconmax=24, njmax=64, solver="CG", camera="egocentric"),
  "apollo": dict(path="models/apptronik_apollo/scene_flat.xml", nworld=4096, nconmax=16, njmax=64, solver=None, camera="torso_oak_d_pro_w_front"),
  "aloha_pot": dict(path="models/aloha_pot/scene.xml", nworld=64, nconmax=64, njmax=256, solver=None, camera="overhead_cam", world_camera=True,
                    rays_route=False),
}
FACE_LOOP = False  # --face-loop
WARMUP, CALLS = 5, 20
W = H = 64


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


def local_rays(mjm, cam):
  """The camera-frame directions of the W x H pixels, (H * W, 3) float64 (the kernel's pixel_ray, fovy path)."""
  half_h = np.tan(0.5 * np.deg2rad(float(mjm.cam_fovy[cam])))
  py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
  x = -half_h * W / H + 2 * half_h * W / H * (px.ravel() + 0.5) / W
  y = half_h - 2 * half_h * (py.ravel() + 0.5) / H
  v = np.stack([x, y, -np.ones(W * H)], axis=1)
  return v / np.linalg.norm(v, axis=1, keepdims=True)


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
  nworld = cfg["nworld"]
  d = mjw.put_data(mjm, mjd, nworld=nworld, nconmax=cfg["nconmax"], njmax=cfg["njmax"], device="cuda", m=m)
  mjw.forward(m, d)
  torch.cuda.synchronize()
  cam = mjm.cam_names.index(cfg["camera"])
  assert float(mjm.cam_sensorsize[cam][1]) == 0.0 and (cfg.get("world_camera") or int(mjm.cam_bodyid[cam]) > 0)
  if FACE_LOOP:  # identical rows per world: the trees are not used
    m.mesh_vert = m.mesh_vert.repeat(nworld, *([1] * (m.mesh_vert.dim() - 1))).contiguous()
  active = [i == cam for i in range(mjm.ncam)]
  npix = W * H
  out = dict(config=name, nworld=nworld, camera=cfg["camera"], width=W, height=H, ngeom=int(mjm.ngeom), nlight=int(mjm.nlight),
             nmeshface=int(mjm.nmeshface), face_loop=FACE_LOOP)

  def case(key, **kw):
    t0 = time.perf_counter()
    rc = mjw.create_render_context(mjm, nworld=nworld, cam_res=(W, H), cam_active=active, device="cuda", **kw)
    out["s_create_render_context"] = round(time.perf_counter() - t0, 4)
    ms = timed(lambda: mjw.render(m, d, rc), torch)
    out["ms_" + key], out["pixels_per_s_" + key] = round(ms, 5), round(nworld * npix / (ms * 1e-3))
    return rc

  rc = case("depth_seg", render_rgb=False, render_depth=True, render_seg=True)
  out["hit_share"] = round(float((rc.seg_data >= 0).float().mean()), 4)
  case("rgb", render_rgb=True, render_depth=False, render_seg=False)
  case("rgb_shadows", render_rgb=True, render_depth=False, render_seg=False, use_shadows=True)

  if not cfg.get("rays_route", True):
    out.update(warmup=WARMUP, calls=CALLS, device=torch.cuda.get_device_name(0))
    return out
  # the route without render: rays made in torch, one rays call, depth in torch
  local = torch.as_tensor(local_rays(mjm, cam), dtype=torch.float32, device="cuda")
  cosine = -local[:, 2].contiguous()
  excl = torch.full((npix,), -1, dtype=torch.int32, device="cuda")
  dist = torch.empty(nworld, npix, device="cuda")
  geomid = torch.empty(nworld, npix, dtype=torch.int32, device="cuda")
  normal = torch.empty(nworld, npix, 3, device="cuda")
  depth = torch.empty(nworld, npix, device="cuda")
  groups = (1, 1, 1, 0, 0, 0)  # the context's default groups 0-2

  def rays_route():
    xpos = d.cam_xpos.reshape(nworld, mjm.ncam, 3)[:, cam]
    xmat = d.cam_xmat.reshape(nworld, mjm.ncam, 3, 3)[:, cam]
    pnt = xpos[:, None, :].expand(nworld, npix, 3).contiguous()
    vec = torch.matmul(local[None], xmat.transpose(1, 2)).contiguous()
    mjw.rays(m, d, pnt, vec, groups, True, excl, dist, geomid, normal)
    torch.mul(dist, cosine[None], out=depth)
    depth.masked_fill_(geomid < 0, 0.0)

  ms = timed(rays_route, torch)
  out["ms_depth_seg_rays_route"], out["pixels_per_s_depth_seg_rays_route"] = round(ms, 5), round(nworld * npix / (ms * 1e-3))
  agree = float((geomid == rc.seg_data.reshape(nworld, npix)).float().mean())
  out["rays_route_seg_agreement"] = round(agree, 5)
  out.update(warmup=WARMUP, calls=CALLS, device=torch.cuda.get_device_name(0))
  return out


if __name__ == "__main__":
  FACE_LOOP = "--face-loop" in sys.argv[1:]
  names = [a for a in sys.argv[1:] if a != "--face-loop"] or list(CONFIGS)
  for n in names:
    if n not in CONFIGS:
      sys.exit(f"unknown configuration {n}: one of {', '.join(CONFIGS)}")
  for n in names:
    print(json.dumps(run(n)), flush=True)
