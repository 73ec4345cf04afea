"""Times flex rendering on the device and prints one JSON line per scene.

  python tools/flex_render_bench.py [cloth] [aloha_cloth] [--res N]      (default: both scenes, 64 x 64 pixels)

Each scene runs at its benchmark nworld (bench.py CONFIGS) from its benchmark start state, takes a few steps so that
the towel has moved off its rest shape, and renders one camera (depth + segmentation + RGB, no shadows) through a
context made with render_flex.  Timed with HIP events around a window of calls on the stream the kernels run on,
after warm-up calls of the same shape:
  ms_step          one mjw.step, for scale
  ms_refit         one mjw.refit_bvh
  ms_render_walk   one mjw.render with flex_bvh_min_faces = 0 (every flex through its tree)
  ms_render_loop   one mjw.render with flex_bvh_min_faces above every face count (every face of every flex)
Walk and loop are timed twice each, alternating, and both figures are reported (their spread is the noise to hold a
difference against); the number of calls in a window is chosen from one timed call so that a window lasts about a
second (at least 2, at most 50 calls).  The two must give the same images bit for bit; the line says whether they
did.  Also reported: the context's per-world bytes (node boxes + vertex normals) and the bytes of its shared tables.
There is no CPU fallback: without a GPU this fails.
"""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
  "cloth": dict(path="models/cloth/scene.xml", nworld=1024, nconmax=200, njmax=3000, key=None, camera="side", steps=10),
  # groups 0 and 2: floor, table and the arms' visual meshes; the overhead camera's own housing (group 1) would fill the picture
  "aloha_cloth": dict(path="models/aloha_cloth/scene.xml", nworld=1024, nconmax=4096, njmax=16384, key=0, camera="overhead_cam", steps=5, groups=[0, 2]),
}
LOOP = 1 << 30


def window(fn, torch, calls, warmup):
  for _ in range(warmup):
    fn()
  beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  beg.record()
  for _ in range(calls):
    fn()
  end.record()
  torch.cuda.synchronize()
  return beg.elapsed_time(end) / calls


def timed(fn, torch):
  """(ms per call, calls): one call sizes the window."""
  one = window(fn, torch, 1, 1)
  calls = max(2, min(50, int(1000.0 / max(one, 1e-3))))
  return window(fn, torch, calls, 1), calls


def run(name, res):
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf

  cfg = CONFIGS[name]
  mjm = mjcf.load_model(os.path.join(ROOT, cfg["path"]))
  mjd = mjcf.MjData(mjm)
  if cfg["key"] is not None:
    mjcf.reset_data_keyframe(mjm, mjd, cfg["key"])
  nworld = cfg["nworld"]
  m = mjw.put_model(mjm, device="cuda")
  d = mjw.put_data(mjm, mjd, nworld=nworld, nconmax=cfg["nconmax"], njmax=cfg["njmax"], device="cuda", m=m)
  for _ in range(cfg["steps"]):
    mjw.step(m, d)
  torch.cuda.synchronize()
  cam = mjm.cam_names.index(cfg["camera"])
  rc = mjw.create_render_context(mjm, nworld=nworld, cam_res=(res, res), cam_active=[i == cam for i in range(mjm.ncam)], render_rgb=True,
                                 render_depth=True, render_seg=True, render_flex=True, enabled_geom_groups=cfg.get("groups", [0, 1, 2]), device="cuda")
  info = rc.flex_info.cpu().numpy()
  out = dict(config=name, nworld=nworld, camera=cfg["camera"], width=res, height=res, ngeom=int(mjm.ngeom), nflex=int(mjm.nflex),
             flex_faces=[int(x) for x in info[:, 4]], flex_nodes=[int(x) for x in info[:, 6]], flex_depth=[int(x) for x in info[:, 7]],
             steps_before=cfg["steps"], default_flex_bvh_min_faces=int(rc.flex_bvh_min_faces))
  per_world = (rc.flex_node_box[0].numel() + rc.flexvert_norm[0].numel()) * 4
  shared = sum(getattr(rc, n).numel() * 4 for n in ("flex_info", "flex_corner", "flex_elem_vert", "flex_edge_vert", "flex_inc_adr", "flex_inc",
                                                    "flex_bvh_node", "flex_bvh_tri", "flex_bvh_level", "flex_radius", "flex_rgba"))
  out.update(bytes_per_world=int(per_world), bytes_shared_tables=int(shared))

  ms, calls = timed(lambda: mjw.refit_bvh(m, d, rc), torch)
  out.update(ms_refit=round(ms, 5), calls_refit=calls)

  def render(min_faces):
    rc.flex_bvh_min_faces = min_faces
    return lambda: mjw.render(m, d, rc)

  images = {}
  for rep in (0, 1):
    for key, mf in (("walk", 0), ("loop", LOOP)):
      ms, calls = timed(render(mf), torch)
      out.setdefault("ms_render_" + key, []).append(round(ms, 5))
      out["calls_render_" + key] = calls
      images[key] = (rc.rgb_data.clone(), rc.depth_data.clone(), rc.seg_data.clone())
  out["walk_equals_loop_bitwise"] = all(torch.equal(a, b) for a, b in zip(images["walk"], images["loop"]))
  seg = images["walk"][2]
  out["flex_pixel_share"] = round(float((seg == -2).float().mean()), 4)
  out["geom_pixel_share"] = round(float((seg >= 0).float().mean()), 4)
  # the step last: it moves the towel, which the windows above must not see
  ms, calls = timed(lambda: mjw.step(m, d), torch)
  out.update(ms_step=round(ms, 5), calls_step=calls, device=torch.cuda.get_device_name(0))
  return out


if __name__ == "__main__":
  args = sys.argv[1:]
  res = 64
  if "--res" in args:
    i = args.index("--res")
    res = int(args[i + 1])
    del args[i : i + 2]
  names = args or list(CONFIGS)
  for n in names:
    if n not in CONFIGS:
      sys.exit(f"unknown configuration {n}: one of {', '.join(CONFIGS)}")
  for n in names:
    print(json.dumps(run(n, res)), flush=True)
