"""Times mjw.render with and without textures on the device and prints one JSON line.

  python tools/texture_bench.py [--windows N]      (default: 5 windows each)

The scene of tools/render_bench.py `humanoid`: models/humanoid.xml, keyframe 0 in each of 8192 worlds, one forward,
the egocentric camera at 64 x 64, RGB without shadows.  Two contexts are made in one process, use_textures=False
(the launch of a build without textures, `mjw_render_bvh`) and use_textures=True (`mjw_render_tex`: the floor takes
its 512 x 512 checker).  They are timed alternately, one window each in turn: a window is 20 `render` calls after 5
warm-up calls between one pair of HIP events on the stream the kernels run on.  Reported per context: the median
ms per call over its windows, the least and the largest window (the spread), and every window; and the ratio of the
medians.  There is no CPU fallback: without a GPU this fails.
"""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NWORLD, W, H = 8192, 64, 64
WARMUP, CALLS = 5, 20


def window(fn, torch):
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


def run(windows):
  import numpy as np
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf

  if not torch.cuda.is_available():
    sys.exit("texture_bench: needs the ROCm device")
  mjm = mjcf.load_model(os.path.join(ROOT, "models", "humanoid.xml"))
  mjw.override_model(mjm, ["opt.solver=CG"])
  mjd = mjcf.MjData(mjm)
  mjcf.reset_data_keyframe(mjm, mjd, 0)
  m = mjw.put_model(mjm, device="cuda")
  d = mjw.put_data(mjm, mjd, nworld=NWORLD, nconmax=24, njmax=64, device="cuda", m=m)
  mjw.forward(m, d)
  torch.cuda.synchronize()
  cam = mjm.cam_names.index("egocentric")
  kw = dict(nworld=NWORLD, cam_res=(W, H), cam_active=[i == cam for i in range(mjm.ncam)], device="cuda", render_rgb=True, render_depth=False,
            render_seg=False)
  rcs = {False: mjw.create_render_context(mjm, use_textures=False, **kw), True: mjw.create_render_context(mjm, use_textures=True, **kw)}
  assert rcs[True].has_textures and not rcs[False].has_textures
  ms = {False: [], True: []}
  for _ in range(windows):
    for on in (False, True):
      ms[on].append(window(lambda: mjw.render(m, d, rcs[on]), torch))
  changed = float((rcs[True].rgb_data != rcs[False].rgb_data).float().mean())
  out = dict(config="humanoid", nworld=NWORLD, camera="egocentric", width=W, height=H, windows=windows, warmup=WARMUP, calls=CALLS,
             texels=int(rcs[True].tex_data.shape[0]), pixels_changed_by_textures=round(changed, 4))
  for on, key in ((False, "off"), (True, "on")):
    out[f"ms_textures_{key}"] = round(float(np.median(ms[on])), 5)
    out[f"ms_textures_{key}_min"], out[f"ms_textures_{key}_max"] = round(min(ms[on]), 5), round(max(ms[on]), 5)
    out[f"ms_textures_{key}_windows"] = [round(x, 5) for x in ms[on]]
  out["on_over_off"] = round(out["ms_textures_on"] / out["ms_textures_off"], 4)
  out["device"] = torch.cuda.get_device_name(0)
  return out


if __name__ == "__main__":
  n = int(sys.argv[sys.argv.index("--windows") + 1]) if "--windows" in sys.argv else 5
  print(json.dumps(run(n)), flush=True)
