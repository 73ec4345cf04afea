"""Measures mjw.transition_fd on the device: accuracy over eps and time.  One JSON line per configuration.

  python tools/fd_bench.py [accuracy_squat] [accuracy_contact] [time_humanoid] [time_franka]      (default: all four)

Each configuration runs in a child process of its own under a time limit, and the tool ends at the first one that
fails or runs out of time (nothing more is started on the device after a failure).

accuracy_*   The humanoid, 64 worlds, centred, CG solver.  `squat`: every world at the squat key with seeded noise on
             the joint angles and velocities and the root lifted 0.05 m (the key itself already touches the floor), so
             before ground contact; `contact`: the same worlds, not lifted, advanced 400 steps: settled on the
             floor.  The JSON line says how many constraint rows the nominal worlds have.  The reference is the same
             finite difference (tests/fd_ref.py) over the fp64 CPU oracle at eps = 1e-6, from the float32 state and
             qacc_warmstart of the device Data, its solver run to tolerance 1e-14 (500 iterations at the most) so that
             the solver's own tolerance over 1e-6 is not what is measured; `ref_self_*` is that reference against itself at eps = 1e-5, which
             says how far the reference can be trusted (in contact a nudge can switch rows on and off, and no finite
             difference is then well defined); a world whose reference agrees with itself to 1e-5 in every entry is
             `smooth`.  For eps = 2^-4 .. 2^-14 the line gives the maximum, the 99th percentile and the median of
             |A - A_ref| and |B - B_ref| over all worlds and entries, the same over the smooth worlds, and `best`:
             the eps of the smallest 99th percentile over the smooth worlds (over all worlds if none is smooth).  The
             maximum is not used for that: it belongs to entries where a nudge of the device's size crosses a joint
             limit or a contact's margin that the reference's 1e-6 does not reach.
time_*       humanoid and franka, 64 worlds, centred, one pass.  A window is REPS calls of transition_fd with events
             between its three parts; per part the window's time is the sum over its calls.  WINDOWS windows after
             WARMUP warm-up calls; reported are the medians over the windows, per call, in ms: perturb, step,
             difference, their sum, `call_ms`: the host clock around REPS calls without inner events, ended by a
             synchronise, and `graph_call_ms`: the same around REPS replays of one call captured in a graph, which
             leaves the host's launch work out (where the parts' sum is near call_ms and far above graph_call_ms, the
             parts were waiting for the host, not running).  `plain_step_ms` is mjw.step alone on a Data of the same number of worlds (the context's
             scratch Data after a perturbation), REPS consecutive steps per window, so that the step share can be
             compared with a commit that has no transition_fd.  `*_gbps`: the bytes each kernel has to move (perturb:
             every slot's rows written once and the worlds' rows read once; difference: two slots read per column, A..D
             written once) over its time.  There is no CPU fallback: without a GPU this fails.
"""

import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NWORLD = 64
EXPONENTS = list(range(4, 15))
WARMUP, WINDOWS, REPS = 5, 7, 20
REF_TOLERANCE, REF_ITERATIONS = 1e-14, 500
SMOOTH = 1e-5  # a world is smooth if its fp64 reference at eps = 1e-6 and at 1e-5 agree to this in every entry
CONFIGS = {
  "accuracy_squat": dict(kind="accuracy", settle=0, lift=0.05, limit_s=400),
  "accuracy_contact": dict(kind="accuracy", settle=400, lift=0.0, limit_s=400),
  "time_humanoid": dict(kind="time", path="models/humanoid.xml", solver="CG", nconmax=24, njmax=64, settle=100, limit_s=240),
  "time_franka": dict(kind="time", path="models/franka_emika_panda/scene.xml", solver=None, nconmax=None, njmax=None, settle=0, limit_s=240),
}


def _load(path, solver, settle, noise_seed=None, nconmax=None, njmax=None, lift=0.0):
  import torch

  import mujoco_warp_amd as mjw
  from mujoco_warp_amd import mjcf

  mjm = mjcf.load_model(os.path.join(ROOT, path))
  if solver:
    mjw.override_model(mjm, [f"opt.solver={solver}"])
  mjd = mjcf.MjData(mjm)
  if len(getattr(mjm, "key_qpos", [])):
    mjcf.reset_data_keyframe(mjm, mjd, 0)
  m = mjw.put_model(mjm, device="cuda")
  d = mjw.put_data(mjm, mjd, nworld=NWORLD, nconmax=nconmax, njmax=njmax, device="cuda", m=m)
  if noise_seed is not None:  # humanoid: joint angles past the free joint, and all velocities
    rng = np.random.default_rng(noise_seed)
    d.qpos[:, 7:] += torch.as_tensor(rng.normal(0, 0.05, (NWORLD, mjm.nq - 7)), dtype=torch.float32, device="cuda")
    d.qvel[:] = torch.as_tensor(rng.normal(0, 0.1, (NWORLD, mjm.nv)), dtype=torch.float32, device="cuda")
  if lift:
    d.qpos[:, 2] += lift
  for _ in range(settle):
    mjw.step(m, d)
  torch.cuda.synchronize()
  return mjw, mjm, m, d


def run_accuracy(name):
  import torch

  from tests import fd_ref as fr

  cfg = CONFIGS[name]
  mjw, mjm, m, d = _load("models/humanoid.xml", "CG", cfg["settle"], noise_seed=0, nconmax=24, njmax=64, lift=cfg["lift"])
  ndx, nu = 2 * mjm.nv + mjm.na, mjm.nu
  ctx = mjw.make_fd_context(mjm, m, NWORLD, nconmax=24, njmax=64)
  A = torch.empty((NWORLD, ndx, ndx), device="cuda")
  B = torch.empty((NWORLD, ndx, nu), device="cuda")
  host = {n: getattr(d, n).double().cpu().numpy() for n in ("qpos", "qvel", "act", "ctrl", "qacc_warmstart")}
  t0 = time.time()
  Aref, Bref = np.zeros((NWORLD, ndx, ndx)), np.zeros((NWORLD, ndx, nu))
  selfA, selfB = [], []
  nefc, base = [], {}
  # the reference's solver runs to fp64 convergence, so that its own tolerance over 1e-6 is not what is measured
  from mujoco_warp_amd import mjcf

  mjm_ref = mjcf.load_model(os.path.join(ROOT, "models/humanoid.xml"))
  mjw.override_model(mjm_ref, ["opt.solver=CG"])
  mjm_ref.opt.tolerance, mjm_ref.opt.iterations, mjm_ref.opt.ls_iterations = REF_TOLERANCE, REF_ITERATIONS, REF_ITERATIONS
  stepfn = fr.oracle_stepfn(mjm_ref, njmax=128, nconmax=64, base=base, nefc_out=nefc, nthread=8)
  for w in range(NWORLD):
    base["qacc_warmstart"] = host["qacc_warmstart"][w]
    x = {n: host[n][w] for n in ("qpos", "qvel", "act", "ctrl")}
    Aref[w], Bref[w], _, _ = fr.transition(mjm, stepfn, x, 1e-6, True)
    A5, B5, _, _ = fr.transition(mjm, stepfn, x, 1e-5, True)
    selfA.append(np.abs(A5 - Aref[w]))
    selfB.append(np.abs(B5 - Bref[w]))
  out = dict(config=name, model="humanoid", nworld=NWORLD, centered=True, settle=cfg["settle"], ref_eps=1e-6, ref_tolerance=REF_TOLERANCE, ref_iterations=REF_ITERATIONS, ref_seconds=round(time.time() - t0, 1),
             nefc_nominal_min=int(min(nefc[::2])), nefc_nominal_max=int(max(nefc[::2])), A_ref_absmax=float(np.abs(Aref).max()), B_ref_absmax=float(np.abs(Bref).max()),
             ref_self_A_max=float(f"{np.max(selfA):.3e}"), ref_self_A_median=float(f"{np.median(selfA):.3e}"),
             ref_self_B_max=float(f"{np.max(selfB):.3e}"), ref_self_B_median=float(f"{np.median(selfB):.3e}"), sweep=[])
  smooth = np.array([max(a.max(), b.max()) < SMOOTH for a, b in zip(selfA, selfB)])
  out["smooth_worlds"] = int(smooth.sum())
  stats = lambda e: dict(max=float(f"{e.max():.3e}"), p99=float(f"{np.percentile(e, 99):.3e}"), median=float(f"{np.median(e):.3e}"))  # noqa: E731
  for e in EXPONENTS:
    mjw.transition_fd(m, d, 2.0**-e, True, A, B, ctx=ctx)
    torch.cuda.synchronize()
    ea, eb = np.abs(A.double().cpu().numpy() - Aref), np.abs(B.double().cpu().numpy() - Bref)
    row = dict(eps=f"2^-{e}", A=stats(ea), B=stats(eb))
    if smooth.any():
      row.update(A_smooth=stats(ea[smooth]), B_smooth=stats(eb[smooth]))
    out["sweep"].append(row)
  key = "_smooth" if smooth.any() else ""
  out["best"] = dict(min(out["sweep"], key=lambda r: max(r["A" + key]["p99"], r["B" + key]["p99"])), by="p99", over="smooth worlds" if key else "all worlds")
  out["device"] = torch.cuda.get_device_name(0)
  return out


def run_time(name):
  import torch

  cfg = CONFIGS[name]
  mjw, mjm, m, d = _load(cfg["path"], cfg["solver"], cfg["settle"], nconmax=cfg["nconmax"], njmax=cfg["njmax"])
  ndx, nu, ns = 2 * mjm.nv + mjm.na, mjm.nu, mjm.nsensordata
  ctx = mjw.make_fd_context(mjm, m, NWORLD, nconmax=cfg["nconmax"], njmax=cfg["njmax"])
  A, B = torch.empty((NWORLD, ndx, ndx), device="cuda"), torch.empty((NWORLD, ndx, nu), device="cuda")
  C, D = torch.empty((NWORLD, ns, ndx), device="cuda"), torch.empty((NWORLD, ns, nu), device="cuda")
  eps = 2.0**-9
  for _ in range(WARMUP):
    mjw.transition_fd(m, d, eps, True, A, B, C, D, ctx=ctx)
  torch.cuda.synchronize()
  parts = {k: [] for k in ("perturb", "step", "difference")}
  call, plain = [], []
  ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(REPS)]
  for _ in range(WINDOWS):
    for e in ev:
      e[0].record()
      mjw.fd_perturb(m, d, ctx, eps)
      e[1].record()
      mjw.step(m, ctx.data)
      e[2].record()
      mjw.fd_difference(m, d, ctx, eps, A, B, C, D)
      e[3].record()
    torch.cuda.synchronize()
    for i, k in enumerate(parts):
      parts[k].append(sum(e[i].elapsed_time(e[i + 1]) for e in ev) / REPS)
    t0 = time.perf_counter()
    for _ in range(REPS):
      mjw.transition_fd(m, d, eps, True, A, B, C, D, ctx=ctx)
    torch.cuda.synchronize()
    call.append((time.perf_counter() - t0) * 1e3 / REPS)
    mjw.fd_perturb(m, d, ctx, eps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
      mjw.step(m, ctx.data)
    torch.cuda.synchronize()
    plain.append((time.perf_counter() - t0) * 1e3 / REPS)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    mjw.transition_fd(m, d, eps, True, A, B, C, D, ctx=ctx)
  torch.cuda.synchronize()
  replay = []
  for _ in range(WINDOWS):
    t0 = time.perf_counter()
    for _ in range(REPS):
      graph.replay()
    torch.cuda.synchronize()
    replay.append((time.perf_counter() - t0) * 1e3 / REPS)
  med = {k: float(np.median(v)) for k, v in parts.items()}
  nslot = ctx.ncol_pass * NWORLD
  row = 1 + mjm.nq + 3 * mjm.nv + mjm.na + mjm.nu + 6 * mjm.nbody + 7 * mjm.nmocap + mjm.neq  # words a slot receives
  perturb_bytes = 4 * row * (nslot + NWORLD)
  diff_bytes = 4 * NWORLD * ctx.ncol * (2 * (mjm.nq + mjm.nv + mjm.na + ns) + ndx + ns)
  out = dict(config=name, nworld=NWORLD, centered=True, nv=int(mjm.nv), na=int(mjm.na), nu=int(nu), nsensordata=int(ns), ncol=ctx.ncol,
             scratch_worlds=nslot, sparse=bool(m.is_sparse),
             perturb_ms=round(med["perturb"], 5), step_ms=round(med["step"], 5), difference_ms=round(med["difference"], 5),
             parts_sum_ms=round(sum(med.values()), 5), call_ms=round(float(np.median(call)), 5), graph_call_ms=round(float(np.median(replay)), 5), plain_step_ms=round(float(np.median(plain)), 5),
             frame_over_step=round((med["perturb"] + med["difference"]) / med["step"], 4),
             perturb_bytes=perturb_bytes, difference_bytes=diff_bytes,
             perturb_gbps=round(perturb_bytes / med["perturb"] / 1e6, 2), difference_gbps=round(diff_bytes / med["difference"] / 1e6, 2),
             world_steps_per_s=round(nslot / med["step"] * 1e3), warmup=WARMUP, windows=WINDOWS, reps=REPS, device=torch.cuda.get_device_name(0))
  return out


if __name__ == "__main__":
  if len(sys.argv) == 3 and sys.argv[1] == "--one":
    kind = CONFIGS[sys.argv[2]]["kind"]
    print(json.dumps((run_accuracy if kind == "accuracy" else run_time)(sys.argv[2])), flush=True)
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
