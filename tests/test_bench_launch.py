"""bench.py as the driver runs it: `--gpus N` starts N ranks itself (one process per GPU, gloo barrier,
no collective on the data path), weak and strong sharding, hipGraph replay.

On the 1-GPU box the two ranks share the device round-robin; each rank's final qpos must equal the
matching world range of a single-process run of the same global worlds (ctrl noise is indexed by global
world id through world_offset)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, timeout=240):
  env = dict(os.environ)
  env.pop("WORLD_SIZE", None)
  env.pop("RANK", None)
  env.pop("LOCAL_RANK", None)
  out = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
  assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
  lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
  assert len(lines) == 1, out.stdout
  return json.loads(lines[0])


def test_launcher_command_without_gpu(monkeypatch):
  """`--gpus 2` with no WORLD_SIZE re-launches itself through torch.distributed.run (parent never touches HIP)."""
  sys.path.insert(0, ROOT)
  import bench

  seen = {}

  def fake_call(cmd, env=None):
    seen["cmd"], seen["env"] = cmd, env
    return 0

  monkeypatch.setattr(subprocess, "call", fake_call)
  monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "3"])
  assert bench.launch_ranks(2) == 0
  cmd = seen["cmd"]
  assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=2" in cmd
  assert "127.0.0.1" in cmd and cmd[-4:] == ["--gpus", "2", "--steps", "3"]
  assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


@pytest.mark.gpu
@pytest.mark.parametrize("model,per_rank", [("humanoid", 256), ("apollo", 64)])
def test_gpu_bench_two_ranks_weak_equals_single(tmp_path, model, per_rank):
  """C2 and C4 (apollo: Newton, sensors, box-box CCD) sharded over two ranks: each rank's worlds
  bitwise equal to the same global worlds of one 2 x per_rank run."""
  common = ["--model", model, "--steps", "5", "--warmup", "2", "--cpu-baseline", "0", "--graph", "0"]
  two = _run(["--gpus", "2", "--nworld", str(per_rank), "--dump-qpos", str(tmp_path / "two")] + common)
  assert two["n_gpus"] == 2 and two["scaling"] == "weak"
  assert two["config"]["nworld_total"] == 2 * per_rank and two["config"]["converged_worlds"] == 2 * per_rank
  one = _run(["--gpus", "1", "--nworld", str(2 * per_rank), "--dump-qpos", str(tmp_path / "one")] + common)
  assert one["n_gpus"] == 1
  q1 = np.load(tmp_path / "one" / "qpos_rank0.npz")["qpos"]
  for r in range(2):
    z = np.load(tmp_path / "two" / f"qpos_rank{r}.npz")
    off = int(z["offset"])
    assert off == per_rank * r
    np.testing.assert_array_equal(z["qpos"], q1[off:off + per_rank])


@pytest.mark.gpu
def test_gpu_bench_two_ranks_strong_and_graph(tmp_path):
  common = ["--full", "--steps", "5", "--warmup", "2", "--cpu-baseline", "0", "--nworld", "301", "--trace-steps", "2"]
  strong = _run(["--gpus", "2", "--scaling", "strong", "--graph", "0", "--dump-qpos", str(tmp_path / "s")] + common)
  assert strong["scaling"] == "strong" and strong["config"]["nworld_total"] == 301
  # graph replay over two stream shards of one rank: the timed region is replays only, the kernel times
  # come from the 2-step eager trace pass after it (same number of steps as the strong run's)
  graph = _run(["--gpus", "1", "--graph", "1", "--streams", "2", "--dump-qpos", str(tmp_path / "g")] + common)
  assert graph["config"]["graph"] is True and graph["config"]["streams"] == 2
  assert graph["config"]["timed_region"] == "graph replays only" and graph["config"]["trace_steps"] == 2
  qg = np.load(tmp_path / "g" / "qpos_rank0.npz")["qpos"]
  got = [np.load(tmp_path / "s" / f"qpos_rank{r}.npz") for r in range(2)]
  assert [int(z["offset"]) for z in got] == [0, 151]
  np.testing.assert_array_equal(np.concatenate([z["qpos"] for z in got]), qg)


@pytest.mark.gpu
def test_gpu_bench_plain_run_and_dump_outputs(tmp_path):
  """A plain run times its steps and reports the headline only (no trace pass, roofline or CPU baseline);
  --dump-outputs writes the last timed step's Data arrays as float32, the same from run to run."""
  args = ["--gpus", "1", "--nworld", "70", "--steps", "3", "--warmup", "2"]
  runs = [_run(args + ["--dump-outputs", str(tmp_path / tag)]) for tag in ("a", "b")]
  rec = runs[0]
  assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["dtype"] == "fp32" and rec["higher_is_better"] is True
  assert abs(rec["value"] - 70 * 1e3 / rec["ms_per_step"]) <= 1e-6 * rec["value"]
  assert rec["roofline"] is None and rec["cpu_baseline"] is None and rec["config"]["full"] is False
  assert "trace_steps" not in rec["config"] and rec["config"]["converged_worlds"] == 70
  names = sorted(os.listdir(tmp_path / "a"))
  assert names == sorted(os.listdir(tmp_path / "b")) and {"qpos.npy", "qvel.npy", "qacc.npy", "xpos.npy", "nefc.npy"} <= set(names)
  total = 0
  for n in names:
    a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
    assert a.dtype == np.float32 and a.shape[0] == 70 and np.isfinite(a).all(), n
    np.testing.assert_array_equal(a, b, err_msg=n)
    total += a.nbytes
  assert 0 < total <= 64 * 2**20
  q = np.load(tmp_path / "a" / "qpos.npy")
  assert q.shape == (70, 28) and np.abs(q[0] - q[1]).max() > 0  # the ctrl noise differs per world: the steps ran


def test_dump_outputs_samples_a_fixed_set_of_worlds(tmp_path, monkeypatch):
  """Above the byte budget every array keeps the same seeded sample of worlds, in world order."""
  import types

  import torch

  sys.path.insert(0, ROOT)
  import bench

  def shard(lo, n):
    ids = torch.arange(lo, lo + n, dtype=torch.float32)
    d = types.SimpleNamespace(nworld=n)
    for name in bench.DUMP_FIELDS:
      setattr(d, name, torch.zeros(n, 0))
    d.qpos = ids[:, None] * torch.ones(1, 5)
    d.xpos = ids[:, None, None] * torch.ones(1, 2, 3)
    d.nefc = ids.to(torch.int32)
    return d

  shards = [shard(0, 60), shard(60, 40)]
  per_world = 4 * (5 + 6 + 1)
  monkeypatch.setattr(bench, "DUMP_BYTES", 25 * per_world + 7)
  for tag in ("a", "b"):
    bench.dump_outputs(str(tmp_path / tag), shards, 0, 1)
  assert sorted(os.listdir(tmp_path / "a")) == ["nefc.npy", "qpos.npy", "xpos.npy"]  # empty fields are not written
  got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("qpos", "xpos", "nefc")}
  assert all(v.dtype == np.float32 for v in got.values())
  assert got["qpos"].shape == (25, 5) and got["xpos"].shape == (25, 2, 3) and got["nefc"].shape == (25,)
  assert sum(v.nbytes for v in got.values()) <= 25 * per_world + 7
  ids = got["nefc"]
  assert (np.diff(ids) > 0).all() and ids.max() >= 60  # sorted, distinct, drawn over both shards
  assert (got["qpos"] == ids[:, None]).all() and (got["xpos"] == ids[:, None, None]).all()
  for n in got:
    np.testing.assert_array_equal(got[n], np.load(tmp_path / "b" / f"{n}.npy"))
  # within the budget every world is kept; other ranks write under their own names
  monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 100 * per_world)
  bench.dump_outputs(str(tmp_path / "c"), shards, 1, 2)
  assert np.load(tmp_path / "c" / "qpos_rank1.npy").shape == (100, 5)


def test_pmc_traffic_is_bound_to_the_kernel_sources(tmp_path):
  """bench.py reports `roofline.traffic` only from a PMC summary of the same workload taken on a build of
  the current kernel sources (csrc_sha == build.sources_hash())."""
  sys.path.insert(0, ROOT)
  import bench
  from mujoco_warp_amd import build

  pmc = {"nworld": 8192, "solver": "CG", "model": "humanoid", "csrc_sha": build.sources_hash(),
         "kernels": {"mjw::dense_kernel<7, false>": {"hbm_bytes_per_launch": 123.0, "hbm_bytes_per_step": 123.0, "launches_per_step": 1.0}}}
  f = tmp_path / "pmc_humanoid_r99.json"
  f.write_text(json.dumps(pmc))
  assert bench.pmc_traffic(str(f), "humanoid", 8192, "CG")[0]["mjw::dense_kernel<7, false>"]["bytes_per_launch"] == 123.0
  assert bench.pmc_traffic(str(f), "humanoid", 4096, "CG")[0] is None  # other workload
  pmc["csrc_sha"] = "0" * 16
  f.write_text(json.dumps(pmc))
  traffic, why = bench.pmc_traffic(str(f), "humanoid", 8192, "CG")
  assert traffic is None and "predates" in why
  assert bench.pmc_traffic(str(tmp_path / "missing.json"), "humanoid", 8192, "CG")[0] is None


def test_pmc_traffic_ratio_uses_the_pmc_window(tmp_path):
  """traffic_over_alg divides the PMC bytes by the algorithmic bytes at the counted window's own nefc / ncon
  (tools/pmc_traffic.py records them from the PMC passes' bench lines), not at the trace pass's."""
  sys.path.insert(0, ROOT)
  import bench
  from mujoco_warp_amd import build

  k = "mjw::mjw_kernel<79, false, false>"
  pmc = {"nworld": 8, "solver": "CG", "model": "humanoid", "csrc_sha": build.sources_hash(),
         "window": {"fetch": {"nefc_mean": 10.0, "ncon_mean": 2.0}},
         "kernels": {k: {"hbm_bytes_per_launch": 8000.0, "hbm_bytes_per_step": 8000.0, "launches_per_step": 1.0}}}
  f = tmp_path / "pmc_humanoid_r99.json"
  f.write_text(json.dumps(pmc))
  traffic, src = bench.pmc_traffic(str(f), "humanoid", 8, "CG")
  tab = {k: {"ms_per_step": 1.0, "launches_per_step": 1.0, "group": "forward"}}
  alg_at = lambda ne, nc: {"forward": 100.0 * ne + nc}
  rec = bench.roofline_record(tab, alg_at(30.0, 5.0), 8, traffic, src, alg_at)
  assert rec["groups"]["forward"]["traffic_over_alg"] == 8000.0 / (8 * 1002.0)
  assert rec["groups"]["forward"]["alg_bytes_per_env_step"] == 3005.0
