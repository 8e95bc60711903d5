"""The driver's exact round-end bench command on the GPU (round 1 died on it).

Runs ``python bench.py --gpus 1 --steps 20 --warmup 5 --full`` as a child
process (with a 1-second CPU-baseline budget) and checks the JSON line: rc 0,
whole segments executed, ``roofline`` and ``cpu_baseline`` present, and the
timed steps fit in the wall time of the run. The plain command (no ``--full``)
times exactly the steps asked, measures nothing beside them, and with
``--dump-outputs`` writes the last step's arrays, the same from run to run.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_driver_bench_command():
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20",
                        "--warmup", "5", "--full", "--cpu-seconds", "1"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    # >= 8 timed segments, the warm-up past the clock boost, and the timed region lasts >= 1 s
    # (bench.MIN_TIMED_SECONDS, sized at the warm-up's post-boost rate)
    assert d["steps"] % 256 == 0 and d["steps"] >= 8 * 256 and d["n_gpus"] == 1
    assert d["warmup"] == 256 * 24
    assert d["ms_per_step"] * d["steps"] * 1e-3 >= 1.0
    assert d["value"] > 0 and d["unit"] == "env-steps/s"
    assert d["ms_per_step"] * d["steps"] * 1e-3 <= wall
    # every captured graph (4 action-table segments) ran once before the warm-up
    assert d["setup"]["graph_first_replays"] == 512
    rf = d["roofline"]
    # the persistent step is bound by FP64 instruction issue (PMC: profiles/*pmc_segment.json);
    # the byte figures stay beside it
    assert rf["bound"] == "fp64-issue" and rf["unit"] == "TFLOP/s" and 0 < rf["frac"] < 1
    assert 0 < rf["issue_floor_frac"] <= 1.05 and rf["kernel_avg_us"] > 0
    assert 0 < rf["hbm"]["frac"] < 1 and rf["hbm"]["unit"] == "GB/s"
    # the N>1 replay path at one GPU, measured on the same line, with the sampler it timed, and
    # the same with the collective's kernel stood in for
    rp, sd = d["replay_path"], d["replay_path_collective_standin"]
    assert rp["value"] > 0 and d["every_output"]["value"] > 0
    assert rp["sampler"] == "philox" and rp["exchange"] == "allgather"
    assert sd["value"] > 0 and sd["standin"]["workgroups"] == 16 and sd["standin"]["bytes"] > 20e6
    # one GPU as rank 0 of the 8-rank pooled buffer (the N = 8 line's per-rank work)
    rk = d["replay_path_rank_of_world"]
    assert rk["value"] > 0 and rk["world"] == 8 and 0 < rk["frac_of_value"] < 1.05
    assert 0 < rp["frac_of_value"] < 1.05
    if rf["kernel"].startswith("k_rollout"):  # the persistent launch: resident-state bytes headline
        assert abs(rf["bytes_per_env_step"] - (70 + 152 / 256)) < 1e-9
        assert rf["survey_222B"]["bytes_per_env_step"] == 222
    # the timed step includes its refill: never faster than the kernel alone
    assert rf["step_us_incl_refill"] >= rf["kernel_avg_us"]
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] == "port" and cb["one_core"] > 0
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        assert d["metric"] == json.load(f)["metric"]


def _dump_in_process(argv, path, gpu):
    """bench.py's default line in this process (make_workload + run_bench), dumping to path."""
    import bench
    args = bench.parse([*argv, "--dump-outputs", str(path)])
    out = bench.run_bench(args, 0, 1, gpu, bench.make_workload(args, 0, gpu))
    return out, {f[:-4]: np.load(os.path.join(path, f)) for f in out["outputs"]["files"]}


@pytest.mark.gpu
def test_plain_bench_command_is_lean_and_dumps_its_outputs(built_lib, gpu, tmp_path):
    """``bench.py --gpus 1 --steps 300 --warmup 5 --dump-outputs DIR`` (no --full): exactly 300
    timed steps (one whole segment + a 44-step launch), no side measurement, the headline
    fields as the full line has them, less than 30 s outside the steps, and the last step's
    arrays on disk -- bit for bit what a second run (in this process) writes."""
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "300",
                        "--warmup", "5", "--dump-outputs", str(tmp_path / "a")],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 300 and d["warmup"] == 256 * 24 and d["n_gpus"] == 1 and d["full"] is False
    assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] * 1e-3 / 65536 - 1) < 1e-9
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        assert d["metric"] == json.load(f)["metric"]
    for side in ("cpu_baseline", "every_output", "replay_path", "replay_path_collective_standin",
                 "replay_path_rank_of_world", "pooling"):
        assert d[side] is None, side
    # the kernel time comes from the timed region's own launches: the roofline stays
    assert d["roofline"]["bound"] == "fp64-issue" and d["roofline"]["kernel_avg_us"] > 0
    assert wall - (d["steps"] + d["warmup"]) * d["ms_per_step"] * 1e-3 < 30.0
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(d["outputs"]["files"]) and "boat_obs.npy" in files
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) == d["outputs"]["bytes"] <= 64 << 20
    assert got["boat_obs"].shape == (65536, 11) and got["boat_state_s_x"].dtype == np.float64
    # the run is past its transient: envs have ended and restarted, some in the last step
    assert got["boat_counters"].sum() > 0 and np.isfinite(got["boat_obs"]).all()
    out, again = _dump_in_process(["--gpus", "1", "--steps", "300", "--warmup", "5"], tmp_path / "b", gpu)
    assert out["steps"] == 300 and sorted(again) == sorted(got)
    for name in got:
        assert np.array_equal(got[name], again[name]), name


@pytest.mark.gpu
def test_plain_bench_short_launch_agrees_across_launch_modes(built_lib, gpu, tmp_path):
    """--steps 300 = one whole segment + 44 steps: the persistent launch's short segment, the
    graph mode's eager tail and the eager mode leave the same arrays (4 096 envs)."""
    base = ["--steps", "300", "--warmup", "5", "--envs", "4096"]
    outs = [_dump_in_process([*base, *extra], tmp_path / str(i), gpu)
            for i, extra in enumerate(([], ["--launch", "step"], ["--no-graph"]))]
    assert [o["steps"] for o, _ in outs] == [300] * 3
    assert outs[0][0]["roofline"] is not None and outs[2][0]["roofline"] is None   # (eager: --full times it)
    ref = outs[0][1]
    assert ref["boat_obs"].shape == (4096, 11) and (ref["boat_state_index"] > 0).any()
    for _, arrs in outs[1:]:
        assert sorted(arrs) == sorted(ref)
        for name in ref:
            assert np.array_equal(ref[name], arrs[name]), name


def _two_rank_env():
    return dict(os.environ, SACENV_BENCH_BACKEND="gloo", SACENV_BENCH_ONE_DEVICE="1")


@pytest.mark.gpu
def test_bench_two_ranks_gloo_on_one_device():
    """The N>1 bench path (the staged replay exchange of the kernel-written transition rows,
    max-over-ranks timing; the all-gather beside it) as two processes sharing the one GPU
    over gloo, under the launcher the driver uses (torch.distributed.run). RCCL needs one
    device per rank; the driver's 8-GPU run is the RCCL one."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--steps", "20", "--warmup", "5", "--full", "--envs", "8192"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=_two_rank_env())
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["steps"] % 256 == 0 and d["steps"] >= 8 * 256 and d["value"] > 0
    assert d["config"]["global_envs"] == 2 * 8192
    c = d["config"]["collective"]
    assert "gloo all_gather" in c and f"({d['steps'] // 256} in the timed region)" in c and "StagedReplay" in c
    po = d["pooling"]
    assert po["mode"] == "sharded" and po["exchanges_timed"] == d["steps"] // 256
    assert po["all_gather"]["value"] > 0 and po["no_exchange"]["value"] > 0


@pytest.mark.gpu
def test_bench_self_launch_two_ranks_on_one_device():
    """``python bench.py --gpus 2`` with no launcher: bench starts its own two ranks."""
    env = {k: v for k, v in _two_rank_env().items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20",
                        "--warmup", "5", "--full", "--envs", "4096", "--exchange-segs", "1"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["pooling"]["mode"] == "sharded" and d["value"] > 0


@pytest.mark.gpu
def test_bench_two_ranks_allreduce_exact_sampler():
    """The previous default, kept as options: the MT-exact draws and the SUM all-reduce."""
    env = {k: v for k, v in _two_rank_env().items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20",
                        "--warmup", "5", "--full", "--envs", "4096", "--exchange-segs", "1", "--sampler", "mt",
                        "--exchange", "allreduce"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["pooling"]["exchange"] == "allreduce" and "gloo SUM all_reduce" in d["config"]["collective"]
