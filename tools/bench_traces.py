"""Time the episode traces (sacenv_traces_update) beside what they are judged against.

    python tools/bench_traces.py [--reps 500] [--windows 5] [--example-iters 200] [--skip-example] [--out FILE]

Three shapes: 4 096 envs (4 members x 1 024) and 65 536 envs (64 x 1 024) with one step per
``update`` on the env's own record, and 65 536 envs with a rollout's 256 steps per ``update``
(``max_steps`` 500). Per shape, each timed between two device events over ``--reps`` calls (a
tenth of them for the 256-step shape), ``--windows`` windows, median / min / max:

* ``BestEpisodes.update``: both launches. The walk's bytes -- every step's obs block, action and
  reward read once and written once into the store (52 B each way per env and step), the done and
  term bytes read -- over that time is the rate reported; the pick launch (one workgroup per
  member) is inside the time, so the walk alone is no slower than this. Put against the HBM rate
  a copy reaches on this GPU (6.29 TB/s measured, 8 TB/s specified).
* ``EpisodeLog.update`` alone on the same records: the same walk over 6 of the record's 50 bytes
  (7 with its count launch), the floor the new unit is judged against; its bytes per second too.
* one step only: ``VecRecorder.record()`` + ``after_step()`` for 64 chosen envs, the only other way
  to a trajectory (its rows stay on the device; nothing is flushed inside the window).

The 256-step shape scans ``--buffers`` rollouts in turn, so that a call's records were not left in
the Infinity Cache by the call before. Then the example's ``ms_per_iter`` with and without
``--keep-traces`` at 16 x 1 024 envs, batch 256, alternating, twice each. The store's size at the
three shapes comes from ``sacenv_traces_bytes``. Prints one JSON line.
"""
from __future__ import annotations

import argparse
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sac-agent_amd"))

HBM_COPY_RATE = 6.29e12   # B/s, a float4 copy on the MI355X
SHAPES = ((4, 1024, 1, None), (64, 1024, 1, None), (64, 1024, 256, 500))   # members, envs per member, K, max_steps


def timed(fn, reps, windows, between=None):
    """us per call of fn(i): median, min, max over the windows"""
    times = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / reps * 1e3)
        if between is not None:
            between()
    return {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))}


def shape(P, N, K, max_steps, args):
    from sacenv import BestEpisodes, VecBoatEnv
    from sacenv.episodes import EpisodeLog
    from sacenv.recorder import VecRecorder
    dev = torch.device("cuda")
    n = P * N
    env = VecBoatEnv({"base_settings": {"experiment": 6, "test_mode": 0}}, n, seed=0, device=dev, max_episode_steps=500)
    env.reset()
    NP = env.n_pad
    traces = BestEpisodes(env, members=P, envs_per_member=N, max_steps=max_steps, call_steps=K, max_bytes=8 << 30)
    log = EpisodeLog(env, capacity=max(n * K // 2, 1 << 20))
    g = torch.Generator(device=dev).manual_seed(0)
    reps = args.reps if K == 1 else max(args.reps // 10, 1)
    out = {"members": P, "envs_per_member": N, "envs": n, "n_pad": NP, "steps_per_update": K, "max_steps": traces.R,
           "reps_per_window": reps, "store_bytes": int(traces.store.numel()), "member_bytes": int(traces.members.numel())}
    if K == 1:
        actions = torch.rand(n, device=dev, generator=g) * 2 - 1
        for _ in range(64):                      # past the first endings of the shortest episodes
            env.step(actions)
        up_traces = lambda i: traces.update(actions)          # noqa: E731
        up_log = lambda i: log.update()                       # noqa: E731
    else:
        actions = torch.rand(K, n, device=dev, generator=g) * 2 - 1
        bufs = []
        for _ in range(args.buffers):
            final = torch.empty((K, NP, 11), dtype=torch.float32, device=dev)
            bufs.append((env.rollout(actions, final_obs=final)[0], final))
        out["record_buffers"] = len(bufs)
        up_traces = lambda i: traces.update(actions, *bufs[i % len(bufs)])     # noqa: E731
        up_log = lambda i: log.update(bufs[i % len(bufs)][0])                   # noqa: E731
    for i in range(8):                           # warm-up: code objects, every buffer once
        up_traces(i)
        up_log(i)
    log.drain()
    t_tr = timed(up_traces, reps, args.windows)
    t_log = timed(up_log, reps, args.windows, between=log.drain)
    moved = (52 + 52 + 2) * K * NP               # the walk: read 54 B, write 52 B per env and step
    log_bytes = 7 * K * NP                       # the log: done (count) + reward, done, term (emit)
    out.update({
        "traces_update_us": t_tr, "episode_log_update_us": t_log, "log_dropped": int(log.dropped_total),
        "traces_over_log": t_tr["median"] / t_log["median"],
        "walk_bytes_per_update": moved, "appended_bytes_per_update": 52 * K * NP,
        "walk_bytes_per_s": moved / (t_tr["median"] * 1e-6),
        "appended_bytes_per_s": 52 * K * NP / (t_tr["median"] * 1e-6),
        "walk_share_of_hbm_copy_rate_6.29TBps": moved / (t_tr["median"] * 1e-6) / HBM_COPY_RATE,
        "episode_log_bytes_per_s": log_bytes / (t_log["median"] * 1e-6),
        "best_episodes": traces.table()[:4]})
    if K == 1:
        with tempfile.TemporaryDirectory() as d:
            rec = VecRecorder(env, list(range(0, n, n // 64))[:64], d, flush_steps=1 << 30)

            def record(i):
                rec.record()
                rec.after_step(actions)

            def forget():
                rec._rows, rec._events = [], []
            for i in range(8):
                record(i)
            forget()
            out["vec_recorder_64_envs_us"] = timed(record, reps, args.windows, between=forget)
    del traces, log, env
    torch.cuda.empty_cache()
    return out


def example(args):
    spec = importlib.util.spec_from_file_location("train_population", os.path.join(ROOT, "examples", "train_population.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--members", "16", "--envs-per-member", "1024", "--batch", "256", "--iters", str(args.example_iters)]
    ms = {"plain": [], "keep_traces": []}
    with tempfile.TemporaryDirectory() as d:
        for _ in range(2):
            for name, extra in (("plain", []), ("keep_traces", ["--keep-traces", d])):
                torch.manual_seed(0)
                with contextlib.redirect_stdout(io.StringIO()):
                    ms[name].append(mod.main(base + extra)["ms_per_iter"])
    return {"members": 16, "envs_per_member": 1024, "batch": 256, "iters": args.example_iters, "ms_per_iter": ms,
            "overhead_ms_per_iter": float(np.mean(ms["keep_traces"]) - np.mean(ms["plain"]))}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=3)
    ap.add_argument("--example-iters", type=int, default=200)
    ap.add_argument("--skip-example", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    out = {"what": "sacenv_traces_update (walk + pick launches) beside sacenv_episodes_update and VecRecorder",
           "shapes": [shape(*s, args) for s in SHAPES]}
    if not args.skip_example:
        out["example"] = example(args)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
