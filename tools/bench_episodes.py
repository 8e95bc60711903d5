"""Time the episode scan (sacenv_episodes_update) on a rollout's records.

    python tools/bench_episodes.py [--envs 65536] [--steps 256] [--reps 200] [--out FILE]

One rollout of ``--steps`` steps over ``--envs`` boat envs (experiment 6, U(-1, 1)
actions, max_episode_steps 500) gives the records; the scan of those same records is
then timed ``--reps`` times between two device events (the log drained of its count
between windows, the carry left to run on: the work per call does not depend on it).
``--buffers`` consecutive rollouts are kept and scanned in turn, so that the columns a
call reads (117 MB at the default size) were not left in the 256 MB Infinity Cache by
the call before.
Beside the time, the bytes the scan has to move -- the done column once (count launch),
reward + done + term once (emit launch), 16 B of counts and their scan per step and 64
envs -- and the time those bytes take at the HBM rate a copy reaches on this GPU
(6.29 TB/s measured, 8 TB/s specified). Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sac-agent_amd"))

HBM_COPY_RATE = 6.29e12   # B/s, a float4 copy on the MI355X


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from sacenv import VecBoatEnv
    from sacenv.episodes import EpisodeLog
    dev = torch.device("cuda")
    N, K = args.envs, args.steps
    env = VecBoatEnv({"base_settings": {"experiment": 6, "test_mode": 0}}, N, seed=0, device=dev,
                     max_episode_steps=500)
    log = EpisodeLog(env, capacity=N * K // 2)    # (no window overflows it: nothing dropped)
    g = torch.Generator(device=dev).manual_seed(0)
    actions = torch.rand(K, N, device=dev, generator=g) * 2 - 1
    rollouts = [env.rollout(actions)[0] for _ in range(args.buffers)]
    log.update(rollouts[0])
    first = log.drain()
    for i in range(2 * args.buffers):         # warm-up
        log.update(rollouts[i % args.buffers])
    log.drain()
    times = []
    for _ in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.reps):
            log.update(rollouts[i % args.buffers])
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / args.reps * 1e3)
        log.drain()
    NP = env.n_pad
    nbytes = (1 + 6) * K * NP + 2 * 16 * K * (NP // 64) + 32 * len(first)
    out = {"what": "sacenv_episodes_update on one rollout's records (count + scan + emit launches)",
           "envs": N, "n_pad": NP, "steps": K, "episodes_in_the_records": int(len(first)),
           "dropped": int(log.dropped), "reps_per_window": args.reps, "record_buffers": args.buffers,
           "us_per_call": {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))},
           "bytes_per_call": int(nbytes),
           "hbm_floor_us_at_6.29TBps": nbytes / HBM_COPY_RATE * 1e6,
           "two_passes_over_6B_floor_us": 2 * 6 * K * NP / HBM_COPY_RATE * 1e6,
           "env_steps_scanned_per_s": N * K / (float(np.median(times)) * 1e-6)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
