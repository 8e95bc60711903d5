"""Time one round of population selection: ``PopulationSelection.select`` against the host-side
path a user had before it.

    python tools/bench_selection.py [--runs 5] [--calls 200] [--out profiles/selection_bench.json]

Per P in ``--members`` (16 and 64), with q = P / 4, on the real slab of a 256-wide agent (batch
256) and a board written by hand in which every member is ready at every call (the members'
``episodes`` move on by one between calls -- one small launch, ``bump``, part of both sides and
timed alone too -- so every call replaces q members, as the first round of a run does):

* ``device``: ``select()``: the decision launch and the copy launch, nothing read back;
* ``host``: what a user did before: ``board.records()`` (a synchronise and a copy to the host), a
  numpy rank, q draws and one ``weights[l].copy_(weights[w])`` per loser;
* ``decide``: ``select()`` of a selection for which nobody is ever ready: the decision launch and
  a copy launch whose workgroups all exit at once.

HIP events around windows of ``--calls`` calls after a warm-up, the sides alternating ``--runs``
times (the method of tools/bench_population.py), and beside the times the bytes one call moves
(q x member_floats x 4 read and the same written). These are times per CALL in a stream of
calls: three small launches per call keep the host busier than the device (``bump`` alone costs
what the host needs to enqueue one launch), so ``device - decide`` is NOT the copy kernel's time.
That comes from a kernel trace, taken in a run of its own and added to the same JSON:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- \\
        python tools/bench_selection.py --sides device --runs 1 --out /dev/null
    python tools/bench_selection.py --kernel-trace DIR

``kernel_trace`` then holds the decision launch's and, per P, the copy launch's median time and
the copy's share of the HBM peak, (read + written) / time / 8 TB/s. At P = 16 all slabs together
(95 MB) fit the 256 MiB Infinity Cache, so there the peak is not a bound the copy has to respect.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sac-agent_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_population import configs, window  # noqa: E402

HBM_PEAK = 8.0e12       # bytes / s (MI355X, spec)
LOOKBACK = 5


def hand_board(dev, pop, P):
    """A ``MemberScoreboard`` (no snapshot) whose members hold distinct means and one episode."""
    from sacenv import MemberScoreboard
    from sacenv.scoreboard import MEMBER_DTYPE
    log = types.SimpleNamespace(device=dev, env_base=0, capacity=64, watchers=[], term_names=(),
                                log=torch.zeros(32 + 32 * 64, dtype=torch.uint8, device=dev))
    board = MemberScoreboard(log, P, 64, lookback=LOOKBACK)
    raw = board.board.cpu().numpy().copy()
    rec = raw[32: 32 + 128 * P].view(MEMBER_DTYPE)
    rec["episodes"] = 1
    rec["avg"] = np.random.default_rng(P).permutation(P).astype(np.float64)
    board.board.copy_(torch.from_numpy(raw))
    # the members' `episodes` as a strided view: bump() makes every member ready again
    episodes = board.board[32: 32 + 128 * P].view(torch.int64).view(P, 16)[:, 0]
    return board, episodes


def member_floats():
    """The real slab's floats per member (a host computation)."""
    from sacenv import _lib
    p = _lib.SacParams(obs_dim=11, n_actions=1, hidden=_lib.SAC_HIDDEN, batch=256, max_action=1.0, gamma=0.99,
                       tau=0.005, reward_scale=2.0, lr_actor=3e-4, lr_critic=3e-4, adam_beta1=0.9,
                       adam_beta2=0.999, adam_eps=1e-8)
    return int(_lib.sac_pop_layout(p, 2).member_floats)


def trace_summary(trace_dir, members):
    """The two launches' times from a rocprofv3 kernel trace of a ``--sides device`` run (every
    copy launch in it replaces q members): median, min and max over the dispatches, in µs, and
    per P the copy's bytes over its median time against the HBM peak."""
    import csv
    import glob
    import statistics
    from sacenv import _lib
    mf = member_floats()
    per = _lib.SELECT_COPY_THREADS * _lib.SELECT_COPY_UNROLL
    chunks = min(-(-(mf // 4) // per), _lib.SELECT_COPY_CHUNKS)
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for f in files for r in csv.DictReader(open(f))]

    def stats(mine):
        us = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine)
        return {"dispatches": len(us), "median_us": statistics.median(us), "min_us": us[0], "max_us": us[-1]}

    def items(r):     # a dispatch's work-items
        return int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) if "Grid_Size_X" in r else int(r["Grid_Size"])

    out = {"member_floats": mf, "copy_chunks": chunks,
           "k_select_decide": stats([r for r in rows if "k_select_decide" in r["Kernel_Name"]]), "copy": []}
    for P in members:     # the copy grid is (chunks, P) workgroups: P tells the cells apart
        q = P // 4
        mine = [r for r in rows if "k_select_copy" in r["Kernel_Name"]
                and items(r) == chunks * _lib.SELECT_COPY_THREADS * P]
        cell = {"P": P, "q": q, "bytes_read": q * mf * 4, "bytes_written": q * mf * 4, **stats(mine)}
        rate = 2 * q * mf * 4 / (cell["median_us"] * 1e-6)
        cell.update(bytes_per_s=rate, share_of_hbm_peak=rate / HBM_PEAK)
        out["copy"].append(cell)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", default="device,host,decide,bump", help="which sides to run (a profiler run: device)")
    ap.add_argument("--kernel-trace", default=None, metavar="DIR",
                    help="no run: add the kernel times of a rocprofv3 --kernel-trace of a `--sides device` run "
                         "(its output directory) to the JSON at --out")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window (>= 100)")
    ap.add_argument("--members", default="16,64")
    ap.add_argument("--warmup", type=float, default=3.0, help="seconds of work before the first window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selection_bench.json"))
    args = ap.parse_args(argv)
    if args.calls < 100:
        raise SystemExit("--calls must be at least 100")
    members = [int(x) for x in args.members.split(",")]
    if args.kernel_trace:
        with open(args.out) as f:
            result = json.load(f)
        result["kernel_trace"] = trace_summary(args.kernel_trace, members)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result["kernel_trace"]))
        return result
    from sacenv import _lib
    from sacenv.population import NativeSACPopulation
    from sacenv.selection import PopulationSelection
    dev = torch.device("cuda:0")
    cells = []
    for P in members:
        q = P // 4
        pop = NativeSACPopulation(dev, configs(P, 256), init_seeds=list(range(P)), with_memory=False)
        mf = int(pop.pop_layout.member_floats)
        board, episodes = hand_board(dev, pop, P)
        selection = PopulationSelection(board, pop, quantile=q, min_episodes=1, seed=1)
        idle = PopulationSelection(board, pop, quantile=q, min_episodes=1 << 40, seed=1)
        rng = np.random.default_rng(0)
        weights = pop.weights

        def bump():
            episodes.add_(1)

        def device():
            bump()
            selection.select()

        def decide():
            bump()
            idle.select()

        def host():
            bump()
            rec = board.records()
            order = np.argsort(-rec["avg"], kind="stable")
            for l, j in zip(order[P - q:], rng.integers(0, q, q)):
                weights[int(l)].copy_(weights[int(order[j])])

        sides = {"device": device, "host": host, "decide": decide, "bump": bump}
        sides = {k: sides[k] for k in args.sides.split(",")}
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.warmup:     # past the clock boost, every path loaded
            for fn in sides.values():
                window(fn, 20)
        ms = {k: [] for k in sides}
        for _ in range(args.runs):
            for k, fn in sides.items():
                ms[k].append(window(fn, args.calls))
        if "device" in sides:
            assert selection.header()["replaced_total"] >= q * args.calls * args.runs
        assert idle.header()["replaced_total"] == 0
        mean = {k: sum(v) / len(v) for k, v in ms.items()}
        cell = {"P": P, "q": q, "member_floats": mf, "calls_per_window": args.calls, "ms": ms, "mean_ms": mean,
                "spread_ms": {k: max(v) - min(v) for k, v in ms.items()},
                "bytes_read": q * mf * 4, "bytes_written": q * mf * 4, "slabs_bytes": P * mf * 4}
        if "device" in mean and "host" in mean:
            cell["host_over_device"] = mean["host"] / mean["device"]
        cells.append(cell)
        print(json.dumps({k: cell[k] for k in ("P", "q", "mean_ms", "bytes_read") + (
            ("host_over_device",) if "host_over_device" in cell else ())}), flush=True)
        del selection, idle, board, pop, weights
        torch.cuda.empty_cache()
    result = {
        "what": "one round of population selection (q = P / 4 members replaced per call, real 256-wide slab): "
                "device = PopulationSelection.select(), host = board.records() + numpy rank + one copy_ per loser, "
                "decide = select() with nobody ready; ms per call, HIP events, one MI355X",
        "lib": os.path.relpath(_lib.LIB_PATH, ROOT), "runs": args.runs, "hbm_peak_bytes_per_s": HBM_PEAK,
        "kernel_trace": None,   # filled from a profiler run of its own by --kernel-trace
        "cells": cells,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return result


if __name__ == "__main__":
    main()
