"""Time the prioritized population replay against the uniform one.

    python tools/bench_prioritized_replay.py [--runs 5] [--example-parent DIR] [--out profiles/prioritized_replay_bench.json]

The method of tools/bench_population_replay.py ``--pool-rows``: one process, P = 16 members with
full rings of 1 000 000 rows and a priority on every row, a warm-up past the clock boost, the
variants alternating ``--runs`` times (median and max - min). Per batch B, ms per call for all
members:

* ``call``: HIP events around a window of calls enqueued from Python (what an iteration pays);
* ``device``: the same calls queued behind a blocker (the device's time for the call's launches);

for ``plain`` (``PopulationReplay.sample``: ``sacenv_replay_pop_sample``, on the same arena),
``prioritized`` (``PrioritizedPopulationReplay.sample``: draw, weights, gather), ``prioritized_bare``
(``sacenv_replay_prio_sample`` with no weights: draw and gather), ``gather`` (the gather launch
alone), ``update_td`` and ``mark`` (1 024 rows per member). ``draw_device`` is ``prioritized_bare``
minus ``gather``: the draw launch alone. The draw reads one node per level and slot (256 B of
leaves, 512 B per level above, 32 B at the top of a 1 000 000-row ring); its bytes per second stand
beside a plain device copy's.

With ``--example-parent DIR`` (a built checkout of the parent commit) the example's ``ms_per_iter``
at 16 x 1 024 goes into the same file: with the flag, without it, and at the parent, alternating
three times.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sac-agent_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_population import window  # noqa: E402
from bench_population_replay import Blocker, D, blocked, example_line, median, rows, summary  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--max-size", type=int, default=1_000_000)
    ap.add_argument("--window", type=float, default=0.15, help="seconds of work per timed window")
    ap.add_argument("--warmup", type=float, default=3.0, help="seconds of work before the first window")
    ap.add_argument("--example-parent", default=None, metavar="DIR",
                    help="a built checkout of the parent commit, for the example's ms_per_iter")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prioritized_replay_bench.json"))
    args = ap.parse_args(argv)
    from sacenv import _lib
    from sacenv.population_replay import PopulationReplay
    from sacenv.prioritized import PrioritizedPopulationReplay
    dev = torch.device("cuda:0")
    P, M = args.members, args.max_size
    batches = [int(x) for x in args.batches.split(",")]
    rep = PrioritizedPopulationReplay(P, M, (D,), 1, device=dev, seeds=list(range(P)))
    n = 1 << 16
    s, a, r, s2, c, fs = rows(dev, P, n)
    while rep.mem_cntr < M:                                   # full rings
        rep.store_batch(s, a, r, s2, c, final_state=fs)
    g = torch.Generator().manual_seed(1)
    every = torch.arange(M).expand(P, M).contiguous()
    rep.set_priorities(every, torch.randint(1, 1 << 20, (P, M), generator=g))   # a priority of its own on every row
    del every
    torch.cuda.synchronize()
    levels = [int(x) for x in list(rep.prio_layout.count)[: rep.prio_layout.levels]]
    slot_bytes = sum(min(64, levels[k]) * (4 if k == 0 else 8) for k in range(len(levels)))
    n_mark = 1024
    blocker = Blocker(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    y = torch.empty_like(blocker.x)
    y.copy_(blocker.x)
    e0.record()
    for _ in range(10):
        y.copy_(blocker.x)
    e1.record()
    torch.cuda.synchronize()
    copy_bytes_per_s = 10 * 2 * blocker.x.numel() * 4 / (e0.elapsed_time(e1) * 1e-3)    # read + write
    del y
    cells = []
    for B in batches:
        idx = torch.randint(0, M, (P, B), generator=g).to(dev)
        sq1, sq2 = torch.rand((P, B), generator=g).to(dev), torch.rand((P, B), generator=g).to(dev)
        leaf = torch.empty((P, B), dtype=torch.int32, device=dev)
        out = rep._outputs(B, idx=True)
        ptrs = [t.data_ptr() for t in out[:5]]
        stream = rep.stream

        def bare():
            _lib.check(rep._sample(rep._pp, P, rep.arena.data_ptr(), rep.prio.data_ptr(), B, 0, rep._prio_seeds,
                                   out[5].data_ptr(), leaf.data_ptr(), None, 0.0, *ptrs, stream))

        def mark():
            _lib.check(rep._mark(rep._pp, P, None, rep.prio.data_ptr(), 12345, n_mark, stream))

        fns = {"plain": lambda: PopulationReplay.sample(rep, B, as_bool=False),
               "prioritized": lambda: rep.sample(B, as_bool=False),
               "prioritized_bare": bare,
               "gather": lambda: rep.gather(idx, as_bool=False),
               "update_td": lambda: rep.update_priorities(idx, sq1, sq2),
               "mark": mark}
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.warmup:         # past the clock boost, every variant warm
            for fn in fns.values():
                for _ in range(20):
                    fn()
            torch.cuda.synchronize()
        est = max(window(fns["plain"], 20), 1e-3)
        iters = int(min(max(args.window * 1e3 / est, 50), 20000))
        nq = 200
        raw = {k: {"call": [], "device": []} for k in fns}
        ok = True
        for _ in range(args.runs):
            for k, fn in fns.items():
                raw[k]["call"].append(window(fn, iters))
            for k, fn in fns.items():
                ms, queued = blocked(fn, nq, blocker)
                ok &= queued
                raw[k]["device"].append(ms)
        cell = {"B": B, "P": P, "max_size": M, "levels": levels, "window_iters": iters, "queued_calls": nq,
                "device_figures_queued": ok, "mark_rows": n_mark,
                **{k: {what: summary(xs) for what, xs in v.items()} for k, v in raw.items()}}
        draw = cell["prioritized_bare"]["device"]["median"] - cell["gather"]["device"]["median"]
        cell["draw_device_median"] = draw
        cell["draw_bytes"] = P * B * slot_bytes
        cell["draw_bytes_per_s"] = cell["draw_bytes"] / (draw * 1e-3) if draw > 0 else None
        cells.append(cell)
        print(json.dumps({"B": B, **{k: {"call": round(cell[k]["call"]["median"], 5),
                                         "device": round(cell[k]["device"]["median"], 5)} for k in fns},
                          "draw": round(draw, 5), "draw_GBps": None if draw <= 0 else round(cell["draw_bytes_per_s"] / 1e9, 3),
                          "plain_call_spread": round(cell["plain"]["call"]["spread"], 5), "queued": ok}), flush=True)
    result = {
        "what": "PrioritizedPopulationReplay (include/sacenv_prioritized_replay.h) against PopulationReplay.sample on "
                "the same arena; ms per call for all members, HIP events, one MI355X, one process",
        "lib": os.path.relpath(_lib.LIB_PATH, ROOT), "runs": args.runs, "window_s": args.window,
        "slot_bytes": slot_bytes, "copy_bytes_per_s": copy_bytes_per_s, "cells": cells,
    }
    del rep, blocker
    torch.cuda.empty_cache()
    if args.example_parent:
        base = ["--members", "16", "--envs-per-member", "1024"]
        runs = {"parent": [], "head": [], "head_prioritized": []}
        for _ in range(3):
            for side, tree, extra in (("parent", args.example_parent, []), ("head", ROOT, []),
                                      ("head_prioritized", ROOT, ["--prioritized"])):
                runs[side].append(example_line(tree, base + extra)["ms_per_iter"])
        result["example_16x1024_ms_per_iter"] = {
            **runs, "parent_spread": max(runs["parent"]) - min(runs["parent"]),
            "head_median_minus_parent_median": median(runs["head"]) - median(runs["parent"]),
            "prioritized_median_minus_head_median": median(runs["head_prioritized"]) - median(runs["head"])}
        print(json.dumps(result["example_16x1024_ms_per_iter"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return result


if __name__ == "__main__":
    main()
