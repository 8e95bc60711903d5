"""Time a population's replay side: one PopulationReplay against one DeviceReplayBuffer per member.

    python tools/bench_population_replay.py [--runs 5] [--out profiles/r12_population_replay.json]

The method of tools/bench_population.py: HIP events around a window of calls, in one process,
after a warm-up past the clock boost; the two sides of every comparison alternate ``--runs``
times. Per cell (P members x batch B, n rows per member per store, D = 11, the default
``max_size``) and per side, ms per

* store: the rows of one step into every member's buffer
  ("members": P ``DeviceReplayBuffer.store_batch`` calls, the parent's path;
  "population": one ``PopulationReplay.store_batch``);
* sample: one batch per member as ``learn`` takes them
  ("members": P ``sample`` calls and the five ``torch.stack`` copies; "population": one ``sample``);
* iter: store + sample + the population's learn (``NativeSACPopulation.learn()`` on its own memory).

Every input is a device tensor of the dtype the kernels read, so neither side launches a
conversion. The project's A/B rule per cell and metric: the band is 3 x (max - min) of the
members side in this session; at P = 1 the population side may not be slower than the members
side by more than the band, at P >= 4 it must be faster by more than the band (P = 2 is
reported without a bar). Every run goes into the JSON.
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

from bench_population import configs, window  # noqa: E402

D = 11


def compare(members, population, runs, target_s):
    for fn in (members, population):
        window(fn, 5)
    est = max(window(members, 10), 1e-3)                  # ms per call
    iters = int(min(max(target_s * 1e3 / est, 20), 5000))
    a, b = [], []
    for _ in range(runs):
        a.append(window(members, iters))
        b.append(window(population, iters))
    ma, mb = sum(a) / runs, sum(b) / runs
    return {"iters": iters, "members_ms": a, "population_ms": b, "members_mean": ma, "population_mean": mb,
            "members_spread": max(a) - min(a), "population_spread": max(b) - min(b), "speedup": ma / mb}


def rule(P, row):
    """The A/B rule for one cell and metric."""
    band = 3.0 * row["members_spread"]
    gain = row["members_mean"] - row["population_mean"]   # > 0: the population side is faster
    if P == 1:
        bar, ok = "not slower than members by more than the band", gain >= -band
    elif P >= 4:
        bar, ok = "faster than members by more than the band", gain > band
    else:
        bar, ok = "none (reported only)", None
    return {"band_ms": band, "members_minus_population_ms": gain, "bar": bar, "ok": ok}


def rows(dev, P, n):
    g = torch.Generator().manual_seed(P * 7919 + n)
    s = torch.rand((P, n, D), generator=g).to(dev)
    a = (torch.rand((P, n, 1), generator=g) * 2 - 1).to(dev)
    r = torch.rand((P, n), generator=g).to(dev)
    s2 = torch.rand((P, n, D), generator=g).to(dev)
    fs = torch.rand((P, n, D), generator=g).to(dev)
    c = (torch.rand((P, n), generator=g) < 0.02).to(torch.uint8).to(dev)
    return s, a, r, s2, c, fs


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--members", default="1,2,4,8,16")
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--rows", type=int, default=1024, help="rows per member per store")
    ap.add_argument("--max-size", type=int, default=None, help="ring rows per member (default: AgentConfig's)")
    ap.add_argument("--window", type=float, default=0.15, help="seconds of work per timed window")
    ap.add_argument("--warmup", type=float, default=3.0, help="seconds of work before the first window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_population_replay.json"))
    args = ap.parse_args(argv)
    import dataclasses
    from sacenv import _lib
    from sacenv.agent import AgentConfig
    from sacenv.population import NativeSACPopulation
    from sacenv.population_replay import PopulationReplay
    dev = torch.device("cuda:0")
    members = [int(x) for x in args.members.split(",")]
    batches = [int(x) for x in args.batches.split(",")]
    M = args.max_size or AgentConfig().max_size
    n = args.rows

    cells = []
    warmed = False
    for B in batches:
        for P in members:
            cfgs = [dataclasses.replace(c, max_size=M) for c in configs(P, B)]
            seeds = list(range(P))
            replay = PopulationReplay(P, M, (D,), 1, device=dev, seeds=seeds)
            pa = NativeSACPopulation(dev, cfgs, init_seeds=seeds, replay=replay)
            pb = NativeSACPopulation(dev, cfgs, init_seeds=seeds, buffer_seeds=seeds)
            s, a, r, s2, c, fs = rows(dev, P, n)
            lt_a = torch.zeros((P, n), dtype=torch.uint8, device=dev)
            lt_b = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(P)]
            per = [tuple(t[m] for t in (s, a, r, s2, c, fs)) for m in range(P)]   # (views: no launches)
            noise = (torch.randn((P, B), device=dev), torch.randn((P, B), device=dev))

            def store_members():
                for m in range(P):
                    sm, am, rm, s2m, cm, fsm = per[m]
                    pb.remember(m, sm, am, rm, s2m, cm, final_state=fsm, last_term=lt_b[m])

            def store_population():
                replay.store_batch(s, a, r, s2, c, final_state=fs, last_term=lt_a)

            def iter_members():
                store_members()
                pb.learn(noise=noise, losses=False)

            def iter_population():
                store_population()
                pa.learn(noise=noise, losses=False)

            if not warmed:  # past the clock boost: the first seconds of a session run faster
                t0 = time.perf_counter()
                while time.perf_counter() - t0 < args.warmup:
                    for _ in range(50):
                        iter_members()
                        iter_population()
                    torch.cuda.synchronize()
                warmed = True
            store_members()
            store_population()                                # (both sides hold rows to sample)
            cell = {"B": B, "P": P, "rows_per_store": n, "max_size": M,
                    "store": compare(store_members, store_population, args.runs, args.window),
                    "sample": compare(pb.sample, pa.sample, args.runs, args.window),
                    "iter": compare(iter_members, iter_population, args.runs, args.window)}
            cell["rule"] = {k: rule(P, cell[k]) for k in ("store", "sample", "iter")}
            cells.append(cell)
            print(json.dumps({"B": B, "P": P, **{k: {"members": round(cell[k]["members_mean"], 5),
                                                     "population": round(cell[k]["population_mean"], 5),
                                                     "band": round(cell["rule"][k]["band_ms"], 5),
                                                     "ok": cell["rule"][k]["ok"]}
                                                 for k in ("store", "sample", "iter")}}), flush=True)
            del replay, pa, pb
            torch.cuda.empty_cache()

    result = {
        "what": "replay side of a SAC population: one PopulationReplay (population) vs one DeviceReplayBuffer per "
                "member and five stack copies (members); ms per call for all members, HIP events, one MI355X",
        "lib": os.path.relpath(_lib.LIB_PATH, ROOT), "runs": args.runs, "window_s": args.window,
        "rule": "band = 3 x (max - min) of the members side in this session; P = 1: population not slower than "
                "members by more than the band; P >= 4: faster by more than the band",
        "cells": cells,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return result


if __name__ == "__main__":
    main()
