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

    python tools/bench_population_replay.py --pool-rows [--example-parent DIR] [--example-learn]

times the pooled sample (part of each batch drawn from all members' rings) against the plain one
instead and writes profiles/shared_replay_bench.json: see ``pooled_main``.
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


def median(xs):
    s = sorted(xs)
    n = len(s)
    return s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])


def summary(xs):
    return {"ms": xs, "median": median(xs), "spread": max(xs) - min(xs)}


class Blocker:
    """Device work the timed launches queue up behind, so that the events around them see the
    device's time per launch and not the host's time per call: ``passes`` in-place sweeps of a
    1-GiB tensor (the calls are enqueued while it runs; ``blocked`` says when they were not)."""

    def __init__(self, dev, passes=48):
        self.x = torch.ones(1 << 28, dtype=torch.float32, device=dev)
        self.passes = passes

    def __call__(self):
        for _ in range(self.passes):
            self.x.mul_(1.0)


def blocked(fn, n, blocker):
    """(ms per call on the device, queued): n calls enqueued behind the blocker; ``queued`` is
    False if the blocker had finished before the last call was enqueued (then the figure holds
    host time and is not used)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    blocker()
    e0.record()
    for _ in range(n):
        fn()
    queued = not e0.query()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, queued


def example_line(tree, argv):
    """The JSON line of one ``examples/train_population.py`` run in a process of its own, from
    the checkout at ``tree``."""
    import subprocess
    tree = os.path.abspath(tree)
    out = subprocess.run([sys.executable, os.path.join(tree, "examples", "train_population.py"), *argv], cwd=tree,
                         check=True, capture_output=True, text=True).stdout
    return json.loads([l for l in out.split("\n") if l.startswith("{")][-1])


def pooled_main(args):
    """``--pool-rows``: the pooled sample (``PopulationReplay.sample(B, pool_rows=K)``, K = B / 2
    and K = B) against the plain one in the same process: P members with full rings of M rows.
    Per B and variant, ms per call for all members, the variants alternating ``--runs`` times
    (median and max - min): ``call`` is HIP events around a window of calls enqueued from Python
    (what an iteration pays), ``device`` the same calls queued behind a blocker (the device's
    time for the draw and the gather launch together), ``gather_device`` the gather launch alone
    (``gather`` / ``gather_pool`` on the indices just drawn) and ``draw_device`` their difference.
    With ``--example-parent DIR`` (a built checkout of the parent commit) the example's
    ``ms_per_iter`` at 16 x 1 024 without the flag, parent and head alternating three times, and
    with ``--example-learn`` its score tables at 4 x 1 024 for 300 iterations with
    ``--share-replay 0`` and ``--share-replay B / 2``, go into the same file."""
    from sacenv import _lib
    from sacenv.population_replay import PopulationReplay
    dev = torch.device("cuda:0")
    P, M = int(args.members.split(",")[-1]), args.max_size or 1_000_000
    batches = [int(x) for x in args.batches.split(",")]
    replay = PopulationReplay(P, M, (D,), 1, device=dev, seeds=list(range(P)))
    n = 1 << 16
    s, a, r, s2, c, fs = rows(dev, P, n)
    while replay.mem_cntr < M:                               # full rings
        replay.store_batch(s, a, r, s2, c, final_state=fs)
    blocker = Blocker(dev)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.warmup:            # past the clock boost, every variant warm
        for B in batches:
            for K in (0, B // 2, B):
                for _ in range(20):
                    replay.sample(B, as_bool=False, pool_rows=K)
        torch.cuda.synchronize()
    cells = []
    for B in batches:
        variants = {"plain": 0, "half": B // 2, "full": B}
        samplers = {k: (lambda K=K: replay.sample(B, as_bool=False, pool_rows=K)) for k, K in variants.items()}
        idx = {k: samplers[k]()[5] for k in variants}
        gathers = {k: ((lambda i=idx[k]: replay.gather_pool(i, as_bool=False)) if K else
                       (lambda i=idx[k]: replay.gather(i, as_bool=False))) for k, K in variants.items()}
        est = max(window(samplers["plain"], 20), 1e-3)
        iters = int(min(max(args.window * 1e3 / est, 50), 20000))
        nq = 200
        raw = {k: {"call": [], "device": [], "gather_device": []} for k in variants}
        ok = True
        for _ in range(args.runs):
            for k in variants:
                raw[k]["call"].append(window(samplers[k], iters))
            for k in variants:
                for what, fn in (("device", samplers[k]), ("gather_device", gathers[k])):
                    ms, queued = blocked(fn, nq, blocker)
                    ok &= queued
                    raw[k][what].append(ms)
        cell = {"B": B, "P": P, "max_size": M, "rows_held": M, "window_iters": iters, "queued_calls": nq,
                "device_figures_queued": ok}
        for k, K in variants.items():
            v = {"pool_rows": K, **{what: summary(xs) for what, xs in raw[k].items()}}
            v["draw_device_median"] = v["device"]["median"] - v["gather_device"]["median"]
            cell[k] = v
        cells.append(cell)
        print(json.dumps({"B": B, **{k: {"call": round(cell[k]["call"]["median"], 5),
                                         "device": round(cell[k]["device"]["median"], 5),
                                         "gather": round(cell[k]["gather_device"]["median"], 5),
                                         "draw": round(cell[k]["draw_device_median"], 5)} for k in variants},
                          "plain_call_spread": round(cell["plain"]["call"]["spread"], 5), "queued": ok}), flush=True)
    result = {
        "what": "PopulationReplay.sample with pool rows (include/sacenv_population_share.h) against the plain "
                "sample, whose two kernels are the parent commit's (tools/kernel_diff.py: no difference); ms per "
                "call for all members, HIP events, one MI355X, one process",
        "lib": os.path.relpath(_lib.LIB_PATH, ROOT), "runs": args.runs, "window_s": args.window, "cells": cells,
    }
    del replay, blocker
    torch.cuda.empty_cache()
    if args.example_parent:
        base = ["--members", "16", "--envs-per-member", "1024"]
        runs = {"parent": [], "head": []}
        for _ in range(3):
            for side, tree in (("parent", args.example_parent), ("head", ROOT)):
                runs[side].append(example_line(tree, base)["ms_per_iter"])
        result["example_16x1024_ms_per_iter"] = {
            **runs, "parent_spread": max(runs["parent"]) - min(runs["parent"]),
            "head_median_minus_parent_median": median(runs["head"]) - median(runs["parent"])}
        print(json.dumps(result["example_16x1024_ms_per_iter"]), flush=True)
    if args.example_learn:
        base = ["--members", "4", "--envs-per-member", "1024", "--iters", "300"]
        B = 1024                                             # the example's default batch
        result["example_4x1024_300_iters"] = {
            f"share_replay_{K}": (lambda o: {"ms_per_iter": o["ms_per_iter"], "pool_rows": o["pool_rows"],
                                             "table": o["table"]})(example_line(ROOT, base + ["--share-replay", str(K)]))
            for K in (0, B // 2)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return result


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool-rows", action="store_true",
                    help="time the pooled sample against the plain one (the last of --members, full rings) and "
                         "write profiles/shared_replay_bench.json")
    ap.add_argument("--example-parent", default=None, metavar="DIR",
                    help="with --pool-rows: a built checkout of the parent commit, for the example's ms_per_iter")
    ap.add_argument("--example-learn", action="store_true",
                    help="with --pool-rows: the example's score tables with and without shared replay")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--members", default="1,2,4,8,16")
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--rows", type=int, default=1024, help="rows per member per store")
    ap.add_argument("--max-size", type=int, default=None, help="ring rows per member (default: AgentConfig's)")
    ap.add_argument("--window", type=float, default=0.15, help="seconds of work per timed window")
    ap.add_argument("--warmup", type=float, default=3.0, help="seconds of work before the first window")
    ap.add_argument("--out", default=None,
                    help="default: profiles/r12_population_replay.json, with --pool-rows profiles/shared_replay_bench.json")
    args = ap.parse_args(argv)
    args.out = args.out or os.path.join(ROOT, "profiles", "shared_replay_bench.json" if args.pool_rows
                                        else "r12_population_replay.json")
    if args.pool_rows:
        return pooled_main(args)
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
