"""Time a SAC population against the same agents stepped one after the other.

    python tools/bench_population.py [--runs 5] [--label padded] [--out profiles/r11_population.json]

Three arms, HIP events around a window of calls, after a warm-up past the clock boost; the two
sides of every comparison alternate within one process, ``--runs`` times:

* learn: one ``NativeSACPopulation.learn(batch)`` for P in 1, 2, 4, 8, 16 at B = 256 and 1024,
  against P ``NativeSAC.learn(batch)`` calls enqueued back to back on one stream (the yardstick:
  code this tool's subject does not touch);
* act: one population act of P x (65536 / P) rows against P ``NativeSAC.choose_action`` calls.

Every input is a device tensor of the dtype the kernels read, so neither side launches a
conversion. Per case the JSON holds each run's ms per call for both sides, their means, the
spread (max - min) of the sequential side and mean(sequential) / mean(population). ``p1_rule``
is the project's A/B rule for the case it already has: at P = 1 the population call may not be
slower than the one-agent call by more than 3 x that call's spread in the session.

``--p1-objects`` times two equal ``NativeSAC`` objects and two equal one-member populations
instead: how far equal objects are apart, which bounds what the P = 1 comparison resolves.

``--label`` names the library build under test (``SACENV_LIB`` picks another one, e.g. a build
with -DSACENV_POP_PLAIN_GRID); the result is stored under that key of ``--out``, beside what
the file already holds.
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

D = 11


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def compare(seq, pop, runs, target_s):
    """Alternate the two sides ``runs`` times; the window is sized from a first estimate."""
    for fn in (seq, pop):
        window(fn, 5)
    est = max(window(seq, 10), 1e-3)                      # ms per call
    iters = int(min(max(target_s * 1e3 / est, 20), 5000))
    s, p = [], []
    for _ in range(runs):
        s.append(window(seq, iters))
        p.append(window(pop, iters))
    ms, mp = sum(s) / runs, sum(p) / runs
    return {"iters": iters, "sequential_ms": s, "population_ms": p, "sequential_mean": ms, "population_mean": mp,
            "sequential_spread": max(s) - min(s), "population_spread": max(p) - min(p),
            "speedup": ms / mp}


def configs(P, B):
    from sacenv.agent import AgentConfig
    return [AgentConfig(lr_alpha=0.001 + 0.0005 * m, lr_beta=0.0008 + 0.0004 * m, gamma=0.95 + 0.002 * m,
                        tau=0.001 + 0.0005 * m, batch_size=B, max_size=1 << 14) for m in range(P)]


def inputs(dev, P, B):
    g = torch.Generator().manual_seed(P * 100003 + B)
    s = torch.rand((P, B, D), generator=g).to(dev)
    a = (torch.rand((P, B), generator=g) * 2 - 1).to(dev)
    r = torch.rand((P, B), generator=g, dtype=torch.float64).to(dev)
    s2 = (s + 0.01 * torch.randn((P, B, D), generator=g).to(dev)).contiguous()
    d = torch.zeros((P, B), dtype=torch.uint8, device=dev)
    e1, e2 = torch.randn((P, B), generator=g).to(dev), torch.randn((P, B), generator=g).to(dev)
    return (s, a, r, s2, d), (e1, e2)


def p1_objects(dev, batches, runs, iters=3000):
    """How far two equal objects are apart: two ``NativeSAC`` built alike and two one-member
    populations, the four alternating ``runs`` times on the same batch. Their launches are the
    same kernels with the same arguments but for the buffers' addresses; the differences between
    equal objects size what the P = 1 comparison can resolve."""
    from sacenv.population import NativeSACPopulation
    from sacenv.sac_native import NativeSAC
    out = []
    for B in batches:
        cfgs = configs(1, B)
        batch, noise = inputs(dev, 1, B)
        b1, n1 = tuple(t[0] for t in batch), tuple(t[0] for t in noise)
        objs = {"agent_a": NativeSAC(dev, cfgs[0], init_seed=0, with_memory=False),
                "population_a": NativeSACPopulation(dev, cfgs, init_seeds=[0], with_memory=False),
                "agent_b": NativeSAC(dev, cfgs[0], init_seed=0, with_memory=False),
                "population_b": NativeSACPopulation(dev, cfgs, init_seeds=[0], with_memory=False)}
        fns = {k: (lambda o=o: o.learn(b1, n1, losses=False)) if k.startswith("agent") else
                  (lambda o=o: o.learn(batch, noise, losses=False)) for k, o in objs.items()}
        for f in fns.values():
            window(f, iters)
        ms = {k: [] for k in fns}
        for _ in range(runs):
            for k, f in fns.items():
                ms[k].append(window(f, iters))
        row = {"B": B, "iters": iters,
               **{k: {"ms": v, "mean": sum(v) / runs, "spread": max(v) - min(v)} for k, v in ms.items()}}
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--p1-objects", action="store_true",
                    help="only the P = 1 comparison of equal objects (stored under --label)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--members", default="1,2,4,8,16")
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--act-rows", type=int, default=65536)
    ap.add_argument("--window", type=float, default=0.15, help="seconds of work per timed window")
    ap.add_argument("--warmup", type=float, default=3.0, help="seconds of learn() before the first window")
    ap.add_argument("--label", default="padded")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_population.json"))
    args = ap.parse_args(argv)
    from sacenv import _lib
    from sacenv.population import NativeSACPopulation
    from sacenv.sac_native import NativeSAC
    dev = torch.device("cuda:0")
    members = [int(x) for x in args.members.split(",")]
    batches = [int(x) for x in args.batches.split(",")]

    # past the clock boost: the first seconds of a session run faster than its steady state
    warm = NativeSAC(dev, configs(1, 1024)[0], init_seed=0, with_memory=False)
    wb, wn = inputs(dev, 1, 1024)
    wb, wn = tuple(t[0] for t in wb), tuple(t[0] for t in wn)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.warmup:
        for _ in range(200):
            warm.learn(wb, wn, losses=False)
        torch.cuda.synchronize()
    del warm

    def store(result):
        data = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                data = json.load(f)
        data[args.label] = result
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(data, f, indent=1)
            f.write("\n")

    if args.p1_objects:
        result = {"what": "learn() ms per call of two equal NativeSAC objects and two equal one-member "
                          "populations, alternating in one process", "runs": args.runs,
                  "learn": p1_objects(dev, batches, args.runs)}
        store(result)
        return result

    learn, act = [], []
    for B in batches:
        for P in members:
            cfgs = configs(P, B)
            agents = [NativeSAC(dev, cfgs[m], init_seed=m, with_memory=False) for m in range(P)]
            pop = NativeSACPopulation(dev, cfgs, init_seeds=list(range(P)), with_memory=False)
            batch, noise = inputs(dev, P, B)
            per = [(tuple(t[m] for t in batch), tuple(t[m] for t in noise)) for m in range(P)]

            def seq():
                for m in range(P):
                    agents[m].learn(per[m][0], per[m][1], losses=False)

            def one():
                pop.learn(batch, noise, losses=False)

            row = {"B": B, "P": P, **compare(seq, one, args.runs, args.window)}
            learn.append(row)
            print(json.dumps(row), flush=True)
            del agents, pop
    for P in members:
        n = args.act_rows // P
        cfgs = configs(P, 256)
        agents = [NativeSAC(dev, cfgs[m], init_seed=m, with_memory=False) for m in range(P)]
        pop = NativeSACPopulation(dev, cfgs, init_seeds=list(range(P)), with_memory=False)
        obs, eps = torch.rand((P, n, D), device=dev), torch.randn((P, n), device=dev)

        def seq():
            for m in range(P):
                agents[m].choose_action(obs[m], eps[m])

        def one():
            pop.choose_action(obs, eps)

        row = {"P": P, "rows_per_member": n, **compare(seq, one, args.runs, args.window)}
        act.append(row)
        print(json.dumps(row), flush=True)
        del agents, pop

    def rule(row):
        slack = 3.0 * row["sequential_spread"]
        return {"population_minus_single_ms": row["population_mean"] - row["sequential_mean"],
                "allowed_ms": slack, "ok": row["population_mean"] - row["sequential_mean"] <= slack}

    result = {
        "what": "SAC population (one set of launches for P agents) vs the same P NativeSAC agents stepped "
                "back to back on one stream; ms per call of the whole population, HIP events, one MI355X",
        "lib": os.path.relpath(_lib.LIB_PATH, ROOT), "runs": args.runs, "window_s": args.window,
        "learn": learn, "act": act,
        "p1_rule": {**{f"learn_B{r['B']}": rule(r) for r in learn if r["P"] == 1},
                    **{"act": rule(r) for r in act if r["P"] == 1}},
    }
    store(result)
    print(json.dumps({"label": args.label, "p1_rule": result["p1_rule"]}))
    return result


if __name__ == "__main__":
    main()
