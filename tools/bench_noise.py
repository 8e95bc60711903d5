"""Time the counter-based policy noise against the torch calls it replaces.

    python tools/bench_noise.py [--runs 5] [--out profiles/policy_noise.json] [--no-train]

HIP events around a window of calls, after a warm-up past the clock boost; the two sides of every
comparison alternate within one process, ``--runs`` times (as tools/bench_population.py does).

* step: one ``PolicyNoise.draw`` of the act draw [P, N] and the two learn draws [P, B] (one launch,
  one allocation) against ``torch.randn((P, N))`` + 2 x ``torch.randn((P, B))`` (three launches,
  three allocations), at P 16, N 1 024, B 256 and at P 16, N 4 096, B 1 024;
* table: one ``PolicyNoise.normal(ACT, 0, 65 536, calls=256)`` against ``torch.randn((256, 65 536))``:
  the eps table of a ``ClosedLoop`` segment;
* train: ``ms_per_iter`` of examples/train_population.py --members 16 --envs-per-member 1024
  --batch 256 under ``--noise torch`` and ``--noise counter``, alternating ``--train-runs`` times.

The counter-based side evaluates log, sqrt and sincospi in f64 for every pair of values; torch's
Philox4x32 + f32 Box-Muller does far less arithmetic per value. The numbers say what that costs.
"""
from __future__ import annotations

import argparse
import importlib.util
import io
import json
import os
import sys
import time
from contextlib import redirect_stdout

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sac-agent_amd"))


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def compare(torch_side, counter_side, runs, target_s):
    for fn in (torch_side, counter_side):
        window(fn, 5)
    est = max(window(torch_side, 10), window(counter_side, 10), 1e-3)     # ms per call
    iters = int(min(max(target_s * 1e3 / est, 20), 5000))
    t, c = [], []
    for _ in range(runs):
        t.append(window(torch_side, iters))
        c.append(window(counter_side, iters))
    mt, mc = sum(t) / runs, sum(c) / runs
    return {"iters": iters, "torch_ms": t, "counter_ms": c, "torch_mean": mt, "counter_mean": mc,
            "torch_spread": max(t) - min(t), "counter_spread": max(c) - min(c), "torch_over_counter": mt / mc}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.15, help="seconds of work per timed window")
    ap.add_argument("--warmup", type=float, default=3.0, help="seconds of draws before the first window")
    ap.add_argument("--no-train", action="store_true", help="skip the train_population.py arm")
    ap.add_argument("--train-iters", type=int, default=300)
    ap.add_argument("--train-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_noise.json"))
    args = ap.parse_args(argv)
    from sacenv import _lib
    from sacenv.noise import ACT, LEARN1, LEARN2, PolicyNoise
    dev = torch.device("cuda:0")

    warm = PolicyNoise(list(range(16)), dev)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.warmup:       # past the clock boost
        for _ in range(200):
            warm.normal(ACT, 0, 4096)
            torch.randn((16, 4096), device=dev)
        torch.cuda.synchronize()

    step = []
    for P, N, B in ((16, 1024, 256), (16, 4096, 1024)):
        noise = PolicyNoise(list(range(P)), dev)
        k = [0]

        def torch_side():
            return torch.randn((P, N), device=dev), torch.randn((P, B), device=dev), torch.randn((P, B), device=dev)

        def counter_side():
            k[0] += 1
            return noise.draw([(ACT, k[0], N), (LEARN1, k[0], B), (LEARN2, k[0], B)])

        row = {"P": P, "N": N, "B": B, "values": P * (N + 2 * B), **compare(torch_side, counter_side, args.runs, args.window)}
        step.append(row)
        print(json.dumps(row), flush=True)

    K, N = 256, 65536
    one = PolicyNoise([0], dev)
    table = {"K": K, "N": N, "values": K * N,
             **compare(lambda: torch.randn((K, N), device=dev), lambda: one.normal(ACT, 0, N, calls=K), args.runs,
                       args.window)}
    table["counter_gvalues_per_s"] = K * N / table["counter_mean"] / 1e6
    print(json.dumps(table), flush=True)

    train = "not measured"
    if not args.no_train:
        spec = importlib.util.spec_from_file_location("train_population",
                                                      os.path.join(ROOT, "examples", "train_population.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        base = ["--members", "16", "--envs-per-member", "1024", "--batch", "256", "--iters", str(args.train_iters)]
        ms = {"torch": [], "counter": []}
        with redirect_stdout(io.StringIO()):
            mod.main(base + ["--noise", "torch"])       # warm-up of the whole loop
            for _ in range(args.train_runs):
                for which in ("torch", "counter"):
                    ms[which].append(mod.main(base + ["--noise", which])["ms_per_iter"])
        train = {"args": base, "runs": args.train_runs, "ms_per_iter": ms,
                 "torch_mean": sum(ms["torch"]) / args.train_runs, "counter_mean": sum(ms["counter"]) / args.train_runs}
        print(json.dumps(train), flush=True)

    result = {"what": "counter-based policy noise (one sacenv_noise_normal launch) vs the torch.randn calls it "
                      "replaces; ms per call, HIP events, both sides alternating in one process, one MI355X; "
                      "train: wall-clock ms per iteration of examples/train_population.py",
              "lib": os.path.relpath(_lib.LIB_PATH, ROOT), "runs": args.runs, "window_s": args.window,
              "step": step, "table": table, "train": train}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return result


if __name__ == "__main__":
    main()
