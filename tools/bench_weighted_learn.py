#!/usr/bin/env python
"""What the weighted learn costs, and that the unweighted one did not move
(profiles/weighted_learn_bench.json).

    python tools/bench_weighted_learn.py --parent-tree DIR [--out profiles/weighted_learn_bench.json]
        [--rounds 4] [--calls 400] [--iters 300]

``DIR`` is a checkout of the parent commit with its library built (``python __graft_entry__.py
build`` there). Every measurement is a process of its own that imports ``sacenv`` from one of the
two trees; the variants alternate within a round, so drift of the machine falls on all of them, and
each variant's own spread over the rounds is reported beside its median:

* ``learn``: ``NativeSACPopulation.learn(batch, noise, losses=False)`` at 16 members, batch 256 and
  1 024, us per call over ``--calls`` calls after a warm-up (host clock around work that ends in a
  device synchronise): the parent, the head with ``weights=None``, the head with weights;
* ``example``: the median ``ms_per_iter`` of examples/train_population.py at 16 x 1 024 envs,
  ``--iters`` iterations: parent and head without ``--prioritized``, head with it, head with
  ``--importance-weights --beta-final 1 --beta-anneal N``;
* ``sample``: ``PrioritizedPopulationReplay.sample`` plain and annealed, us per call, in one process.

Needs a GPU; there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, D = 16, 11


def _use(tree: str) -> None:
    sys.path.insert(0, os.path.join(tree, "sac-agent_amd"))


def _timed(fn, calls: int) -> float:
    """us per call of ``fn`` over ``calls`` calls, device-synchronised at both ends."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def worker_learn(tree: str, weighted: bool, calls: int) -> dict:
    _use(tree)
    import torch
    from sacenv import NativeSACPopulation
    from sacenv.agent import AgentConfig
    dev = torch.device("cuda")
    out = {}
    for B in (256, 1024):
        pop = NativeSACPopulation(dev, [AgentConfig(batch_size=B, lr_alpha=0.001 + 1e-4 * m) for m in range(P)],
                                  init_seeds=list(range(P)), with_memory=False)
        g = torch.Generator().manual_seed(B)
        batch = (torch.rand((P, B, D), generator=g).to(dev), (torch.rand((P, B, 1), generator=g) * 2 - 1).to(dev),
                 torch.rand((P, B), generator=g, dtype=torch.float64).to(dev),
                 torch.rand((P, B, D), generator=g).to(dev), (torch.rand((P, B), generator=g) < 0.1).to(dev))
        noise = (torch.randn((P, B), generator=g).to(dev), torch.randn((P, B), generator=g).to(dev))
        kw = {"weights": (torch.rand((P, B), generator=g) * 0.95 + 0.05).to(dev)} if weighted else {}
        fn = lambda: pop.learn(batch, noise, losses=False, **kw)  # noqa: E731
        _timed(fn, 50)                                             # warm-up: code objects, allocator
        out[str(B)] = [_timed(fn, calls) for _ in range(3)]        # three windows
    return out


def worker_example(tree: str, flags: list, iters: int) -> dict:
    _use(tree)
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_population",
                                                  os.path.join(tree, "examples", "train_population.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--members", str(P), "--envs-per-member", "1024", "--batch", "1024", "--iters", str(iters),
            "--noise", "counter"]
    sys.stdout, keep = open(os.devnull, "w"), sys.stdout           # the example prints its tables
    try:
        mod.main(base[:7] + ["40"] + base[8:] + flags)             # warm-up
        runs = [mod.main(base + flags)["ms_per_iter"] for _ in range(3)]
    finally:
        sys.stdout = keep
    return {"ms_per_iter": runs}


def worker_sample(tree: str, calls: int) -> dict:
    _use(tree)
    import torch
    from sacenv.prioritized import PrioritizedPopulationReplay
    dev, M, B = torch.device("cuda"), 1 << 16, 1024
    g = torch.Generator().manual_seed(3)
    rows = (torch.rand((P, M, D), generator=g), torch.rand((P, M, 1), generator=g), torch.rand((P, M), generator=g),
            torch.rand((P, M, D), generator=g), torch.zeros((P, M), dtype=torch.uint8))
    idx, leaf = torch.randint(0, M, (P, 8192), generator=g), torch.randint(1, 1 << 22, (P, 8192), generator=g)
    reps = {}
    for name, kw in (("plain", {}), ("annealed", dict(beta_final=1.0, beta_anneal=10 ** 6))):
        for safe in (False, True):
            r = PrioritizedPopulationReplay(P, M, (D,), 1, device=dev, seeds=list(range(P)), **kw)
            r.store_batch(*rows)
            r.set_priorities(idx, leaf)
            reps[f"{name}{'_graph_safe' if safe else ''}"] = (r, safe)
    out = {k: [] for k in reps}
    for k, (r, safe) in reps.items():
        _timed(lambda: r.sample(B, as_bool=False, graph_safe=safe), 50)
    for _ in range(5):                                             # alternating windows
        for k, (r, safe) in reps.items():
            out[k].append(_timed(lambda: r.sample(B, as_bool=False, graph_safe=safe), calls))
    return out


def _spawn(args: list) -> dict:
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", json.dumps(args)], check=True,
                       stdout=subprocess.PIPE, text=True, timeout=600)
    return json.loads(r.stdout.strip().splitlines()[-1])


def _summary(xs: list) -> dict:
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "spread": max(xs) - min(xs), "n": len(xs),
            "values": xs}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_learn_bench.json"))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--worker", default=None)
    a = ap.parse_args()
    if a.worker:
        kind, *rest = json.loads(a.worker)
        fn = {"learn": worker_learn, "example": worker_example, "sample": worker_sample}[kind]
        print(json.dumps(fn(*rest)))
        return
    if not a.parent_tree:
        ap.error("--parent-tree: a checkout of the parent commit with its library built")
    parent = os.path.abspath(a.parent_tree)
    doc = {"what": __doc__.split("\n\n")[0], "members": P, "rounds": a.rounds, "calls": a.calls, "iters": a.iters}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")

    learn = {v: {"256": [], "1024": []} for v in ("parent", "head_none", "head_weights")}
    for rnd in range(a.rounds):
        for v, args in (("parent", [parent, False]), ("head_none", [ROOT, False]), ("head_weights", [ROOT, True])):
            got = _spawn(["learn", *args, a.calls])
            for B in learn[v]:
                learn[v][B].append(statistics.median(got[B]))
            print(f"round {rnd} learn {v}: {got}", flush=True)
    doc["learn_us_per_call"] = {v: {B: _summary(x) for B, x in per.items()} for v, per in learn.items()}
    for B in ("256", "1024"):
        s = doc["learn_us_per_call"]
        d = s["head_none"][B]["median"] - s["parent"][B]["median"]
        doc.setdefault("learn_verdict", {})[B] = {
            "head_none_minus_parent_us": d, "parent_spread_us": s["parent"][B]["spread"],
            "inside_parent_spread": abs(d) <= s["parent"][B]["spread"],
            "weights_minus_none_us": s["head_weights"][B]["median"] - s["head_none"][B]["median"]}
    save()
    N = max(a.iters // 2, 1)
    variants = (("parent_plain", parent, []), ("head_plain", ROOT, []), ("parent_prioritized", parent, ["--prioritized"]),
                ("head_prioritized", ROOT, ["--prioritized"]),
                ("head_importance_weights", ROOT, ["--prioritized", "--importance-weights", "--beta-final", "1",
                                                   "--beta-anneal", str(N)]))
    ex = {v: [] for v, _, _ in variants}
    for rnd in range(max(a.rounds - 1, 1)):
        for v, tree, flags in variants:
            got = _spawn(["example", tree, flags, a.iters])
            ex[v].append(statistics.median(got["ms_per_iter"]))
            print(f"round {rnd} example {v}: {got}", flush=True)
    doc["example_ms_per_iter"] = {v: _summary(x) for v, x in ex.items()}
    doc["example_ms_per_iter"]["beta_anneal"] = N
    save()
    got = _spawn(["sample", ROOT, a.calls])
    doc["sample_us_per_call"] = {k: _summary(x) for k, x in got.items()}
    save()
    print(json.dumps({k: doc[k] for k in ("learn_verdict",)}, indent=1))


if __name__ == "__main__":
    main()
