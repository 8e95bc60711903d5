"""Time the population scoreboard (sacenv_board_update) against the episode scan it follows.

    python tools/bench_scoreboard.py [--members 16] [--envs-per-member 4096] [--steps 256]
        [--reps 200] [--windows 5] [--lookback 50] [--out profiles/scoreboard_bench.json]

Rollouts of ``--steps`` steps over members x envs-per-member boat envs (experiment 6, U(-1, 1)
actions, max_episode_steps 500) give the records, as in tools/bench_episodes.py. Two shapes, in
one process:

* ``rollout``: one scan and one board update per K-step rollout;
* ``step``: one scan and one board update per step (K = 1), over the rows of the same rollouts.

For each, ``--reps`` scans fill the log first (untimed, the log's total noted after each); then
windows of ``--reps`` calls between two device events time

* ``scan``          sacenv_episodes_update on those records (the bar);
* ``board``         sacenv_board_update alone, no snapshot pointers: before each call an 8-B device
                    copy moves the log's total on to where the scan of that call had left it
                    (``copy_only`` times those copies alone, to be subtracted);
* ``board_no_save`` the same with weights and snapshot given, on a copy of the log whose scores
                    are all equal (a tie at every episode: the rule runs in full and selects
                    nobody) -- the case the bar names;
* ``board_all_save`` with weights and snapshot on the real scores (every member saves in every
                    call at these sizes), and ``torch_copy`` of the same [P, member_floats] tensor.

Every window goes to the JSON file; prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sac-agent_amd"))


def _window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us per call


def _stats(ws):
    return {"median": float(np.median(ws)), "min": float(min(ws)), "max": float(max(ws)), "windows": [float(w) for w in ws]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--envs-per-member", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--lookback", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scoreboard_bench.json"))
    args = ap.parse_args(argv)
    from sacenv import VecBoatEnv, _lib
    from sacenv.episodes import ENTRY_DTYPE, EpisodeLog
    dev = torch.device("cuda")
    P, M, K, R = args.members, args.envs_per_member, args.steps, args.reps
    N = P * M
    lib = _lib.load()
    env = VecBoatEnv({"base_settings": {"experiment": 6, "test_mode": 0}}, N, seed=0, device=dev,
                     max_episode_steps=500)
    log = EpisodeLog(env, capacity=N * K)      # (no window overflows it: --reps calls of up to N * K / reps)
    g = torch.Generator(device=dev).manual_seed(0)
    actions = torch.rand(K, N, device=dev, generator=g) * 2 - 1
    rollouts = [env.rollout(actions)[0] for _ in range(args.buffers)]
    sp = _lib.SacParams(obs_dim=11, n_actions=1, hidden=_lib.SAC_HIDDEN, batch=1024, max_action=1.0, gamma=0.99,
                        tau=0.005, reward_scale=2.0, lr_actor=3e-4, lr_critic=3e-4, adam_beta1=0.9,
                        adam_beta2=0.999, adam_eps=1e-8)
    mf = int(_lib.sac_pop_layout(sp, P).member_floats)
    weights = torch.randn((P, mf), device=dev)
    snapshot = torch.zeros((P, mf), device=dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731

    def board_for(member_floats):
        b = _lib.Board(members=P, envs_per_member=M, env_base=0, lookback=args.lookback, cap=log.capacity,
                       member_floats=member_floats)
        need = C.c_int64()
        _lib.check(lib.sacenv_board_bytes(C.byref(b), C.byref(need)))
        buf = torch.zeros(need.value, dtype=torch.uint8, device=dev)
        _lib.check(lib.sacenv_board_init(C.byref(b), buf.data_ptr(), stream()))
        return b, buf

    plain, plain_buf = board_for(0)
    snap, snap_buf = board_for(mf)
    tied, tied_buf = board_for(mf)             # the board of the all-equal log
    flat_log = torch.empty_like(log.log)       # the same entries with equal scores: nobody ever saves

    def records(shape, i):
        if shape == "rollout":
            return rollouts[i % args.buffers]
        return rollouts[(i // K) % args.buffers][i % K: i % K + 1]

    out = {"what": "sacenv_board_update against sacenv_episodes_update on the same records "
                   "(tools/bench_scoreboard.py); us per call, device events around reps calls",
           "members": P, "envs_per_member": M, "envs": N, "steps": K, "lookback": args.lookback,
           "reps_per_window": R, "windows": args.windows, "member_floats": mf,
           "snapshot_bytes": 4 * P * mf, "shapes": {}}
    for shape in ("rollout", "step"):
        # fill: R scans, the total after each
        log.drain()
        totals = []
        for i in range(R):
            log.update(records(shape, i))
            torch.cuda.synchronize()
            totals.append(int(log._total.item()))
        assert totals[-1] <= log.capacity, "the benchmark's log overflowed"
        totals_dev = torch.tensor(totals, dtype=torch.int64, device=dev)
        flat_log.copy_(log.log)
        host = flat_log.cpu().numpy()
        host[32: 32 + 32 * totals[-1]].view(ENTRY_DTYPE)["score"] = 3.75
        flat_log.copy_(torch.from_numpy(host))
        flat_total = flat_log[:8].view(torch.int64)
        saved_calls = []

        def set_total(i, total=log._total):
            total.copy_(totals_dev[i: i + 1])

        def board(i, b=plain, buf=plain_buf, lg=log.log, total=log._total, w=None, s=None):
            set_total(i, total)
            _lib.check(lib.sacenv_board_update(C.byref(b), lg.data_ptr(), buf.data_ptr(), w, s, stream()))

        def rewind(b, buf):
            _lib.check(lib.sacenv_board_rewind(C.byref(b), buf.data_ptr(), stream()))

        res = {k: [] for k in ("scan", "copy_only", "board", "board_no_save", "board_all_save", "torch_copy")}
        board(R - 1)                            # warm-up: everything once
        rewind(plain, plain_buf)
        for _ in range(args.windows):
            res["copy_only"].append(_window(set_total, R))
            res["board"].append(_window(board, R))
            rewind(plain, plain_buf)
            res["board_no_save"].append(_window(
                lambda i: board(i, tied, tied_buf, flat_log, flat_total, weights.data_ptr(), snapshot.data_ptr()), R))
            torch.cuda.synchronize()
            rec = np.frombuffer(tied_buf.cpu().numpy().tobytes()[32: 32 + 128 * P], np.dtype("<i8"))
            saved_calls.append(int(rec.reshape(P, 16)[:, 1].sum()))        # saves so far: must stay 0
            rewind(tied, tied_buf)
            res["board_all_save"].append(_window(
                lambda i: board(i, snap, snap_buf, log.log, log._total, weights.data_ptr(), snapshot.data_ptr()), R))
            rewind(snap, snap_buf)
            res["torch_copy"].append(_window(lambda i: snapshot.copy_(weights), R))
        saves_real = int(np.frombuffer(snap_buf.cpu().numpy().tobytes()[32: 32 + 128 * P], "<i8")
                         .reshape(P, 16)[:, 1].sum())
        # the scan last: it appends to the log (drained between windows, as bench_episodes does)
        for _ in range(args.windows):
            log.drain()
            res["scan"].append(_window(lambda i: log.update(records(shape, i)), R))
        log.drain()
        per_call = np.diff([0] + totals)
        r = {k: _stats(v) for k, v in res.items()}
        net = {k: r[k]["median"] - r["copy_only"]["median"] for k in ("board", "board_no_save", "board_all_save")}
        out["shapes"][shape] = {
            "steps_per_call": K if shape == "rollout" else 1,
            "episodes_per_call": {"mean": float(per_call.mean()), "min": int(per_call.min()), "max": int(per_call.max())},
            "us_per_call": r,
            "net_of_the_8B_copy_us": net,
            "saves_in_the_no_save_windows": saved_calls, "saves_on_the_real_scores": saves_real,
            "bar": "board_no_save (net) <= scan",
            "bar_met": bool(net["board_no_save"] <= r["scan"]["median"]),
            "snapshot_all_saving_us": net["board_all_save"] - net["board"],
            "torch_copy_us": r["torch_copy"]["median"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return out


if __name__ == "__main__":
    main()
