"""Time ``sacenv_frames_render`` (include/sacenv_frames.h) on the GPU.

A 501-row episode (max_steps 500) drawn at 320 x 240 with every = 1: 501 frames per call. Device
events around windows of repeated calls, after a warm-up; the median window is reported. In the
same script: a plain device copy of as many bytes as the call writes (F H W plus the map) between
one pair of buffers, which like the call's own output stays in the Infinity Cache; the same copy
over eight pairs in turn, which does not; a fill of as many bytes, which only writes, as the
call does; a call for one frame (what the two launches in front of the compose cost); and the
numpy restatement's time for the same frames on the host, the only baseline there is. The
frames are compared with the oracle's before anything is timed.

    python tools/bench_frames.py [--out profiles/frames_bench.json] [--windows 7] [--calls 2000]
        [--example [--example-iters 200]]

``--example`` also runs examples/train_population.py at 16 x 1024 with ``--keep-traces``, with and
without ``--render``, three times each in turn after one unrecorded run of each, and records ``ms_per_iter`` (the drawing happens after
the timed loop). There is no CPU path: without a GPU this fails.
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes as C
import importlib.util
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sac-agent_amd"), os.path.join(ROOT, "tests")]

ROWS, W, H, S = 501, 320, 240, 48
GOAL, TRACK = 3900.0, 800.0


def episode(rows: int):
    """A boat that weaves down the track to the goal, turning as it goes."""
    rng = np.random.default_rng(0)
    k = np.arange(rows, dtype=np.float64)
    obs = rng.random((rows, 11), np.float32)
    obs[:, 0] = k / (rows - 1)
    obs[:, 3] = 0.5 + 0.35 * np.sin(k / 23.0)
    obs[:, 6] = (0.08 * np.cos(k / 23.0)) % 1.0
    obs[:, 9] = 0.5 + 0.4 * np.sin(k / 7.0)
    return obs, np.sin(k / 9.0).astype(np.float32)


def windows(fn, n_windows: int, calls: int, warmup: int = 20) -> list:
    """µs per call of ``fn`` in each of ``n_windows`` windows of ``calls`` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return out


def run_example(iters: int) -> dict:
    spec = importlib.util.spec_from_file_location("train_population", os.path.join(ROOT, "examples", "train_population.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    got = {"keep_traces": [], "keep_traces_render": []}
    with tempfile.TemporaryDirectory() as d:
        for rep in range(-1, 3):   # (rep -1: one run of each that is not recorded, the process's first)
            for name, extra in (("keep_traces", []), ("keep_traces_render", ["--render", d])):
                torch.manual_seed(0)
                with contextlib.redirect_stdout(io.StringIO()):
                    out = mod.main(["--members", "16", "--envs-per-member", "1024", "--iters", str(iters),
                                    "--keep-traces", d] + extra)
                if rep >= 0:
                    got[name].append(out["ms_per_iter"])
                if extra and rep == 0:
                    got["frames_drawn"] = sum(r["frames"] for r in out["frames"])
    return {"members": 16, "envs_per_member": 1024, "iters": iters, "runs_per_arm": 3,
            "note": "after one unrecorded run of each, the two arms in turn", "ms_per_iter": got}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_bench.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--example", action="store_true")
    ap.add_argument("--example-iters", type=int, default=200)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames.py times a GPU: no HIP device is visible")
    import frames_oracle as fo
    from sacenv import _lib
    lib = _lib.load()
    render, = _lib.require(_lib.FRAMES_EXPORTS[1:], "sacenv_frames.h", lib)
    dev = torch.device("cuda")
    spec = fo.Spec(W, H, S, GOAL, TRACK)
    R = ROWS - 1
    p = _lib.Frames(width=W, height=H, strip=S, members=1, max_steps=R, rad=spec.rad, boat_len=spec.boat_len,
                    boat_half=spec.boat_half, x0=float(spec.x0), y0=float(spec.y0), scale_x=float(spec.sx),
                    scale_y=float(spec.sy), goal_line=GOAL, track_width=TRACK)
    from sacenv.frames import direction_table
    table = direction_table()                  # the host's own table; the oracle's frames use the oracle's
    C.memmove(p.dir, table.ctypes.data, table.nbytes)
    obs, act = episode(ROWS)
    members = torch.from_numpy(np.frombuffer(fo.pack_member(R, obs, act), np.uint8).copy()).to(dev)
    map_bytes = 4 * W * (H - S)
    point_bytes = fo.scratch_bytes(spec, R) - map_bytes      # the rows' and the strip columns' values
    scratch = torch.empty(point_bytes + map_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty((ROWS, H, W), dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(n=ROWS):
        _lib.check(render(C.byref(p), members.data_ptr(), 0, 0, 1, n, out.data_ptr(), scratch.data_ptr(), stream))

    call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = fo.render(spec, obs, act, list(range(ROWS)))
    oracle_s = time.perf_counter() - t0
    same = bool((out.cpu().numpy() == want).all())
    if not same:
        raise SystemExit("the device's frames differ from the oracle's: nothing timed")
    written = ROWS * H * W + map_bytes                          # the frames and the map; the 37 KB of rows' and
    pairs = [(torch.empty(written, dtype=torch.uint8, device=dev),   # columns' values are listed beside them
              torch.empty(written, dtype=torch.uint8, device=dev)) for _ in range(8)]
    src, dst = pairs[0]
    turn = [0]

    def copy_rotating():   # eight pairs in turn, 620 MB in all: more than the 256 MiB Infinity Cache holds
        a, b = pairs[turn[0] & 7]
        turn[0] += 1
        b.copy_(a)

    # the call and its yardsticks in turn, so that all see the same machine
    full, copy, rot, fill, one = [], [], [], [], []
    for _ in range(args.windows):
        full += windows(call, 1, args.calls)
        copy += windows(lambda: dst.copy_(src), 1, args.calls)
        rot += windows(copy_rotating, 1, args.calls)
        fill += windows(lambda: dst.fill_(7), 1, args.calls)
        one += windows(lambda: call(1), 1, args.calls)
    us, us_copy, us_one = statistics.median(full), statistics.median(copy), statistics.median(one)
    us_rot, us_fill = statistics.median(rot), statistics.median(fill)
    res = {"what": "sacenv_frames_render, one call: 501 rows -> 501 frames of 320 x 240 (strip 48), every 1",
           "device": torch.cuda.get_device_name(0), "windows": args.windows, "calls_per_window": args.calls,
           "us_per_call": us, "us_per_call_windows": full, "launches_per_call": 3, "us_per_launch": us / 3,
           "us_per_call_one_frame": us_one, "us_per_frame": us / ROWS,
           "bytes_written": {"frames": ROWS * H * W, "map": map_bytes, "total": written,
                             "rows_and_columns_not_in_total": point_bytes},
           "write_gb_per_s": written / us * 1e-3,
           "copy_us": us_copy, "copy_gb_per_s_written": written / us_copy * 1e-3,
           "fraction_of_copy_rate": us_copy / us,
           "copy_note": "one pair of buffers copied again and again: `total` bytes read and as many written per copy, "
                        "a working set of two times `total` that the 256 MiB Infinity Cache holds, as it holds "
                        "the call's own output; copy_rotating takes eight pairs in turn (16 x `total`, more than "
                        "the cache holds); fill writes `total` bytes and reads none, as the call's stores do",
           "copy_rotating_us": us_rot, "copy_rotating_gb_per_s_written": written / us_rot * 1e-3,
           "fraction_of_copy_rotating_rate": us_rot / us,
           "fill_us": us_fill, "fill_gb_per_s": written / us_fill * 1e-3, "fraction_of_fill_rate": us_fill / us,
           "pixel_segment_tests_upper_bound": W * (H - S) * (ROWS - 1),
           "oracle_numpy_s": oracle_s, "oracle_over_device": oracle_s * 1e6 / us, "matches_oracle": same}
    if args.example:
        res["example"] = run_example(args.example_iters)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
