"""Episode frames on the device (include/sacenv_frames.h, sacenv/frames.py), byte for byte against
the numpy restatement (tests/frames_oracle.py), which tests/test_frames_cpu.py holds against
frames worked out by hand.

The kernel cases drive the C entry points through ctypes with member buffers written in numpy:
three members, the middle one drawn (the member offset), junk bytes behind the kept rows and in
the scratch (nothing but the kept rows is read, and all the scratch that is read is written).
Shapes are the smallest at which each mechanism can go wrong: 64 x 48 is whole 16 x 16 tiles,
68 x 52 is not; the coverage launch stages 128 segments at a time, so the row counts sit on both
sides of one chunk, past two, and at the buffer's end.
"""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import frames_oracle as fo
from conftest import ROOT

pytestmark = pytest.mark.gpu

R_MAX = 300                         # max_steps of the synthetic buffers: at most 301 rows
GOAL, TRACK = 3900.0, 800.0
SHAPES = {"64x48": (64, 48, 12), "68x52": (68, 52, 12)}
ROWS = (0, 1, 2, fo.CHUNK, fo.CHUNK + 1, fo.CHUNK + 2, 2 * fo.CHUNK + 2, R_MAX + 1)
KINDS = ("still", "wild", "headings", "nonfinite")


def _episode(kind: str, rows: int, seed: int):
    """(obs [rows, 11], action [rows]) of a made-up episode. `walk` wanders over the track and out
    of the window on every side, turning more than once around."""
    rng = np.random.default_rng(seed)
    obs = rng.random((rows, 11), np.float32)
    act = rng.uniform(-1, 1, rows).astype(np.float32)
    if rows == 0:
        return obs, act
    k = np.arange(rows, dtype=np.float64)
    if kind == "still":
        obs[:, 0], obs[:, 3], obs[:, 6] = 0.4, 0.55, 0.1
    elif kind == "wild":                       # jumps between points far outside the window and inside it
        obs[:, 0] = rng.choice([-0.6, -0.01, 0.3, 0.9, 1.12, 1.7], rows)
        obs[:, 3] = rng.choice([-0.7, -0.06, 0.2, 0.5, 1.07, 1.9], rows)
    else:
        obs[:, 0] = 0.5 + 0.75 * np.sin(k / 17.0) + 0.002 * k
        obs[:, 3] = 0.5 + 0.7 * np.cos(k / 11.0)
        obs[:, 6] = -1.3 + k / 39.7 if kind == "headings" else (k / 97.0) % 1.0
        obs[:, 9] = 0.5 + 0.5 * np.sin(k / 5.0)
    if kind == "nonfinite":
        bad = np.array([np.nan, np.inf, -np.inf], np.float32)
        for col in (0, 3, 6, 9):
            idx = rng.choice(rows, max(rows // 6, 1), replace=False)
            obs[idx, col] = rng.choice(bad, idx.size)
        idx = rng.choice(rows, max(rows // 6, 1), replace=False)
        act[idx] = rng.choice(bad, idx.size)
    return obs, act


class Dev:
    """Member buffers and a scratch on the device, drawn through the C entry points."""

    def __init__(self, gpu, lib, spec: fo.Spec, episodes, R=R_MAX, first_row=0):
        from sacenv import _lib
        self._lib, self.lib, self.gpu, self.s, self.P = _lib, lib, gpu, spec, len(episodes)
        s = spec
        self.params = _lib.Frames(width=s.W, height=s.H, strip=s.S, members=self.P, max_steps=R, rad=s.rad,
                                  boat_len=s.boat_len, boat_half=s.boat_half, x0=float(s.x0), y0=float(s.y0),
                                  scale_x=float(s.sx), scale_y=float(s.sy), goal_line=float(s.goal_line),
                                  track_width=float(s.track_width))
        ctypes.memmove(self.params.dir, s.dir.ctypes.data, s.dir.nbytes)
        sb, fb = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(lib.sacenv_frames_bytes(ctypes.byref(self.params), ctypes.byref(sb), ctypes.byref(fb)))
        assert sb.value == self.scratch_bytes() and fb.value == s.W * s.H
        raw = b"".join(fo.pack_member(R, o, a, first_row=first_row, junk=0xEE) for o, a in episodes)
        self.members = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(gpu)
        self.scratch = self.new_scratch()

    def scratch_bytes(self):
        return fo.scratch_bytes(self.s, self.params.max_steps)

    def new_scratch(self, fill=0xCD):
        return torch.full((self.scratch_bytes(),), fill, dtype=torch.uint8, device=self.gpu)

    def render(self, m, first, every, n, scratch=None) -> np.ndarray:
        out = torch.full((n, self.s.H, self.s.W), 0xFF, dtype=torch.uint8, device=self.gpu)
        scratch = self.scratch if scratch is None else scratch
        self._lib.check(self.lib.sacenv_frames_render(
            ctypes.byref(self.params), self.members.data_ptr(), m, first, every, n, out.data_ptr(),
            scratch.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(self.gpu).cuda_stream)))
        torch.cuda.synchronize(self.gpu)
        return out.cpu().numpy()


def _spec(shape, **kw):
    W, H, S = SHAPES[shape]
    return fo.Spec(W, H, S, GOAL, TRACK, **kw)


def _diff(got, want, ts) -> str:
    if got.shape == want.shape and (got == want).all():
        return ""
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    f, r, c = bad[0]
    return (f"{len(bad)} pixels differ in frames {sorted(set(bad[:, 0].tolist()))[:8]}; first at frame {f} "
            f"(step {ts[f]}) row {r} column {c}: {got[f, r, c]} != {want[f, r, c]}")


_ORACLE = {}


def _oracle(shape, kind, rows, seed):
    """The oracle's frames of every step of an episode, computed once and never changed."""
    key = (shape, kind, rows, seed)
    if key not in _ORACLE:
        obs, act = _episode(kind, rows, seed)
        full = fo.render(_spec(shape), obs, act, list(range(rows)) if rows else [-1])
        full.setflags(write=False)
        _ORACLE[key] = (obs, act, full)
    return _ORACLE[key]


def _check(gpu, lib, shape, kind, rows, seed=1, everys=(1, 7), first_row=0):
    obs, act, full = _oracle(shape, kind, rows, seed)
    others = (_episode("walk", 40, seed + 100), _episode("wild", 9, seed + 200))
    dev = Dev(gpu, lib, _spec(shape), [others[0], (obs, act), others[1]], first_row=first_row)
    for every in everys:
        n = (max(rows - 1, 0) + every - 1) // every + 1
        ts = fo.frame_ts(rows, 0, every, n + 2)                  # two frames past the end
        got = dev.render(1, 0, every, n + 2)
        d = _diff(got, full[[max(t, 0) for t in ts]], ts)
        assert not d, f"{shape} {kind} rows {rows} every {every}: {d}"
        if rows:
            assert ts[-3:] == [rows - 1] * 3 and (got[-1] == got[-3]).all()
    return dev, full


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_row_counts_against_the_oracle(gpu, built_lib, shape, rows):
    dev, full = _check(gpu, built_lib, shape, "walk", rows)
    if rows == 0:
        s = dev.s
        assert (full[0, : s.HP] == fo.background(s)).all() and not np.isin(full, (fo.PATH, fo.BOAT, fo.CURSOR)).any()
    if rows > 2:
        assert (full[-1] == fo.PATH).sum() > 20 and (full == fo.BOAT).any()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_other_paths_against_the_oracle(gpu, built_lib, shape, kind):
    rows = fo.CHUNK + 12
    _, full = _check(gpu, built_lib, shape, kind, rows)
    obs, act, _ = _oracle(shape, kind, rows, 1)
    p = fo.points(_spec(shape), obs, act)
    W, H, S = SHAPES[shape]
    if kind == "still":
        disc = fo.coverage(_spec(shape), p["X"], p["Y"]) == 1     # (a pixel centre is within 0.71 px of any point)
        assert len(set(zip(p["X"].tolist(), p["Y"].tolist()))) == 1 and 0 < disc.sum() < 6
    if kind == "wild":                         # the path leaves the window on every side
        assert p["X"].min() < 0 and p["X"].max() > 16 * W and p["Y"].min() < 0 and p["Y"].max() > 16 * (H - S)
    if kind == "headings":
        assert obs[:, 6].min() < -1 and obs[:, 6].max() > 2 and len(set(p["hd"].tolist())) > 100
    if kind == "nonfinite":
        assert not np.isfinite(obs[:, [0, 3, 6, 9]]).all(axis=0).any() and not np.isfinite(act).all()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_truncated_episode_starts_at_its_first_kept_row(gpu, built_lib, shape):
    _check(gpu, built_lib, shape, "walk", 50, everys=(3,), first_row=17)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_split_calls_and_a_shared_scratch(gpu, built_lib, shape):
    """Frames [0, F) in one call are the frames of [0, a) and [a, F); a scratch that has just
    drawn another member (longer, elsewhere) gives the same frames as a fresh one."""
    every = 2
    eps = [_episode("walk", 290, 5), _episode("wild", 140, 6), _episode("walk", 0, 7)]
    dev = Dev(gpu, built_lib, _spec(shape), eps)
    F = 75
    whole = dev.render(1, 0, every, F)
    for a in (1, 33, 74):
        parts = np.concatenate([dev.render(1, 0, every, a), dev.render(1, a, every, F - a)])
        assert (parts == whole).all(), a
    want = fo.render(_spec(shape), *eps[1], fo.frame_ts(140, 0, every, F))
    assert not _diff(whole, want, fo.frame_ts(140, 0, every, F))
    for m, n in ((0, 290), (2, 0), (1, 140)):                      # one scratch, member after member
        ts = fo.frame_ts(n, 3, 5, 30)
        used = dev.render(m, 3, 5, 30)
        fresh = dev.render(m, 3, 5, 30, scratch=dev.new_scratch(0x11))
        assert (used == fresh).all(), m
        want = fo.render(_spec(shape), *eps[m], ts)
        assert not _diff(used, want, ts), m


def test_the_default_frame_and_other_sizes(gpu, built_lib):
    """320 x 240 with a 48-row strip, and a frame with a wider path and a larger boat."""
    eps = [_episode("walk", 60, 9)]
    for spec in (fo.Spec(320, 240, 48, GOAL, TRACK), fo.Spec(96, 80, 20, GOAL, TRACK, rad=40, boat_len=200, boat_half=90,
                                                            window=(-300.0, 2500.0, -500.0, 900.0))):
        dev = Dev(gpu, built_lib, spec, eps, R=64)
        ts = fo.frame_ts(60, 0, 4, 16)
        got = dev.render(0, 0, 4, 16)
        assert not _diff(got, fo.render(spec, *eps[0], ts), ts)


# ---- the real env

P_REAL, N_REAL, T_REAL, MAX_STEPS = 2, 64, 80, 24


@pytest.fixture(scope="module")
def real_traces(gpu, built_lib):
    from sacenv import BestEpisodes, VecBoatEnv
    env = VecBoatEnv({"base_settings": {"experiment": 6, "test_mode": 0}}, P_REAL * N_REAL, seed=0, device=gpu,
                     max_episode_steps=MAX_STEPS)
    env.reset()
    traces = BestEpisodes(env, members=P_REAL, envs_per_member=N_REAL)
    rng = np.random.default_rng(21)
    acts = torch.from_numpy(rng.uniform(-1, 1, (T_REAL, P_REAL * N_REAL)).astype(np.float32)).to(gpu)
    for k in range(T_REAL):
        env.step(acts[k])
        traces.update(acts[k])
    return traces


def _real_spec(traces, frames):
    cfg = traces.env.cfg
    return fo.Spec(frames.W, frames.H, frames.S, float(cfg.goal_line), float(cfg.track_width))


@pytest.mark.parametrize("every", [1, 3])
def test_real_env_against_the_oracle(real_traces, every):
    from sacenv import EpisodeFrames
    frames = EpisodeFrames(real_traces, every=every)
    assert (frames.W, frames.H, frames.S) == (320, 240, 48)
    spec = _real_spec(real_traces, frames)
    for m in range(P_REAL):
        b = real_traces.best(m)
        assert b is not None and b["rows"] >= 2
        ts = frames.frame_steps(m)
        assert ts[0] == 0 and ts[-1] == b["rows"] - 1 and ts == sorted(set(range(0, b["rows"], every)) | {b["rows"] - 1})
        got = frames.render(m)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (len(ts), 240, 320) and got.device == real_traces.device
        want = fo.render(spec, b["obs"], b["action"], ts)
        assert not _diff(got.cpu().numpy(), want, ts), m
        part = frames.render(m, first=1, count=2)
        assert (part.cpu().numpy() == want[[min(1, len(ts) - 1), min(2, len(ts) - 1)]]).all()
        rgb = frames.rgb(got[:2])
        assert tuple(rgb.shape) == (2, 240, 320, 3) and (rgb.cpu().numpy() == frames.rgb(want[:2])).all()
    with pytest.raises(IndexError):
        frames.render(P_REAL)
    with pytest.raises(ValueError, match="max_bytes"):
        EpisodeFrames(real_traces, max_bytes=1 << 20).render(0, count=64)


def _indices(im, palette):
    """A GIF frame's palette indices, through its colours (Pillow may hand later frames out as RGB)."""
    lut = {(int(r) << 16) | (int(g) << 8) | int(b): i for i, (r, g, b) in enumerate(palette.tolist())}
    rgb = np.asarray(im.convert("RGB")).astype(np.int64)
    key = (rgb[..., 0] << 16) | (rgb[..., 1] << 8) | rgb[..., 2]
    return np.vectorize(lut.__getitem__, otypes=[np.uint8])(key)


def _gif_frames(path, palette, ms=40) -> np.ndarray:
    """The index frames a GIF shows, one per ``ms``: Pillow writes a run of identical frames as one
    frame that lasts as long as the run."""
    from PIL import Image
    out = []
    with Image.open(path) as im:
        for i in range(im.n_frames):
            im.seek(i)
            assert im.info["duration"] % ms == 0
            out += [_indices(im, palette)] * (im.info["duration"] // ms)
    return np.stack(out)


def test_save_gif_is_lossless(real_traces, tmp_path):
    pytest.importorskip("PIL")
    from sacenv import EpisodeFrames
    from sacenv.frames import PALETTE
    frames = EpisodeFrames(real_traces, width=96, height=64, strip=16, every=2)
    assert frames.save_gif(str(tmp_path)) == [0, 1]
    for m in range(P_REAL):
        want = frames.render(m).cpu().numpy()
        got = _gif_frames(tmp_path / f"member_{m}" / "rendering" / "episode_0.gif", PALETTE)
        assert len(want) == len(frames.frame_steps(m)) > 2
        assert got.shape == want.shape and (got == want).all(), m


def _example():
    spec = importlib.util.spec_from_file_location("train_population",
                                                  os.path.join(ROOT, "examples", "train_population.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


PLAIN_KEYS = ["pipeline", "replay", "noise", "members", "envs_per_member", "iters", "batch", "env_steps_per_s",
              "ms_per_iter", "losses", "table"]


def test_the_example_renders(gpu, built_lib, tmp_path, capsys):
    """``--render DIR``: a GIF per member that finished an episode, one printed line, and the JSON
    line gains ``frames`` alone; without the flag the JSON line has the keys it had before."""
    pytest.importorskip("PIL")
    from sacenv.frames import PALETTE
    args = ["--members", "2", "--envs-per-member", "64", "--iters", "60", "--batch", "256", "--max-episode-steps", "20"]
    out_dir = tmp_path / "best"
    torch.manual_seed(5)
    out = _example().main(args + ["--keep-traces", str(out_dir), "--render", str(out_dir), "--render-every", "4"])
    printed = capsys.readouterr().out
    line = json.loads(printed.strip().split("\n")[-1])
    assert list(out) == list(line) == PLAIN_KEYS + ["traces", "frames"]
    assert line["frames"] == out["frames"] and len(out["frames"]) == 2
    assert f"frames of members [0, 1] in {out_dir}" in printed
    for row, trace in zip(out["frames"], out["traces"]):
        assert row["member"] == trace["member"] and row["frames"] == (trace["rows"] - 2) // 4 + 2
        assert row["file"] == str(out_dir / f"member_{row['member']}" / "rendering" / "episode_0.gif")
        assert _gif_frames(row["file"], PALETTE).shape == (row["frames"], 240, 320)
    torch.manual_seed(5)
    kept = _example().main(args + ["--keep-traces", str(tmp_path / "kept")])
    assert list(kept) == PLAIN_KEYS + ["traces"] and kept["traces"] == out["traces"]
    assert "frames of members" not in capsys.readouterr().out
    torch.manual_seed(5)
    plain = _example().main(args)
    assert list(plain) == PLAIN_KEYS
    with pytest.raises(SystemExit):
        _example().main(args + ["--render", str(out_dir)])
