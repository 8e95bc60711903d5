"""Episode frames without a GPU (include/sacenv_frames.h, tests/frames_oracle.py).

* the header's functions are ``_lib.FRAMES_EXPORTS``, beside every older list; the build still has
  ten units and lists the two new headers;
* the descriptor has the layout of its ctypes mirror;
* every argument error is found on the host, before anything is launched;
* the numpy restatement against frames worked out by hand on a 16 x 16 frame, against exact
  rational distances, and its int64 arithmetic against Python's integers at the extremes;
* the direction table.
"""
import ctypes
import itertools
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import frames_oracle as fo
from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "sacenv_frames.h")
E_NULL, E_SIZE, E_RANGE = -1, -4, -5


def _frames(**kw):
    from sacenv import _lib
    base = dict(width=64, height=48, strip=12, members=3, max_steps=40, rad=12, boat_len=96, boat_half=48,
                x0=-5.0, y0=880.0, scale_x=0.25, scale_y=0.5, goal_line=3900.0, track_width=800.0)
    base.update(kw)
    return _lib.Frames(**base)


def test_header_and_exports(built_lib):
    from sacenv import _build, _lib
    src = open(HEADER).read()
    names = set(re.findall(r"\b(sacenv_\w+)\s*\(", src))
    assert names == set(_lib.FRAMES_EXPORTS) and len(_lib.FRAMES_EXPORTS) == 2
    for older in (_lib.EXPORTS, _lib.EPISODE_EXPORTS, _lib.POPULATION_EXPORTS, _lib.REPLAY_POP_EXPORTS,
                  _lib.NOISE_EXPORTS, _lib.SCOREBOARD_EXPORTS, _lib.SELECTION_EXPORTS, _lib.TRACES_EXPORTS):
        assert not names & set(older)
    for n in names:
        assert hasattr(built_lib, n), n

    def define(name):
        return int(re.search(rf"#define SACENV_FRAMES_{name} (\d+)\b", src).group(1))

    assert define("VERSION") == _lib.FRAMES_VERSION == 1
    assert (define("MIN_DIM"), define("MAX_DIM")) == (_lib.FRAMES_MIN_DIM, _lib.FRAMES_MAX_DIM) == (16, 1024)
    assert define("MAX_FRAMES") == _lib.FRAMES_MAX_FRAMES
    assert (define("MAX_RAD"), define("MAX_BOAT")) == (_lib.FRAMES_MAX_RAD, _lib.FRAMES_MAX_BOAT)
    assert define("CHUNK") == _lib.FRAMES_CHUNK == fo.CHUNK
    assert define("WATER") == _lib.FRAMES_WATER == fo.WATER == 32
    for name in ("OUTSIDE", "BOUNDARY", "GOAL", "PATH", "BOAT", "STRIP", "ZERO", "RUDDER", "ACTION", "CURSOR",
                 "COLOURS"):
        assert define(name) == getattr(_lib, "FRAMES_" + name) == getattr(fo, name), name
    assert _lib.FRAMES_COLOURS < 256
    assert _lib.ABI_VERSION == 20 == built_lib.sacenv_abi_version()        # sacenv.h is untouched
    assert len(_build.SOURCES) == 10                                       # no new translation unit
    rel = [r for r, _ in _build.deps()]
    assert os.path.join("include", "sacenv_frames.h") in rel and "sacenv_frames.h" in _build.PUBLIC_HEADERS
    assert os.path.join("sac-agent_amd", "csrc", "sacenv_traces_frames.h") in rel
    assert "sacenv_traces_frames.h" in _build.HEADERS
    unit = open(os.path.join(_build.CSRC, "sacenv_traces.hip")).read()
    assert '#include "sacenv_traces_frames.h"' in unit
    topic = open(os.path.join(_build.CSRC, "sacenv_traces_frames.h")).read()
    assert not re.search(r"atomic\w*\s*\(", topic) and not re.search(r"\b(sinf|cosf|sincosf)\s*\(", topic)
    import sacenv
    from sacenv.frames import PALETTE, EpisodeFrames
    assert sacenv.EpisodeFrames is EpisodeFrames and "EpisodeFrames" in sacenv.__all__
    assert PALETTE.shape == (_lib.FRAMES_COLOURS, 3) and len({tuple(c) for c in PALETTE.tolist()}) == len(PALETTE)


def test_struct_matches_c_layout(tmp_path):
    """offsetof / sizeof of SacenvFrames, from gcc on the header, against the ctypes mirror."""
    from sacenv import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sacenv_frames.h"', "int main(void) {",
             'printf("SacenvFrames %zu\\n", sizeof(SacenvFrames));']
    for fname, _ in _lib.Frames._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(SacenvFrames, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[0]: int(l.split()[1]) for l in out if l.strip()}
    assert got["SacenvFrames"] == ctypes.sizeof(_lib.Frames) == 32 + 24 + 1024
    for fname, _ in _lib.Frames._fields_:
        assert got[fname] == getattr(_lib.Frames, fname).offset, fname
    assert _lib.Frames.dir.offset == 56 and _lib.Frames.dir.size == 1024


def test_argument_errors_are_found_on_the_host(built_lib):
    """Each error returns its code before anything is launched (no device here): pointers are
    made-up addresses that are never followed."""
    lib = built_lib
    sb, fb = ctypes.c_int64(-7), ctypes.c_int64(-7)
    good, p = _frames(), 0x10000
    R = ctypes.byref

    def render(f, member_buf=p, member=1, first=0, every=1, n=4, out=p, scratch=p):
        return lib.sacenv_frames_render(None if f is None else R(f), member_buf, member, first, every, n, out,
                                        scratch, None)

    assert lib.sacenv_frames_bytes(R(good), R(sb), R(fb)) == 0
    assert sb.value == 16 + 64 * 41 + 16 * 64 + 4 * 64 * 36 and fb.value == 64 * 48
    assert lib.sacenv_frames_bytes(None, R(sb), R(fb)) == E_NULL
    assert lib.sacenv_frames_bytes(R(good), None, R(fb)) == E_NULL
    assert lib.sacenv_frames_bytes(R(good), R(sb), None) == E_NULL
    size = [dict(width=12), dict(width=1028), dict(width=66), dict(height=15), dict(height=1025), dict(strip=1),
            dict(strip=41), dict(members=0), dict(members=65), dict(max_steps=0), dict(max_steps=(1 << 20) + 1),
            dict(rad=0), dict(rad=257), dict(boat_len=0), dict(boat_len=1025), dict(boat_half=0),
            dict(boat_half=1025)]
    for kw in size:
        f = _frames(**kw)
        assert lib.sacenv_frames_bytes(R(f), R(sb), R(fb)) == E_SIZE, kw
        assert render(f) == E_SIZE, kw
    nan, inf = float("nan"), float("inf")
    rng = [dict(scale_x=0.0), dict(scale_y=-1.0), dict(scale_x=nan), dict(scale_y=inf), dict(x0=nan), dict(y0=-inf),
           dict(goal_line=nan), dict(track_width=inf)]
    for kw in rng:
        f = _frames(**kw)
        assert lib.sacenv_frames_bytes(R(f), R(sb), R(fb)) == E_RANGE, kw
        assert render(f) == E_RANGE, kw
    assert sb.value == 16 + 64 * 41 + 16 * 64 + 4 * 64 * 36
    assert render(None) == E_NULL
    for kw in (dict(member_buf=None), dict(out=None), dict(scratch=None)):
        assert render(good, **kw) == E_NULL, kw
    for kw in (dict(member=-1), dict(member=3), dict(every=0), dict(every=-2), dict(n=0), dict(n=(1 << 20) + 1)):
        assert render(good, **kw) == E_SIZE, kw
    for kw in (dict(first=-1), dict(first=(1 << 62) + 1), dict(member_buf=p + 8), dict(scratch=p + 4),
               dict(out=p + 2)):
        assert render(good, **kw) == E_RANGE, kw
    # the limits themselves pass
    for kw in (dict(width=16, height=16, strip=4), dict(width=1024, height=1024, strip=1016), dict(members=64),
               dict(max_steps=1 << 20), dict(rad=256, boat_len=1024, boat_half=1024)):
        assert lib.sacenv_frames_bytes(R(_frames(**kw)), R(sb), R(fb)) == 0, kw


def test_lib_loads_a_library_without_the_frames_entry_points(built_lib, tmp_path):
    """``SACENV_LIB`` may point at a build from before sacenv_frames.h; ``require`` then says what to do."""
    from sacenv import _lib
    older = (_lib.EXPORTS + _lib.EPISODE_EXPORTS + _lib.POPULATION_EXPORTS + _lib.REPLAY_POP_EXPORTS +
             _lib.NOISE_EXPORTS + _lib.SCOREBOARD_EXPORTS + _lib.SELECTION_EXPORTS + _lib.TRACES_EXPORTS)
    body = ["int sacenv_abi_version(void) { return %d; }" % _lib.ABI_VERSION]
    body += [f"int {n}(void) {{ return 0; }}" for n in older if n != "sacenv_abi_version"]
    src = tmp_path / "old.c"
    src.write_text("\n".join(body))
    so = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = _lib.load(str(so))
    assert not any(hasattr(lib, n) for n in _lib.FRAMES_EXPORTS) and all(hasattr(lib, n) for n in _lib.TRACES_EXPORTS)
    with pytest.raises(_lib.SacenvError, match="sacenv_frames.h"):
        _lib.require(_lib.FRAMES_EXPORTS, "sacenv_frames.h", lib)
    assert [f.__name__ for f in _lib.require(_lib.FRAMES_EXPORTS, "sacenv_frames.h")] == list(_lib.FRAMES_EXPORTS)


def test_the_host_class_refuses_what_it_cannot_draw():
    from sacenv.frames import EpisodeFrames
    with pytest.raises(ValueError, match="BestEpisodes"):
        EpisodeFrames(object())


# ---- the oracle against frames worked out by hand: 16 x 16, a 4-row strip, one pixel per world
# unit (window x 0 .. 16, y -6 .. 6: both scales are 16), goal_line 8 and track_width 4, so that
# x = 8 obs[0] and y = 8 obs[3] - 4 are exact

def _spec(**kw):
    base = dict(window=(0, 16, -6, 6), rad=20, boat_len=32, boat_half=16)
    base.update(kw)
    return fo.Spec(16, 16, 4, 8.0, 4.0, **base)


def _row(px, py, heading=0.0, rudder=0.5):
    """The obs of a boat at the fixed-point position (16 px, 16 py): pixel units from the panel's
    top left."""
    o = np.zeros(11, np.float32)
    o[0], o[3], o[6], o[9] = px / 8.0, (6.0 - py + 4.0) / 8.0, heading, rudder
    return o


def _set(mask):
    return {(int(r), int(c)) for r, c in np.argwhere(mask)}


def test_the_spec_and_the_background_by_hand():
    s = _spec()
    assert (s.sx, s.sy, s.x0, s.y0, s.HP) == (16.0, 16.0, 0.0, 6.0, 12)
    p = fo.points(s, [_row(4.5, 5.5)], [0.0])
    assert (p["X"][0], p["Y"][0], p["hd"][0]) == (72, 88, 0)
    # y = 0 is 6 px from the top: row 6 is the centre line; y = +-4: rows 2 and 10; x = 8: column 8
    bg = fo.background(s)
    assert bg.shape == (12, 16)
    assert (bg[[0, 1, 11]] == np.where(np.arange(16) == 8, fo.GOAL, fo.OUTSIDE)).all()
    assert (bg[[2, 10]] == np.where(np.arange(16) == 8, fo.GOAL, fo.BOUNDARY)).all()
    # water: |r - 6| * 64 // 12
    for r in range(3, 10):
        assert (np.delete(bg[r], 8) == abs(r - 6) * 64 // 12).all() and bg[r, 8] == fo.GOAL


def test_one_row_is_a_boat_and_no_path():
    """rows = 1, heading 0, the boat's point at (72, 88): V0 = (104, 88), V1 = (56, 72), V2 = (56, 104).
    Pixel centres inside, edges included: the stern column x = 56 at y = 72, 88, 104; the axis
    y = 88 at x = 72, 88, 104."""
    s = _spec()
    f = fo.render(s, [_row(4.5, 5.5)], [0.0], [0])[0]
    assert fo.boat_vertices(s, 72, 88, 0) == [(104, 88), (56, 72), (56, 104)]
    assert _set(f == fo.BOAT) == {(4, 3), (5, 3), (6, 3), (5, 4), (5, 5), (5, 6)}
    assert not (f == fo.PATH).any()
    assert (fo.coverage(s, [72], [88]) == fo.NONE).all()
    # the strip: action 0 -> rint(0.5 * 3) = 2, rudder 0.5 -> 0 -> row 2 as well; the cursor at column 0
    strip = f[12:]
    assert (strip[:, 0] == fo.CURSOR).all()
    assert (strip[2, 1:] == fo.ACTION).all() and (strip[1, 1:] == fo.ZERO).all()
    assert (strip[[0, 3], 1:] == fo.STRIP).all()
    # an empty member: the background alone
    e = fo.render(s, np.zeros((0, 11)), [], [-1])[0]
    assert (e[:12] == fo.background(s)).all() and (e[12:] == np.where(np.arange(4)[:, None] == 1, fo.ZERO, fo.STRIP)).all()


def test_a_horizontal_segment_by_hand():
    """rows = 2, from (72, 88) to (168, 88) with rad 20: on its own row (y = 88) the centres from
    x = 56 to 184 (|dx| <= 20 past the ends: columns 3 .. 11); on the rows beside it (16 away)
    the centres between the ends (columns 4 .. 10); at the corners 16^2 + 16^2 > 20^2."""
    s = _spec()
    obs, act = [_row(4.5, 5.5), _row(10.5, 5.5)], [0.0, 1.0]
    want = {(5, c) for c in range(3, 12)} | {(r, c) for r in (4, 6) for c in range(4, 11)}
    first = fo.coverage(s, [72, 168], [88, 88])
    assert _set(first == 1) == want and _set(first == fo.NONE) == _set(np.ones((12, 16), bool)) - want
    f0, f1 = fo.render(s, obs, act, [0, 1])
    assert not (f0 == fo.PATH).any()
    boat = _set(f1 == fo.BOAT)
    assert boat == {(4, 9), (5, 9), (6, 9), (5, 10), (5, 11), (5, 12)}                # the boat at (168, 88)
    assert _set(f1 == fo.PATH) == want - boat
    # the strip: column c shows row (c * 1) // 15: row 1 only in column 15; action 1 -> strip row 0
    assert (f1[12:, 15] == fo.CURSOR).all() and (f0[12:, 0] == fo.CURSOR).all()
    assert (f1[12 + 2, :15] == fo.ACTION).all() and (f0[12 + 2, 1:15] == fo.ACTION).all()
    assert (f0[12:, 15] == np.array([fo.STRIP, fo.ZERO, fo.STRIP, fo.STRIP])).all()   # row 1 is not shown yet


def test_a_zero_length_segment_is_a_disc():
    s = _spec()
    first = fo.coverage(s, [72, 72], [88, 88])
    cy, cx = np.meshgrid(16 * np.arange(12) + 8, 16 * np.arange(16) + 8, indexing="ij")
    assert _set(first == 1) == _set((cx - 72) ** 2 + (cy - 88) ** 2 <= 400) == {(5, 4), (4, 4), (6, 4), (5, 3), (5, 5)}


def test_headings():
    """0.25 points up the screen (y is flipped): V0 = (72, 56), V1 = (56, 104), V2 = (88, 104);
    1.25 is the same index, -0.75 too; -0.25 points down."""
    s = _spec()
    assert fo.boat_vertices(s, 72, 88, 64) == [(72, 56), (56, 104), (88, 104)]
    frames = [fo.render(s, [_row(4.5, 5.5, h)], [0.0], [0])[0] for h in (0.0, 0.25, 1.25, -0.75, -0.25)]
    up = {(6, 3), (6, 4), (6, 5), (5, 4), (4, 4), (3, 4)}
    assert _set(frames[1] == fo.BOAT) == up
    assert (frames[1] == frames[2]).all() and (frames[1] == frames[3]).all()
    assert _set(frames[4] == fo.BOAT) == {(10 - r, c) for r, c in up}                 # mirrored in y = 88
    assert _set(frames[0] == fo.BOAT) != up
    hd = fo.points(s, [_row(0, 0, h) for h in (0.0, 0.25, 1.25, -0.75, -0.25, 1e30, -1e30)], np.zeros(7))["hd"]
    assert hd.tolist() == [0, 64, 64, 64, 192, 0, 0]


def test_non_finite_values_are_clamped():
    s = _spec()
    nan, inf = np.float32("nan"), np.float32("inf")
    obs = np.stack([_row(4.5, 5.5)] * 6)
    obs[1, 0], obs[2, 0], obs[3, 3], obs[4, 3], obs[5, [0, 3, 6, 9]] = inf, -inf, inf, -inf, nan
    act = np.array([0.0, inf, -inf, nan, 5.0, -5.0], np.float32)
    p = fo.points(s, obs, act)
    assert p["X"].tolist() == [72, 16 * 16 + 1024, -1024, 72, 72, -1024]
    assert p["Y"].tolist() == [88, 88, 88, -1024, 16 * 12 + 1024, -1024]           # y = +inf is above the top
    assert p["hd"][5] == 0 and p["rrow"][5] == 0
    assert p["arow"].tolist() == [2, 0, 3, 0, 0, 3]                                  # -inf -> (1 + inf) -> the last row
    f = fo.render(s, obs, act, list(range(6)))
    assert f.shape == (6, 16, 16) and f.max() < fo.COLOURS


def test_the_prefix_property():
    rng = np.random.default_rng(3)
    s = _spec(rad=12)
    rows = 23
    obs = rng.random((rows, 11), np.float32) * 1.6 - 0.3
    act = rng.uniform(-1, 1, rows).astype(np.float32)
    p = fo.points(s, obs, act)
    first = fo.coverage(s, p["X"], p["Y"])
    frames = fo.render(s, obs, act, list(range(rows)))
    before = set()
    for t in range(rows):
        panel = frames[t, :12]
        assert ((panel == fo.PATH) == ((first <= t) & (panel != fo.BOAT))).all(), t
        shown = _set(first <= t)
        assert before <= shown
        before = shown
        # and from first principles: some segment 1 .. t covers the pixel
        again = fo.coverage(s, p["X"][: t + 1], p["Y"][: t + 1])
        assert ((again != fo.NONE) == (first <= t)).all() and (again[again != fo.NONE] == first[first <= t]).all()
    assert len(before) > 20


def test_coverage_against_exact_rational_distances():
    """The three-way integer test is `squared distance to the segment <= rad^2`, held against
    the distance computed with fractions."""
    rng = np.random.default_rng(11)
    s = _spec(rad=12)
    X, Y = rng.integers(-40, 300, 7).tolist(), rng.integers(-40, 240, 7).tolist()
    X[3], Y[3] = X[2], Y[2]                                                          # a zero-length one
    first = fo.coverage(s, X, Y)
    for r in range(12):
        for c in range(16):
            cx, cy, want = 16 * c + 8, 16 * r + 8, fo.NONE
            for j in range(1, 7):
                ax, ay, dx, dy = X[j - 1], Y[j - 1], X[j] - X[j - 1], Y[j] - Y[j - 1]
                dd = dx * dx + dy * dy
                u = Fraction(0) if dd == 0 else min(max(Fraction((cx - ax) * dx + (cy - ay) * dy, dd), 0), 1)
                d2 = (cx - ax - u * dx) ** 2 + (cy - ay - u * dy) ** 2
                if d2 <= 144:
                    want = j
                    break
            assert first[r, c] == want, (r, c)
    assert (first != fo.NONE).sum() > 10


def test_int64_is_enough_at_the_extremes():
    """Every combination of extreme clamped coordinates at W = H = 1024 (-1024 and 16 * 1024 +
    1024, their neighbours and the middle) with extreme pixel centres and radii: int64 arithmetic
    decides as Python's integers do, the dot and cross products fit an int32 and the squared
    cross product stays below 2^59."""
    hi = 16 * 1024 + 1024
    vals, cvals = [-1024, -1023, 0, 8192, hi - 1, hi], [8, 8200, 16 * 1023 + 8]
    combos = np.array(list(itertools.product(vals, vals, vals, vals, cvals, cvals)), np.int64)
    ax, ay, bx, by, cx, cy = combos.T
    dx, dy, px, py = bx - ax, by - ay, cx - ax, cy - ay
    assert max(np.abs(v).max() for v in (dx, dy, px, py)) <= 18432 < 2 ** 14.2
    for v in (px * dx + py * dy, dx * dx + dy * dy, px * dy - py * dx, px * px + py * py):
        assert np.abs(v).max() <= 2 * 18432 ** 2 < 2 ** 29.4 < 2 ** 31
    assert int(np.abs(px * dy - py * dx).max()) ** 2 < 2 ** 59
    for rad in (1, 12, 256):
        got = fo.covers(ax, ay, bx, by, cx, cy, np.int64(rad))
        want = [fo.covers(*(int(v) for v in row), rad) for row in combos]
        assert got.tolist() == want and rad * rad * 2 * 18432 ** 2 < 2 ** 46
    assert 0 < sum(want) < len(want)


def test_the_direction_table():
    from sacenv.frames import direction_table
    d = fo.direction_table()
    assert d.dtype == np.int16 and d.shape == (256, 2) and (d == direction_table()).all()
    k = np.arange(256)
    exact = 1024 * np.stack([np.cos(2 * np.pi * k / 256), np.sin(2 * np.pi * k / 256)], 1)
    assert np.abs(d - exact).max() <= 0.5 + 1e-9
    norm = np.hypot(d[:, 0].astype(float), d[:, 1].astype(float))
    assert np.abs(norm - 1024).max() <= 1
    assert d[0].tolist() == [1024, 0] and d[64].tolist() == [0, 1024] and d[32, 0] == d[32, 1] == 724
    d = d.astype(int)
    assert (d[(k + 64) % 256] == np.stack([-d[:, 1], d[:, 0]], 1)).all()             # a quarter turn
    assert (d[(k + 128) % 256] == -d).all()                                          # a half turn
    assert (d[(-k) % 256] == d * [1, -1]).all()                                      # the x axis
    assert (d[(64 - k) % 256] == d[:, ::-1]).all()                                   # the diagonal


def test_frame_steps_of_the_oracle():
    assert fo.frame_ts(0, 0, 1, 3) == [-1, -1, -1]
    assert fo.frame_ts(1, 0, 7, 2) == [0, 0]
    assert fo.frame_ts(10, 0, 4, 5) == [0, 4, 8, 9, 9] and fo.frame_ts(10, 2, 4, 2) == [8, 9]
