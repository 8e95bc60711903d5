"""The episode frames in plain numpy (include/sacenv_frames.h).

``Spec`` is the descriptor (frame size, window, scales rounded once to f32, the direction
table); ``points`` turns a member's rows into fixed-point values, ``coverage`` into the map of
each pixel's first covering segment, and ``render`` composes frames from them: the rules of the
header, restated pixel-parallel, every float step a single f32 operation and every integer step
an int64 one. ``pack_member`` lays rows out as a member buffer of include/sacenv_traces.h.
"""
from __future__ import annotations

import struct

import numpy as np

import traces_oracle as to

WATER = 32
OUTSIDE, BOUNDARY, GOAL, PATH, BOAT, STRIP, ZERO, RUDDER, ACTION, CURSOR, COLOURS = range(32, 43)
NONE = 2 ** 31 - 1
CHUNK = 128
F32 = np.float32


def direction_table() -> np.ndarray:
    """int16 [256, 2]: rint(1024 cos), rint(1024 sin) of 2 pi k / 256, in f64. The first quarter
    is computed (the sine as the cosine of the complement), the rest is that quarter turned."""
    q = np.rint(1024.0 * np.cos(2.0 * np.pi * np.arange(65) / 256.0)).astype(np.int64)
    out = np.zeros((256, 2), np.int64)
    out[:64, 0], out[:64, 1] = q[:64], q[64:0:-1]
    for k in range(64, 256):
        out[k] = (-out[k - 64, 1], out[k - 64, 0])
    return out.astype(np.int16)


def default_window(goal_line: float, track_width: float) -> tuple:
    """(xmin, xmax, ymin, ymax) of rendering/boat_env_render.py:50-57."""
    ytop = track_width + int(0.1 * track_width)
    return (-5.0, goal_line + int(0.1 * goal_line), -ytop, ytop)


class Spec:
    def __init__(self, width, height, strip, goal_line, track_width, window=None, rad=12, boat_len=96, boat_half=48):
        self.W, self.H, self.S, self.HP = int(width), int(height), int(strip), int(height) - int(strip)
        self.rad, self.boat_len, self.boat_half = int(rad), int(boat_len), int(boat_half)
        xmin, xmax, ymin, ymax = default_window(goal_line, track_width) if window is None else window
        self.x0, self.y0 = F32(xmin), F32(ymax)
        self.sx = F32(16.0 * self.W / (float(xmax) - float(xmin)))
        self.sy = F32(16.0 * self.HP / (float(ymax) - float(ymin)))
        self.goal_line, self.track_width = F32(goal_line), F32(track_width)
        self.dir = direction_table()


def scratch_bytes(s: Spec, max_steps: int) -> int:
    """The scratch of a render call: the background's four numbers, 64 B per row, 16 B per strip
    column and the coverage map."""
    return 16 + 64 * (max_steps + 1) + 16 * s.W + 4 * s.W * s.HP


def clamp(v, lo, hi):
    """!(v >= lo) ? lo : (v > hi ? hi : v) on f32 arrays: a NaN becomes lo."""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore"):
        return np.where(~(v >= F32(lo)), F32(lo), np.where(v > F32(hi), F32(hi), v)).astype(F32)


def _fixed(v, lo, hi):
    return np.rint(clamp(v, lo, hi)).astype(np.int64)


def fx(s: Spec, x):
    with np.errstate(all="ignore"):
        return _fixed((np.asarray(x, F32) - s.x0) * s.sx, -1024, 16 * s.W + 1024)


def fy(s: Spec, y):
    with np.errstate(all="ignore"):
        return _fixed((s.y0 - np.asarray(y, F32)) * s.sy, -1024, 16 * s.HP + 1024)


def strip_row(s: Spec, a):
    with np.errstate(all="ignore"):
        top = F32(s.S - 1)
        return _fixed((F32(1) - np.asarray(a, F32)) * F32(0.5) * top, 0, s.S - 1)


def points(s: Spec, obs, action) -> dict:
    """The rows' fixed-point values: X, Y, heading index, action row, rudder row (int64 [rows])."""
    obs, action = np.asarray(obs, F32).reshape(-1, to.OBS), np.asarray(action, F32).reshape(-1)
    with np.errstate(all="ignore"):
        x = obs[:, 0] * s.goal_line
        y = obs[:, 3] * (F32(2) * s.track_width) - s.track_width
        hd = _fixed(obs[:, 6] * F32(256), -8388608, 8388608) & 255
        rud = obs[:, 9] * F32(2) - F32(1)
    return {"X": fx(s, x), "Y": fy(s, y), "hd": hd, "arow": strip_row(s, action), "rrow": strip_row(s, rud)}


def covers(ax, ay, bx, by, cx, cy, rad):
    """The header's three-way test, with whatever integers it is given (Python's or int64 arrays)."""
    dx, dy, px, py = bx - ax, by - ay, cx - ax, cy - ay
    t, dd = px * dx + py * dy, dx * dx + dy * dy
    end0 = px * px + py * py <= rad * rad
    end1 = (px - dx) * (px - dx) + (py - dy) * (py - dy) <= rad * rad
    cr = px * dy - py * dx
    mid = cr * cr <= rad * rad * dd
    if isinstance(t, np.ndarray):
        return np.where(t <= 0, end0, np.where(t >= dd, end1, mid))
    return end0 if t <= 0 else (end1 if t >= dd else mid)


def coverage(s: Spec, X, Y) -> np.ndarray:
    """first[r, c]: the smallest segment j (1 .. rows - 1) that covers the panel pixel, NONE if none."""
    cy, cx = np.meshgrid(16 * np.arange(s.HP, dtype=np.int64) + 8, 16 * np.arange(s.W, dtype=np.int64) + 8,
                         indexing="ij")
    first = np.full((s.HP, s.W), NONE, np.int64)
    for j in range(len(X) - 1, 0, -1):                      # descending: the smallest j is written last
        hit = covers(int(X[j - 1]), int(Y[j - 1]), int(X[j]), int(Y[j]), cx, cy, s.rad)
        first[hit] = j
    return first


def boat_vertices(s: Spec, X, Y, hd):
    ux, uy = int(s.dir[hd, 0]), int(s.dir[hd, 1])
    fx_, fy_, sx_, sy_ = ux, -uy, uy, ux
    L, G, B = s.boat_len, s.boat_len >> 1, s.boat_half
    return [(X + ((L * fx_) >> 10), Y + ((L * fy_) >> 10)),
            (X + ((-G * fx_ - B * sx_) >> 10), Y + ((-G * fy_ - B * sy_) >> 10)),
            (X + ((-G * fx_ + B * sx_) >> 10), Y + ((-G * fy_ + B * sy_) >> 10))]


def _edge(a, b, cx, cy):
    return (b[0] - a[0]) * (cy - a[1]) - (b[1] - a[1]) * (cx - a[0])


def background(s: Spec) -> np.ndarray:
    """The panel without path and boat, uint8 [HP, W]."""
    rc, rt, rb = (int(fy(s, v)) >> 4 for v in (F32(0), s.track_width, -s.track_width))
    cg = int(fx(s, s.goal_line)) >> 4
    r = np.arange(s.HP, dtype=np.int64)
    col = np.minimum(WATER - 1, np.abs(r - rc) * 64 // s.HP)
    col = np.where((r < rt) | (r > rb), OUTSIDE, col)
    col = np.where((r == rt) | (r == rb), BOUNDARY, col)
    panel = np.repeat(col[:, None], s.W, axis=1)
    if 0 <= cg < s.W:
        panel[:, cg] = GOAL
    return panel.astype(np.uint8)


def frame_ts(rows: int, first_frame: int, every: int, n_frames: int) -> list:
    """The step each frame of a call shows; -1 for an empty member."""
    return [min((first_frame + f) * every, rows - 1) if rows else -1 for f in range(n_frames)]


def render(s: Spec, obs, action, ts) -> np.ndarray:
    """The frames showing steps ``ts`` (row indices, -1: an empty member) of the episode with
    these kept rows: uint8 [len(ts), H, W]."""
    obs = np.asarray(obs, F32).reshape(-1, to.OBS)
    rows = len(obs)
    p = points(s, obs, action)
    first = coverage(s, p["X"], p["Y"])
    base = background(s)
    cy, cx = np.meshgrid(16 * np.arange(s.HP, dtype=np.int64) + 8, 16 * np.arange(s.W, dtype=np.int64) + 8,
                         indexing="ij")
    cols = np.arange(s.W, dtype=np.int64)
    q = np.arange(s.S, dtype=np.int64)[:, None]
    strip0 = np.where(q == (s.S - 1) >> 1, ZERO, STRIP) * np.ones((1, s.W), np.int64)
    out = np.zeros((len(ts), s.H, s.W), np.uint8)
    if rows:
        j = cols * (rows - 1) // (s.W - 1)
        jp = np.maximum(cols - 1, 0) * (rows - 1) // (s.W - 1)
        between = {}
        for name in ("arow", "rrow"):
            lo, hi = np.minimum(p[name][j], p[name][jp]), np.maximum(p[name][j], p[name][jp])
            between[name] = (q >= lo[None, :]) & (q <= hi[None, :])
    for k, t in enumerate(ts):
        panel, strip = base.copy(), strip0.copy()
        if t >= 0:
            assert rows and t <= rows - 1
            panel[first <= t] = PATH
            v0, v1, v2 = boat_vertices(s, int(p["X"][t]), int(p["Y"][t]), int(p["hd"][t]))
            panel[(_edge(v0, v2, cx, cy) >= 0) & (_edge(v2, v1, cx, cy) >= 0) & (_edge(v1, v0, cx, cy) >= 0)] = BOAT
            shown = (j <= t)[None, :]
            strip[between["rrow"] & shown] = RUDDER
            strip[between["arow"] & shown] = ACTION
            strip[:, t * (s.W - 1) // (rows - 1) if rows > 1 else 0] = CURSOR
        out[k, : s.HP], out[k, s.HP:] = panel, strip
    return out


def pack_member(max_steps: int, obs=None, action=None, first_row: int = 0, junk: int = 0) -> bytes:
    """A member's bytes (header, rows, zeros or ``junk`` bytes up to max_steps + 1 rows) holding
    these kept rows; no rows: the empty state."""
    if obs is None or len(obs) == 0:
        return to.EMPTY + bytes([junk]) * (to.ROW_BYTES * (max_steps + 1))
    obs, action = np.asarray(obs, F32).reshape(-1, to.OBS), np.asarray(action, F32).reshape(-1)
    rows = len(obs)
    assert rows <= max_steps + 1
    head = struct.pack(to.HEADER_FORMAT, 1000, 1.5, 3, first_row + rows - 1, 1, rows, first_row, 0, 1)
    body = b"".join(to.pack_row(obs[i], action[i], 0.25) for i in range(rows))
    return head + body + bytes([junk]) * (to.ROW_BYTES * (max_steps + 1 - rows))
