"""EpisodeFrames: each member's best episode drawn on the device.

The reference draws the episodes that set a new best as animated GIFs (main.py -r,
rendering/boat_env_render.py): per step the track, the path so far, the boat at its heading and
a cursor over the time strips, one matplotlib figure per frame. ``BestEpisodes`` keeps those
episodes' rows on the device; this class draws them there (``sacenv_frames_render``,
include/sacenv_frames.h, which has the rules of the picture): palette-indexed frames, uint8
[F, H, W], straight from the member buffer with no host round trip of the rows.

    traces = BestEpisodes(env, members=P, envs_per_member=N)
    ...
    frames = EpisodeFrames(traces, every=5)
    idx = frames.render(m)                  # uint8 [F, 240, 320] on the device
    rgb = frames.rgb(idx)                   # uint8 [F, 240, 320, 3]
    frames.save_gif("runs/search")          # member_<m>/rendering/episode_0.gif

Not drawn: the reference's two wind strips (the rows hold no wind: the env's wind curve is
redrawn at the reset that follows the ending) and its text (that needs a font); the numbers are
in ``BestEpisodes.best(m)``.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib

# index -> (r, g, b): 32 water levels (matplotlib's Blues between 0.5 on the centre line and 0.1
# at the panel's edge, as the reference's two gradients), then one colour per name
_NAMED = {"OUTSIDE": (222, 226, 230), "BOUNDARY": (0, 0, 0), "GOAL": (0, 128, 0), "PATH": (255, 0, 0),
          "BOAT": (64, 40, 16), "STRIP": (255, 255, 255), "ZERO": (200, 200, 200), "RUDDER": (255, 165, 0),
          "ACTION": (0, 0, 255), "CURSOR": (48, 48, 48)}       # (all different: rgb() can be undone)
PALETTE = np.array(
    [tuple(int(round(a + (b - a) * k / (_lib.FRAMES_WATER - 1))) for a, b in zip((107, 174, 214), (222, 235, 247)))
     for k in range(_lib.FRAMES_WATER)]
    + [_NAMED[n] for n in ("OUTSIDE", "BOUNDARY", "GOAL", "PATH", "BOAT", "STRIP", "ZERO", "RUDDER", "ACTION",
                           "CURSOR")], dtype=np.uint8)
assert len(PALETTE) == _lib.FRAMES_COLOURS < 256


def direction_table() -> np.ndarray:
    """int16 [256, 2]: rint(1024 cos), rint(1024 sin) of 2 pi k / 256 in f64; the first quarter is
    computed (the sine as the cosine of the complement) and the others are that quarter turned,
    so the table has the square's symmetries exactly."""
    out = np.zeros((256, 2), np.int16)
    for k in range(64):
        out[k] = (round(1024.0 * math.cos(2.0 * math.pi * k / 256.0)),
                  round(1024.0 * math.cos(2.0 * math.pi * (64 - k) / 256.0)))
    for k in range(64, 256):
        out[k] = (-out[k - 64, 1], out[k - 64, 0])
    return out


class EpisodeFrames:
    """The frames of the episodes ``traces`` (a ``BestEpisodes``) keeps.

    Parameters
    ----------
    width, height, strip : the frame is ``width`` x ``height`` (16 .. 1024, the width a multiple of
        4); its bottom ``strip`` rows are the time strip (action and rudder against the step).
    every : draw every ``every``-th step, and the last one (main.py's render_skip_size).
    window : (xmin, xmax, ymin, ymax) of the track panel in world units; default the reference's
        (boat_env_render.py:50-57).
    rad : the path's half width in sixteenths of a pixel; boat : (length, half width) likewise.
    max_bytes : refuse a ``render`` whose frames and scratch take more than this.
    """

    def __init__(self, traces, width: int = 320, height: int = 240, strip: int = 48, every: int = 1, window=None,
                 *, rad: int = 12, boat=(96, 48), max_bytes: int = 1 << 30):
        from .traces import BestEpisodes
        if not isinstance(traces, BestEpisodes):
            raise ValueError("EpisodeFrames draws the episodes of a BestEpisodes")
        self.lib = traces.lib
        self._bytes, self._render = _lib.require(_lib.FRAMES_EXPORTS, "sacenv_frames.h", self.lib)
        self.traces, self.device = traces, traces.device
        self.W, self.H, self.S, self.every = int(width), int(height), int(strip), int(every)
        lo, hi = _lib.FRAMES_MIN_DIM, _lib.FRAMES_MAX_DIM
        if not (lo <= self.W <= hi and lo <= self.H <= hi) or self.W % 4:
            raise ValueError(f"a frame is {lo} .. {hi} pixels wide and high, the width a multiple of 4")
        if self.S < 2 or self.H - self.S < 8:
            raise ValueError("the strip takes at least 2 rows and leaves the track panel at least 8")
        if self.every < 1:
            raise ValueError("every must be at least 1")
        cfg = traces.env.cfg
        gl, tw = float(cfg.goal_line), float(cfg.track_width)
        if window is None:
            ytop = tw + int(0.1 * tw)
            window = (-5.0, gl + int(0.1 * gl), -ytop, ytop)
        xmin, xmax, ymin, ymax = (float(v) for v in window)
        if not (xmax > xmin and ymax > ymin):
            raise ValueError("window is (xmin, xmax, ymin, ymax) with xmin < xmax and ymin < ymax")
        self.window = (xmin, xmax, ymin, ymax)
        # the scales in f64, rounded once: the device multiplies by the same f32
        self.params = _lib.Frames(width=self.W, height=self.H, strip=self.S, members=traces.P, max_steps=traces.R,
                                  rad=int(rad), boat_len=int(boat[0]), boat_half=int(boat[1]), x0=xmin, y0=ymax,
                                  scale_x=16.0 * self.W / (xmax - xmin), scale_y=16.0 * (self.H - self.S) / (ymax - ymin),
                                  goal_line=gl, track_width=tw)
        table = direction_table()
        C.memmove(self.params.dir, table.ctypes.data, table.nbytes)
        sb, fb = C.c_int64(), C.c_int64()
        _lib.check(self._bytes(C.byref(self.params), C.byref(sb), C.byref(fb)))
        self.scratch_bytes, self.frame_bytes, self.max_bytes = sb.value, fb.value, int(max_bytes)
        if self.scratch_bytes > self.max_bytes:
            raise ValueError(f"the scratch takes {self.scratch_bytes} bytes, more than max_bytes = {self.max_bytes}")
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=self.device)

    def _member(self, m: int) -> int:
        if not 0 <= m < self.traces.P:
            raise IndexError(f"member {m} of {self.traces.P}")
        return int(m)

    def frame_steps(self, m: int) -> list:
        """The kept rows member m's frames show: 0, every, 2 every, .., then the last row (the
        reference's ``dt % render_skip_size == 0 or dt == total_dt``); [] for a member without
        an episode. One read-back of the headers, as ``BestEpisodes.table``."""
        rows = int(self.traces.headers()[self._member(m)]["rows"])
        return list(range(0, rows - 1, self.every)) + [rows - 1] if rows else []

    def render(self, m: int, first: int = 0, count: int | None = None) -> torch.Tensor:
        """Frames ``first .. first + count - 1`` of member m as a uint8 [count, H, W] device tensor
        of palette indices; only enqueues work (three launches on the env's stream). Frames past
        the episode's end repeat its last one; a member without an episode gives the background.
        ``count=None``: up to the last frame, which costs ``frame_steps``' read-back (at least one
        frame)."""
        m, first = self._member(m), int(first)
        if count is None:
            count = max(len(self.frame_steps(m)) - first, 1)
        count = int(count)
        if first < 0 or count < 1:
            raise ValueError("first must be >= 0 and count >= 1")
        if count * self.frame_bytes + self.scratch_bytes > self.max_bytes:
            raise ValueError(f"{count} frames of {self.W} x {self.H} and the scratch take "
                             f"{count * self.frame_bytes + self.scratch_bytes} bytes, more than max_bytes = "
                             f"{self.max_bytes}")
        out = torch.empty((count, self.H, self.W), dtype=torch.uint8, device=self.device)
        _lib.check(self._render(C.byref(self.params), self.traces.members.data_ptr(), m, first, self.every, count,
                                out.data_ptr(), self.scratch.data_ptr(), self.traces.env.stream))
        return out

    def rgb(self, frames) -> torch.Tensor | np.ndarray:
        """Palette indices -> uint8 [..., 3]; a device tensor stays on its device."""
        if isinstance(frames, torch.Tensor):
            return torch.from_numpy(PALETTE).to(frames.device)[frames.long()]
        return PALETTE[np.asarray(frames)]

    def save_gif(self, experiment_dir: str, duration_ms: int = 40) -> list:
        """Every member's best episode as ``<dir>/member_<m>/rendering/episode_0.gif`` (where the
        reference's renderer puts its GIFs), written with Pillow from the palette indices as they
        are: lossless (Pillow writes a run of identical frames as one frame that lasts as long as
        the run). Returns the members written (those with an episode)."""
        try:
            from PIL import Image
        except ImportError as e:
            raise ImportError("save_gif writes its files with Pillow, which is not installed") from e
        flat = PALETTE.reshape(-1).tolist() + [0] * (768 - 3 * len(PALETTE))
        rows = self.traces.headers()["rows"]
        written = []
        for m in range(self.traces.P):
            if int(rows[m]) == 0:
                continue
            idx = self.render(m).cpu().numpy()
            images = []
            for frame in idx:
                im = Image.fromarray(frame, mode="P")
                im.putpalette(flat)
                images.append(im)
            d = os.path.join(experiment_dir, f"member_{m}", "rendering")
            os.makedirs(d, exist_ok=True)
            # (optimize=False and disposal 1: Pillow neither reorders the palette nor crops frames)
            images[0].save(os.path.join(d, "episode_0.gif"), save_all=True, append_images=images[1:],
                           duration=duration_ms, loop=0, optimize=False, disposal=1)
            written.append(m)
        return written


__all__ = ["EpisodeFrames", "PALETTE", "direction_table"]
