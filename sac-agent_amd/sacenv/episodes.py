"""EpisodeLog: score, length and end of every finished episode of a vectorised env.

The reference's training loop is organised around finished episodes (main.py:70-114):
``score += reward`` per step, ``score_history.append(score)``, a best score, a
look-back average and how each episode ended. ``VecBoatEnv`` and the toy envs
restart inside the step launch and keep only each env's last ending, so this class
rebuilds the per-episode record on the device from the step records those launches
already write (``sacenv_episodes_update``, include/sacenv_episodes.h): one 32-B
entry per finished episode, ascending by (end_step, env), with no host round trip
until ``drain``.

    log = EpisodeLog(env)
    for _ in range(steps):            # a step loop
        env.step(actions)
        log.update()
    records, _ = env.rollout(actions) # or a rollout's records, K steps at once
    log.update(records)
    print(log.summary(lookback=100))

The persistent ``segment_async`` launch rewrites its record in place, so its steps
cannot be logged afterwards; run them through ``rollout`` to log them.
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from .toys import TOY_RECORD_BYTES, VecToyEnv

HEADER_BYTES = _lib.EPISODE_ENTRY_BYTES
# one log entry (include/sacenv_episodes.h); the reserved word is left out of the view
ENTRY_DTYPE = np.dtype({"names": ["end_step", "score", "env", "length", "term"],
                        "formats": ["<i8", "<f8", "<i4", "<i4", "<u4"],
                        "offsets": [0, 8, 16, 20, 24], "itemsize": _lib.EPISODE_ENTRY_BYTES})


class EpisodeLog:
    """The finished episodes of ``env`` (a ``VecBoatEnv`` or a ``VecToyEnv``).

    Parameters
    ----------
    capacity : entries the device log holds between two ``drain`` calls. Episodes
        past it are counted (``dropped``) and not stored.
    history : length of ``history``, the drained entries kept on the host.
    step0 : global number of the next step passed to ``update`` (``end_step`` counts
        from it).
    log_buffer : a uint8 device tensor of at least ``32 + 32 * capacity`` bytes, 16-B
        aligned, to hold the log (e.g. part of a larger pool); default: its own.

    The carry starts from the env's running ``ep_reward`` and ``index`` (a toy's
    ``count``), so a log attached in mid-run reports the episodes in flight with
    their full score and length (the part before the attachment summed by the env,
    in f64, not from the f32 records). Attach between steps, with every env that has
    ended already restarted (always the case with ``autoreset``).
    """

    def __init__(self, env, capacity: int = 1 << 20, *, history: int = 1 << 16, step0: int = 0,
                 log_buffer: torch.Tensor | None = None):
        self.lib = _lib.load()
        self._scratch_bytes, self._update = _lib.require(_lib.EPISODE_EXPORTS, "sacenv_episodes.h", self.lib)
        self.env = env
        self.device = env.device
        self.num_envs, self.n_pad = int(env.num_envs), int(env.n_pad)
        NP = self.n_pad
        toy = isinstance(env, VecToyEnv)
        if toy:
            self.record_bytes = TOY_RECORD_BYTES
            cols = (8, 12, 13)                      # obs f32 x 2 | reward f32 | done u8 | term u8
            self.env_base, self.term_names = 0, _lib.TOY_TERM_NAMES
        else:
            self.record_bytes = _lib.RECORD_BYTES
            cols = (_lib.REC_REWARD, _lib.REC_DONE, _lib.REC_TERM)
            self.env_base, self.term_names = int(env.env_id_offset), _lib.TERM_NAMES
        self.capacity = int(capacity)
        if self.capacity < 0:
            raise ValueError("capacity must not be negative")
        self.scan = _lib.EpisodeScan(n_envs=self.num_envs, n_pad=NP, n_steps=1, env_base=self.env_base,
                                     rec_stride=0, reward_off=cols[0] * NP, done_off=cols[1] * NP,
                                     term_off=cols[2] * NP, step0=int(step0), cap=self.capacity)
        nb = HEADER_BYTES + _lib.EPISODE_ENTRY_BYTES * self.capacity
        if log_buffer is None:
            log_buffer = torch.zeros(nb, dtype=torch.uint8, device=self.device)
        elif (log_buffer.dtype != torch.uint8 or log_buffer.device != self.device or log_buffer.dim() != 1
              or not log_buffer.is_contiguous() or log_buffer.numel() < nb or log_buffer.data_ptr() % 16):
            raise ValueError(f"log_buffer must be a contiguous, 16-B aligned uint8 tensor of >= {nb} bytes "
                             f"on {self.device}")
        self.log = log_buffer[:nb]
        self.log[:HEADER_BYTES].zero_()
        self._total = self.log[:8].view(torch.int64)
        # carry: f64 [n_pad] score so far | i32 [n_pad] steps so far
        self.carry = torch.zeros(12 * NP, dtype=torch.uint8, device=self.device)
        self.carry_score = self.carry[: 8 * NP].view(torch.float64)
        self.carry_length = self.carry[8 * NP:].view(torch.int32)
        if not toy:
            self.carry_score[: self.num_envs].copy_(env.ep_reward)
        self.carry_length[: self.num_envs].copy_(env.count if toy else env.index)
        self.scratch = None
        self.reserve(1)
        self.history = collections.deque(maxlen=int(history))
        self.dropped = self.dropped_total = 0
        self.episodes = 0                      # drained so far, dropped ones included
        self.best_score = float("-inf")
        self.term_counts = np.zeros(len(self.term_names), np.int64)
        # readers of the device log that keep a cursor into it (sacenv/scoreboard.py): ``drain``
        # lets each consume what is there before it empties the log, and rewinds them after
        self.watchers = []

    @property
    def step0(self) -> int:
        """Global number of the next step ``update`` expects."""
        return int(self.scan.step0)

    def reserve(self, n_steps: int) -> None:
        """Make the scratch large enough for ``update`` calls of up to ``n_steps`` steps
        (``update`` does it itself; call this before capturing updates into a graph)."""
        s = self.scan
        sized = _lib.EpisodeScan(n_envs=s.n_envs, n_pad=s.n_pad, n_steps=int(n_steps), env_base=s.env_base,
                                 rec_stride=self.record_bytes * self.n_pad, reward_off=s.reward_off,
                                 done_off=s.done_off, term_off=s.term_off, step0=s.step0, cap=s.cap)
        need = C.c_int64()
        _lib.check(self._scratch_bytes(C.byref(sized), C.byref(need)))
        if self.scratch is None or self.scratch.numel() < need.value:
            self.scratch = torch.empty(need.value, dtype=torch.uint8, device=self.device)

    def update(self, records: torch.Tensor | None = None, n_steps: int | None = None) -> None:
        """Scan the next steps' records; only enqueues work on the env's stream.

        ``records=None``: the env's own ``record``, one step, after a ``step`` /
        ``step_async``. Otherwise a ``[K, >= record_bytes * n_pad]`` uint8 device tensor
        as ``VecBoatEnv.rollout`` returns it (rows may be strided; ``n_steps`` scans
        only the first rows).

        EVERY step of the env must be passed exactly once, in order: the carry holds
        each env's episode in flight, and a step left out or passed twice puts every
        later score and length of that episode off.
        """
        nb = self.record_bytes * self.n_pad
        if records is None:
            if n_steps not in (None, 1):
                raise ValueError("the env's own record holds one step")
            records, K, stride = self.env.record, 1, 0
        else:
            if (not isinstance(records, torch.Tensor) or records.dtype != torch.uint8
                    or records.device != self.device or records.dim() != 2 or records.shape[0] < 1
                    or records.shape[1] < nb or records.stride(1) != 1):
                raise ValueError(f"records must be a uint8 [K, >= {nb}] tensor on {self.device} with "
                                 "contiguous rows")
            K = int(records.shape[0]) if n_steps is None else int(n_steps)
            if not 1 <= K <= records.shape[0]:
                raise ValueError(f"n_steps must be 1..{records.shape[0]}")
            stride = int(records.stride(0)) if K > 1 else 0
        self.reserve(K)
        self.scan.n_steps, self.scan.rec_stride = K, stride
        _lib.check(self._update(C.byref(self.scan), records.data_ptr(), self.carry.data_ptr(),
                                self.log.data_ptr(), self.scratch.data_ptr(), self.scratch.numel(),
                                self.env.stream))
        self._keep = records
        self.scan.step0 += K

    def drain(self) -> np.ndarray:
        """Synchronise the stream, return the stored entries (a structured array with
        fields end_step, score, env, length, term; ``min(total, capacity)`` of them, in
        the order they ended) and empty the device log. ``dropped`` is set to the number
        of episodes that did not fit since the last drain. Watchers (a ``MemberScoreboard``) are
        updated first and rewound after, so they miss nothing and read nothing twice."""
        for w in self.watchers:
            w.update()
        torch.cuda.current_stream(self.device).synchronize()
        total = int(self._total.item())
        n = min(total, self.capacity)
        raw = self.log[HEADER_BYTES: HEADER_BYTES + _lib.EPISODE_ENTRY_BYTES * n].cpu().numpy()
        out = raw.view(ENTRY_DTYPE)
        self._total.zero_()
        for w in self.watchers:
            w.rewind()
        self.dropped = max(total - self.capacity, 0)
        self.dropped_total += self.dropped
        self.episodes += total
        if n:
            self.best_score = max(self.best_score, float(out["score"].max()))
            self.term_counts += np.bincount(np.minimum(out["term"], len(self.term_names) - 1).astype(np.int64),
                                            minlength=len(self.term_names))
            self.history.extend(out[-self.history.maxlen:].tolist() if self.history.maxlen else ())
        return out

    def summary(self, lookback: int = 100) -> dict:
        """What main.py:99-114 prints per episode, over everything drained so far (drains
        first): the number of episodes, the best score, the mean of the last ``lookback``
        scores (``avg_lookback``) and the endings per termination name."""
        self.drain()
        last = [h[1] for h in list(self.history)[-int(lookback):]] if lookback > 0 else []
        return {"episodes": self.episodes,
                "best_score": self.best_score if self.best_score > float("-inf") else None,
                "avg_score": float(np.mean(last)) if last else None,
                "lookback": len(last),
                "terminations": {name: int(self.term_counts[k]) for k, name in enumerate(self.term_names)
                                 if name},
                "dropped": self.dropped_total}


__all__ = ["EpisodeLog", "ENTRY_DTYPE"]
