"""MemberScoreboard: what main.py:99-108 keeps per model, for every member of a population,
on the device.

The reference's training loop keeps a score history, the best score and the mean of the last
``avg_lookback`` scores per model, and saves the model whenever an episode's score beats that
mean (main.py:106-108). A population run has one ``EpisodeLog`` for all members; this class
reads its new entries per member on the device (``sacenv_board_update``,
include/sacenv_scoreboard.h): the look-back mean is numpy's bit for bit, so every save decision
is the reference's, and a device copy keeps the weights slab of each member the rule selects.
No host round trip until ``table``.

    log = EpisodeLog(env)
    board = MemberScoreboard(log, P, N, lookback=50, population=pop)
    for _ in range(iters):
        ...                      # act, env.step
        log.update()
        pop.learn()
        board.update()           # after learn: the point at which main.py:106 saves
    print(board.table())
    board.save_models("runs/search")

The snapshot's granularity is the ``update`` call: it holds the weights as they are when the
call runs, for every member with a saving episode among that call's entries.
"""
from __future__ import annotations

import csv
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .agent import save_models
from .sac_native import NativeSAC, SlabNets

# one member's record (SacenvBoardMember)
MEMBER_DTYPE = np.dtype({
    "names": ["episodes", "saves", "last_save_step", "last_end_step", "last", "best", "avg", "saved_now",
              "reserved", "terms"],
    "formats": ["<i8", "<i8", "<i8", "<i8", "<f8", "<f8", "<f8", "<u4", "<u4", ("<u8", (8,))],
    "offsets": [0, 8, 16, 24, 32, 40, 48, 56, 60, 64], "itemsize": _lib.BOARD_MEMBER_BYTES})


class MemberScoreboard:
    """Scores, look-back mean, save rule and saved weights of ``members`` members, member m
    owning envs ``[log.env_base + m * envs_per_member, + envs_per_member)`` of ``log``'s env.

    ``population``: a ``NativeSACPopulation`` of ``members`` members; the board then owns a
    ``[P, member_floats]`` snapshot of its weights. ``lookback`` is the reference's
    ``avg_lookback`` (1..128).
    """

    def __init__(self, log, members: int, envs_per_member: int, lookback: int = 50, population=None):
        self.lib = _lib.load()
        self._bytes, self._init, self._update, self._rewind = _lib.require(
            _lib.SCOREBOARD_EXPORTS, "sacenv_scoreboard.h", self.lib)
        self.log, self.population = log, population
        self.device = log.device
        self.P, self.N, self.L = int(members), int(envs_per_member), int(lookback)
        member_floats = 0
        if population is not None:
            if population.P != self.P:
                raise ValueError(f"the population has {population.P} members, the board {self.P}")
            if population.device != self.device:
                raise ValueError("the population and the log live on different devices")
            member_floats = int(population.pop_layout.member_floats)
        self.params = _lib.Board(members=self.P, envs_per_member=self.N, env_base=int(log.env_base),
                                 lookback=self.L, cap=int(log.capacity), member_floats=member_floats)
        need = C.c_int64()
        _lib.check(self._bytes(C.byref(self.params), C.byref(need)))
        self.board = torch.zeros(need.value, dtype=torch.uint8, device=self.device)
        self.snapshot = None
        if population is not None:
            self.snapshot = torch.zeros((self.P, member_floats), dtype=torch.float32, device=self.device)
        self._views = {}
        _lib.check(self._init(C.byref(self.params), self.board.data_ptr(), _lib.stream_handle(self.device)))
        log.watchers.append(self)

    def update(self) -> None:
        """Consume the log's new entries; only enqueues work on the current stream (two
        launches). Call it after ``log.update()``; after ``population.learn()`` to snapshot
        where main.py:106 saves."""
        w = s = None
        if self.snapshot is not None:
            w, s = self.population.weights.data_ptr(), self.snapshot.data_ptr()
        _lib.check(self._update(C.byref(self.params), self.log.log.data_ptr(), self.board.data_ptr(), w, s,
                                _lib.stream_handle(self.device)))

    def rewind(self) -> None:
        """The log was emptied (``EpisodeLog.drain`` calls this): start reading at its first entry."""
        _lib.check(self._rewind(C.byref(self.params), self.board.data_ptr(), _lib.stream_handle(self.device)))

    # ---- the host's view (each synchronises)

    def raw(self) -> bytes:
        """The board's bytes, after everything enqueued so far."""
        torch.cuda.current_stream(self.device).synchronize()
        return self.board.cpu().numpy().tobytes()

    def header(self) -> dict:
        cursor, missed, calls, _ = np.frombuffer(self.raw()[: _lib.BOARD_HEADER_BYTES], "<i8").tolist()
        return {"cursor": cursor, "missed": missed, "calls": calls}

    def records(self) -> np.ndarray:
        """The members' records as a structured array (``MEMBER_DTYPE``)."""
        lo = _lib.BOARD_HEADER_BYTES
        return np.frombuffer(self.raw()[lo: lo + _lib.BOARD_MEMBER_BYTES * self.P], MEMBER_DTYPE)

    def table(self) -> list:
        """One dict per member: what main.py:110-113 shows per model (Score, Best Score,
        Average Score), the saves, the endings by name and the member's drawn values."""
        names = self.log.term_names
        out = []
        for m, r in enumerate(self.records()):
            some = int(r["episodes"]) > 0
            terms = {name: int(r["terms"][k]) for k, name in enumerate(names) if name}
            other = int(r["terms"].sum()) - sum(terms.values())
            if other:   # codes without a name (>= 7 are counted in slot 7)
                terms["other"] = other
            row = {"member": m, "episodes": int(r["episodes"]),
                   "score": float(r["last"]) if some else None,
                   "best_score": float(r["best"]) if some else None,
                   "avg_score": float(r["avg"]) if some else None,
                   "saves": int(r["saves"]),
                   "last_save_step": int(r["last_save_step"]) if r["saves"] else None,
                   "terminations": terms}
            if self.population is not None:
                row.update(self.population.members[m].hpset())
            out.append(row)
        return out

    def best_member(self):
        """The member with the highest best score (the lower index on a tie); None before the
        first finished episode."""
        rec = self.records()
        have = np.flatnonzero(rec["episodes"] > 0)
        if have.size == 0:
            return None
        best = rec["best"][have]
        return int(have[np.flatnonzero(best == best.max())[0]])

    # ---- the saved weights

    def _saved(self, m: int) -> None:
        if self.snapshot is None:
            raise RuntimeError("this scoreboard keeps no snapshot (built without population=)")
        if not 0 <= m < self.P:
            raise IndexError(f"member {m} of {self.P}")
        if int(self.records()["saves"][m]) == 0:
            raise RuntimeError(f"member {m} never saved: no episode of its beat the look-back average")

    def snapshot_member(self, m: int) -> NativeSAC:
        """A stand-alone ``NativeSAC`` with the weights member m had at its last save (a copy, as
        ``NativeSACPopulation.export_member`` makes of the live ones)."""
        self._saved(m)
        pop, p = self.population, self.population.params
        return NativeSAC.from_slab(self.device, pop.configs[m], self.snapshot[m], obs_dim=p.obs_dim,
                                   max_action=p.max_action, adam_eps=p.adam_eps,
                                   noise_seed=pop.members[m].noise_seed)

    def _view(self, m: int):
        """Member m's five modules on views of its snapshot slab (``SlabNets``; kept)."""
        if m not in self._views:
            pop = self.population
            self._views[m] = SlabNets(self.snapshot[m], pop.params, pop.layout, pop.configs[m], pop.device, None, False)
        return self._views[m]

    def save_models(self, experiment_dir: str) -> list:
        """For every member that saved, its snapshot as the reference's checkpoint files under
        ``<experiment_dir>/member_<m>/checkpoints/``, and ``<experiment_dir>/overview.csv`` with a
        ``member_<m>;best_score`` row per member (main.py:121-128). Returns the members written."""
        if self.snapshot is None:
            raise RuntimeError("this scoreboard keeps no snapshot (built without population=)")
        rec = self.records()
        os.makedirs(experiment_dir, exist_ok=True)
        written = []
        for m in range(self.P):
            if int(rec["saves"][m]) > 0:
                save_models(self._view(m), os.path.join(experiment_dir, f"member_{m}"))
                written.append(m)
        with open(os.path.join(experiment_dir, "overview.csv"), "w", newline="") as f:
            writer = csv.writer(f, delimiter=";")
            for m in range(self.P):
                writer.writerow([f"member_{m}", float(rec["best"][m])])
        return written


__all__ = ["MemberScoreboard", "MEMBER_DTYPE"]
