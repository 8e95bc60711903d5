"""PopulationSelection: the losers of a hyper-parameter search copy the winners, on the device.

A population (``NativeSACPopulation``) trains P members that differ in four drawn values, and a
``MemberScoreboard`` keeps each member's look-back mean on the device. This class acts on the
two: truncation selection, the exploit and explore steps of population-based training
(include/sacenv_selection.h states the rule completely). Every ``select`` ranks the members that
finished ``min_episodes`` episodes since they were last replaced; if at least ``2 * quantile`` are
ready, each of the worst ``quantile`` becomes a copy of one of the best ``quantile`` -- the whole
slab: nets, target net, Adam moments and the kernels' copies, so no ``sync`` follows -- and takes
the winner's four values, each times one of ``factors`` and clipped to ``ranges``. Two launches,
no host round trip, the same bytes from run to run for the same ``seed``.

    board = MemberScoreboard(log, P, N, lookback=50)
    selection = PopulationSelection(board, pop, quantile=P // 4)
    for it in range(iters):
        ...                              # act, env.step, log.update, pop.learn
        if it % K == K - 1:
            board.update()
            for r in selection.step():   # select() + commit()
                print(r)

``commit`` is the one synchronisation: ``sacenv_sac_pop_learn`` takes the members' values from
host memory, in its kernel arguments, so the new values are read back and written into the
population's table and configs. A ``learn`` captured into a graph before a ``commit`` carries the
old values: capture it again.

What stays put: the board (it is the record of what the envs did; a replaced member keeps its
score history, and ``min_episodes`` keeps it from being judged on it at once -- with
``min_episodes >= lookback`` the window holds post-copy scores only when the member is ready
again) and the loser's replay buffer (SAC is off-policy: its own rows stay valid).
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import torch

from . import _lib
from .population import HPRanges

# one member's record (SacenvSelectMember)
STATE_DTYPE = np.dtype({
    "names": ["since", "replaced", "source_now", "rank_now", "parent", "reserved", "hp"],
    "formats": ["<i8", "<i8", "<i4", "<i4", "<i4", "<i4", ("<f8", (4,))],
    "offsets": [0, 8, 16, 20, 24, 28, 32], "itemsize": _lib.SELECT_MEMBER_BYTES})
# hp[k]: the AgentConfig field and the reference's config key (PopulationMember.hpset)
HP_FIELDS = ("lr_alpha", "lr_beta", "gamma", "tau")
HP_KEYS = ("learning_rate_alpha", "learning_rate_beta", "gamma", "tvn_parameter_modulation_tau")


def clip_ranges(ranges: HPRanges):
    """(lo[4], hi[4]) in the state's order: lr_actor, lr_critic, gamma, tau."""
    return ((ranges.alpha_min, ranges.beta_min, ranges.gamma_min, ranges.tau_min),
            (ranges.alpha_max, ranges.beta_max, ranges.gamma_max, ranges.tau_max))


class PopulationSelection:
    """Truncation selection on ``board``'s look-back means and ``population``'s slab.

    ``quantile`` (default ``P // 4``, at least 1): how many members lose and how many may be
    copied from; ``min_episodes`` (default the board's ``lookback``): episodes a member must
    finish after a replacement before it is ranked again; ``seed``: of the source and factor
    draws; ``factors``: the two multipliers; ``ranges``: the clip range of each value.
    """

    def __init__(self, board, population, quantile: int | None = None, min_episodes: int | None = None,
                 seed: int = 0, factors=(0.8, 1.2), ranges: HPRanges = HPRanges()):
        self.lib = _lib.load()
        self._bytes, self._init, self._step = _lib.require(_lib.SELECTION_EXPORTS, "sacenv_selection.h", self.lib)
        self.board, self.population = board, population
        self.device = board.device
        self.P = int(board.P)
        self.member_floats = int(population.pop_layout.member_floats)
        self._check_population()
        lo, hi = clip_ranges(ranges)
        self.params = _lib.Select(
            members=self.P, quantile=max(self.P // 4, 1) if quantile is None else int(quantile),
            lookback=int(board.L), reserved=0,
            min_episodes=int(board.L) if min_episodes is None else int(min_episodes),
            member_floats=self.member_floats, seed=int(seed) & (2 ** 64 - 1),
            factor=(C.c_double * 2)(*map(float, factors)), lo=(C.c_double * 4)(*lo), hi=(C.c_double * 4)(*hi))
        need = C.c_int64()
        _lib.check(self._bytes(C.byref(self.params), C.byref(need)))
        self.state = torch.zeros(need.value, dtype=torch.uint8, device=self.device)
        _lib.check(self._init(C.byref(self.params), population._hp, self.state.data_ptr(),
                              _lib.stream_handle(self.device)))
        self._committed = np.zeros(self.P, np.int64)   # each member's `replaced` at the last commit

    def _check_population(self) -> None:
        pop = self.population
        if pop.P != self.P:
            raise ValueError(f"the population has {pop.P} members, the selection {self.P}")
        if int(pop.pop_layout.member_floats) != self.member_floats:
            raise ValueError(f"the population's slab holds {int(pop.pop_layout.member_floats)} floats per member, "
                             f"the selection's {self.member_floats}")
        if pop.device != self.device:
            raise ValueError("the population and the board live on different devices")

    def select(self) -> None:
        """One round on the board as it stands (call ``board.update()`` first); only enqueues
        work on the current stream (two launches). The population's host-side values are stale
        until ``commit``."""
        self._check_population()
        _lib.check(self._step(C.byref(self.params), self.board.board.data_ptr(), self.state.data_ptr(),
                              self.population.weights.data_ptr(), _lib.stream_handle(self.device)))

    def commit(self) -> list:
        """Read the state back (the one synchronisation) and give every member replaced since
        the last ``commit`` its new values on the host: ``population._hp[m]`` (what ``learn``
        passes to the kernels), ``population.configs[m]`` and ``members[m].cfg`` -- the state's
        doubles exactly. Returns ``[{"member", "source", **hpset}]``."""
        self._check_population()
        pop, out = self.population, []
        for m, r in enumerate(self.records()):
            if int(r["replaced"]) == self._committed[m]:
                continue
            self._committed[m] = int(r["replaced"])
            v = [float(x) for x in r["hp"]]
            hp = pop._hp[m]
            hp.lr_actor, hp.lr_critic, hp.gamma, hp.tau = v
            cfg = dataclasses.replace(pop.configs[m], **dict(zip(HP_FIELDS, v)))
            pop.configs[m] = pop.members[m].cfg = cfg
            out.append({"member": m, "source": int(r["parent"]), **dict(zip(HP_KEYS, v))})
        return out

    def step(self) -> list:
        """``select()`` and ``commit()``."""
        self.select()
        return self.commit()

    # ---- the host's view (each synchronises)

    def raw(self) -> bytes:
        """The state's bytes, after everything enqueued so far."""
        torch.cuda.current_stream(self.device).synchronize()
        return self.state.cpu().numpy().tobytes()

    def header(self) -> dict:
        rnd, total, _, _ = np.frombuffer(self.raw()[: _lib.SELECT_HEADER_BYTES], "<i8").tolist()
        return {"round": rnd, "replaced_total": total}

    def records(self) -> np.ndarray:
        """The members' records as a structured array (``STATE_DTYPE``)."""
        return np.frombuffer(self.raw()[_lib.SELECT_HEADER_BYTES:], STATE_DTYPE)

    def table(self) -> list:
        """One dict per member: its rank in the last round (None if it was not ready), how often
        it was replaced, the member it was last copied from (None if never) and its current four
        values under the reference's config keys."""
        return [{"member": m, "rank": int(r["rank_now"]) if r["rank_now"] >= 0 else None,
                 "replaced": int(r["replaced"]), "parent": int(r["parent"]) if r["parent"] >= 0 else None,
                 **dict(zip(HP_KEYS, (float(x) for x in r["hp"])))}
                for m, r in enumerate(self.records())]


__all__ = ["PopulationSelection", "STATE_DTYPE", "HP_FIELDS", "HP_KEYS", "clip_ranges"]
