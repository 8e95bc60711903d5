"""Population selection in plain Python and numpy (include/sacenv_selection.h, rule 1-7).

``SelectionOracle`` keeps the selection state as Python lists and restates one
``sacenv_select_step`` on a board given as two sequences (each member's ``episodes`` and
``avg``); ``pack`` gives the state's bytes. The draws come from ``oracle/ctr_sampler.py``'s
Philox4x64-10, which tests/test_ctr_sampler_cpu.py pins to numpy's. The arithmetic of rule 5 is
one f64 multiply and two comparisons, which Python's floats do as the device does.
"""
from __future__ import annotations

import math
import struct

import numpy as np

from ctr_sampler import philox4x64_10

HEADER_BYTES, MEMBER_BYTES = 32, 64
MEMBER_FORMAT = "<qqiiii4d"        # SacenvSelectMember
assert struct.calcsize(MEMBER_FORMAT) == MEMBER_BYTES
KEY1 = int.from_bytes(b"select", "big")
DEFAULT_LO = (0.001, 0.0008, 0.95, 0.001)      # configs/hp_configs.yaml (sacenv.population.HPRanges)
DEFAULT_HI = (0.01, 0.008, 0.99, 0.01)


def source_rank(w0: int, q: int) -> int:
    """Rule 4's multiply-shift: the high 32 bits of w0 scaled to [0, q)."""
    return ((int(w0) >> 32) * q) >> 32


def rank_ready(ready, avg) -> list:
    """Rule 2: rank[m] of a ready m = the ready j with avg[j] > avg[m], or equal and j < m; -1 for
    the others. (Python's float comparisons are IEEE's: -0.0 == 0.0, the infinities ordered.)"""
    P = len(ready)
    return [sum(1 for j in range(P) if ready[j] and (avg[j] > avg[m] or (avg[j] == avg[m] and j < m)))
            if ready[m] else -1 for m in range(P)]


class SelectionOracle:
    def __init__(self, hp, quantile: int, min_episodes: int, seed: int = 0, factor=(0.8, 1.2),
                 lo=DEFAULT_LO, hi=DEFAULT_HI):
        """``hp``: [P][4] initial lr_actor, lr_critic, gamma, tau."""
        self.P, self.q, self.min_episodes, self.seed = len(hp), int(quantile), int(min_episodes), int(seed)
        self.factor, self.lo, self.hi = tuple(map(float, factor)), tuple(map(float, lo)), tuple(map(float, hi))
        self.round = self.replaced_total = 0
        self.since = [0] * self.P
        self.replaced = [0] * self.P
        self.source_now = [-1] * self.P
        self.rank_now = [-1] * self.P
        self.parent = [-1] * self.P
        self.hp = [[float(x) for x in row] for row in hp]

    def step(self, episodes, avg) -> list:
        """One ``sacenv_select_step`` on a board with these per-member ``episodes`` and ``avg``.
        Returns [(loser, source)], ascending by loser: the slab copies of rule 7."""
        P, q, r = self.P, self.q, self.round
        episodes, avg = [int(e) for e in episodes], [float(a) for a in avg]
        ready = [episodes[m] - self.since[m] >= self.min_episodes and not math.isnan(avg[m]) for m in range(P)]
        R = sum(ready)
        rank = rank_ready(ready, avg)
        by_rank = {rank[m]: m for m in range(P) if ready[m]}
        losers = [m for m in range(P) if ready[m] and rank[m] >= R - q] if R >= 2 * q else []
        before = [row[:] for row in self.hp]
        self.rank_now = rank
        self.source_now = [-1] * P
        pairs = []
        for l in losers:
            w = philox4x64_10(np.array([[l, r, 0, 0]], np.uint64), self.seed, KEY1)[0]
            w0, w1 = int(w[0]), int(w[1])
            src = by_rank[source_rank(w0, q)]
            for k in range(4):
                v = before[src][k] * self.factor[(w1 >> k) & 1]
                if v < self.lo[k]:
                    v = self.lo[k]
                if v > self.hi[k]:
                    v = self.hi[k]
                self.hp[l][k] = v
            self.since[l] = episodes[l]
            self.replaced[l] += 1
            self.parent[l] = self.source_now[l] = src
            pairs.append((l, src))
        self.round += 1
        self.replaced_total += len(losers)
        return pairs

    def winners(self) -> list:
        """The members of rank < q after the last step (sources are drawn among them)."""
        return [m for m in range(self.P) if 0 <= self.rank_now[m] < self.q]

    def pack(self) -> bytes:
        """The state's bytes: header, then the members' records."""
        out = [struct.pack("<qqqq", self.round, self.replaced_total, 0, 0)]
        for m in range(self.P):
            out.append(struct.pack(MEMBER_FORMAT, self.since[m], self.replaced[m], self.source_now[m],
                                   self.rank_now[m], self.parent[m], 0, *self.hp[m]))
        return b"".join(out)


FAMILIES = ("distinct", "equal", "zeros", "inf", "nan", "interleaved", "exact", "short")


def board_family(family: str, P: int, q: int, min_episodes: int, seed: int = 0):
    """(episodes [P], avg [P]) of one of the board families both selection test modules use, for a
    selection whose ``since`` is all zero.

    distinct     every member ready, random distinct means
    equal        every member ready, one mean: ties fall to the index
    zeros        every member ready, -0.0 and +0.0 alternating (equal), one member above, one below
    inf          every member ready, random means with a +inf and a -inf
    nan          every member has the episodes, member 1 (and the last) a NaN mean: not ready
    interleaved  odd members one episode short of min_episodes, even ones ready
    exact        exactly 2 q members ready (R = 2 q), spread over the index range
    short        exactly 2 q - 1 members ready: nobody is replaced, rank_now is still written
    """
    rng = np.random.default_rng(seed)
    episodes = np.full(P, min_episodes + 3, np.int64) + rng.integers(0, 5, P)
    avg = rng.permutation(P).astype(np.float64) * 1.5 - 7.25 + rng.uniform(0, 0.5, P)
    if family == "distinct":
        pass
    elif family == "equal":
        avg[:] = 3.75
    elif family == "zeros":
        avg[:] = np.where(np.arange(P) % 2 == 0, -0.0, 0.0)
        if P >= 4:
            avg[P // 2], avg[P - 1] = 1.0, -1.0
    elif family == "inf":
        avg[0] = -np.inf
        avg[P - 1] = np.inf
        if P >= 4:
            avg[1] = np.inf          # two equal infinities: the lower index first
    elif family == "nan":
        avg[min(1, P - 1)] = np.nan
        avg[P - 1] = -np.nan
    elif family == "interleaved":
        episodes[1::2] = min_episodes - 1
    elif family in ("exact", "short"):
        R = 2 * q if family == "exact" else 2 * q - 1
        on = set(np.round(np.linspace(0, P - 1, R)).astype(int).tolist()) if R > 1 else {P - 1}
        k = 0
        while len(on) < R:           # (rounding merged two positions)
            on.add(k)
            k += 1
        for m in range(P):
            if m not in on:
                episodes[m] = min_episodes - 1
    else:
        raise KeyError(family)
    return episodes, avg
