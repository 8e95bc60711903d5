"""The population scoreboard in plain Python (include/sacenv_scoreboard.h).

``np_mean`` writes numpy's summation order out (it is held against ``np.mean`` itself in
tests/test_scoreboard_cpu.py); ``BoardOracle`` keeps, per member, exactly the lines of
main.py:99-108 on a Python list and packs its state into the board's bytes.
"""
from __future__ import annotations

import struct

import numpy as np

HEADER_BYTES, MEMBER_BYTES = 32, 128
MEMBER_FORMAT = "<qqqqdddII8Q"     # SacenvBoardMember
assert struct.calcsize(MEMBER_FORMAT) == MEMBER_BYTES
# a NaN mean is stored as this one (the sign of a generated NaN is the hardware's: x86 sets it)
CANONICAL_NAN = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]


def np_mean(xs) -> float:
    """``np.mean`` of 1..128 doubles, numpy's order written out: below 8 values a running sum
    from -0.0; else eight accumulators from the first eight values, each taking every eighth
    value of the multiple-of-eight part, combined pairwise, the rest added in order. The
    reduction then adds that block sum to its own +0.0 start, which shows in one case: a sum of
    -0.0 becomes +0.0 (``np.mean([-0.0] * n)`` is +0.0 for every n)."""
    n = len(xs)
    assert 1 <= n <= 128
    if n < 8:
        res = -0.0
        for x in xs:
            res = res + x
    else:
        r = [float(x) for x in xs[:8]]
        whole = n - n % 8
        for i in range(8, whole, 8):
            for j in range(8):
                r[j] = r[j] + xs[i + j]
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for x in xs[whole:]:
            res = res + x
    res = 0.0 + res
    return float(np.float64(res) / np.float64(n))     # (np.float64: inf / n without Python's exceptions)


class Member:
    def __init__(self):
        self.history = []
        self.episodes = self.saves = 0
        self.last_save_step = self.last_end_step = -1
        self.last = self.avg = 0.0
        self.best = float("-inf")
        self.saved_now = 0
        self.terms = [0] * 8

    def episode(self, score: float, end_step: int, term: int, L: int) -> bool:
        """main.py:99-108 for one finished episode; True if it saves."""
        score = float(score)
        self.history.append(score)
        self.avg = np_mean(self.history[-L:])
        if score > self.best:
            self.best = score
        saved = score > self.avg
        if saved:
            self.saves += 1
            self.last_save_step = int(end_step)
            self.saved_now = 1
        self.last = score
        self.last_end_step = int(end_step)
        self.episodes += 1
        self.terms[min(int(term), 7)] += 1
        return saved


class BoardOracle:
    def __init__(self, members: int, envs_per_member: int, lookback: int, cap: int, env_base: int = 0):
        self.P, self.N, self.L, self.cap, self.env_base = members, envs_per_member, lookback, cap, env_base
        self.cursor = self.missed = self.calls = 0
        self.members = [Member() for _ in range(members)]

    def update(self, total: int, entries) -> list:
        """``sacenv_board_update`` on a log whose header holds ``total`` and whose entries are
        ``entries`` (anything indexable by position with fields env, score, end_step, term; at
        least ``min(total, cap)`` long). Returns the members that saved in this call."""
        total = max(int(total), self.cursor)
        lo, hi = min(self.cursor, self.cap), min(total, self.cap)
        for mem in self.members:
            mem.saved_now = 0
        for i in range(lo, hi):
            e = entries[i]
            d = int(e["env"]) - self.env_base
            if d < 0 or d // self.N >= self.P:
                continue
            self.members[d // self.N].episode(float(e["score"]), int(e["end_step"]), int(e["term"]), self.L)
        self.missed += max(total, self.cap) - max(self.cursor, self.cap)
        self.cursor = total
        self.calls += 1
        return [m for m, mem in enumerate(self.members) if mem.saved_now]

    def rewind(self) -> None:
        self.cursor = 0

    def pack(self) -> bytes:
        """The board's bytes: header, the members' records, the members' rings."""
        out = [struct.pack("<qqqq", self.cursor, self.missed, self.calls, 0)]
        for mem in self.members:
            out.append(struct.pack(MEMBER_FORMAT, mem.episodes, mem.saves, mem.last_save_step, mem.last_end_step,
                                   mem.last, mem.best, CANONICAL_NAN if mem.avg != mem.avg else mem.avg,
                                   mem.saved_now, 0, *mem.terms))
        for mem in self.members:
            ring = [0.0] * self.L
            for i in range(max(mem.episodes - self.L, 0), mem.episodes):
                ring[i % self.L] = mem.history[i]
            out.append(struct.pack(f"<{self.L}d", *ring))
        return b"".join(out)


FAMILIES = ("random", "equal", "negzero", "nan", "inf", "ties")


def scores(family: str, n: int, L: int, seed: int = 0) -> np.ndarray:
    """n f64 scores of one of the families both scoreboard test modules use.

    random   magnitudes 1e-3 .. 1e6, either sign
    equal    one value throughout, whose multiples up to 128 are exact: a tie at every episode,
             so no save ever
    negzero  all -0.0 (numpy's mean of them is +0.0: its sum starts from +0.0)
    nan      random with a NaN in the middle (every window that holds it has a NaN mean)
    inf      random with +inf and then -inf (windows with one, then both)
    ties     runs of one exactly summable value v, then nextafter(v, +inf) and nextafter(v, -inf):
             score - mean is exactly 0 and one ulp either way
    """
    rng = np.random.default_rng(seed)
    rand = 10.0 ** rng.uniform(-3, 6, n) * rng.choice([-1.0, 1.0], n)
    if family == "random":
        return rand
    if family == "equal":
        return np.full(n, 3.75)
    if family == "negzero":
        return np.full(n, -0.0)
    if family == "nan":
        rand[n // 2] = np.nan
        return rand
    if family == "inf":
        rand[n // 3] = np.inf
        rand[2 * n // 3] = -np.inf
        return rand
    if family == "ties":
        out = []
        for v in (1.5, 96.0, -0.375, 1.5, 80.0, -3.0, 0.75, 640.0):
            out += [v] * (L + 3) + [np.nextafter(v, np.inf), np.nextafter(v, -np.inf), v, v]
        reps = -(-n // len(out))
        return np.array((out * reps)[:n])
    raise KeyError(family)
