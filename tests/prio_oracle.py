"""Oracle (TEST INFRASTRUCTURE ONLY -- never imported by the product path) of the prioritized
population replay (include/sacenv_prioritized_replay.h, sac-agent_amd/csrc/sacenv_replay_prio.h): one
member's sum tree, the rows a store marks, explicit and TD-derived leaves with the highest batch
position winning, the stratified draw and the importance weights, restated on Python ints (node
sums, strata and offsets never leave exact integer arithmetic) with numpy only for the Philox
words (``ctr_sampler.philox4x64_10``) and for the two f64 formulas.
"""
from __future__ import annotations

import numpy as np

import ctr_sampler

FAN = 64
ONE = 65536
CAP = (1 << 31) - 1
KEY1 = 0x7072696F
HEADER_BYTES = 256
MAX_LEVELS = 6


def level_counts(M: int) -> list:
    """Entries per level: M leaves, then ceil(n / 64) nodes, until a level holds <= 64."""
    out = [int(M)]
    while out[-1] > FAN:
        out.append(-(-out[-1] // FAN))
    return out


def layout(M: int) -> dict:
    counts, off, offsets = level_counts(M), HEADER_BYTES, []
    for k, n in enumerate(counts):
        offsets.append(off)
        off = -(-(off + (4 if k == 0 else 8) * n) // 256) * 256
    return {"levels": len(counts), "count": counts, "offset": offsets, "member_bytes": off}


class Tree:
    """One member's priority state."""

    def __init__(self, M: int):
        self.M = int(M)
        self.leaf = [0] * self.M
        self.max_leaf = ONE
        self.calls = 0

    # ---- the tree over the leaves, rebuilt from nothing (the device repairs it in place)
    def levels(self) -> list:
        out = [list(self.leaf)]
        while len(out[-1]) > FAN:
            lo = out[-1]
            out.append([sum(lo[i:i + FAN]) for i in range(0, len(lo), FAN)])
        return out

    def total(self) -> int:
        return sum(self.leaf)

    def to_bytes(self) -> bytes:
        """The slab as the header lays it out."""
        L = layout(self.M)
        buf = np.zeros(L["member_bytes"], np.uint8)
        buf[0:8] = np.frombuffer(np.uint64(self.total()).tobytes(), np.uint8)
        buf[8:12] = np.frombuffer(np.uint32(self.max_leaf).tobytes(), np.uint8)
        buf[16:24] = np.frombuffer(np.int64(self.calls).tobytes(), np.uint8)
        for k, (lv, off) in enumerate(zip(self.levels(), L["offset"])):
            raw = np.array(lv, np.uint32 if k == 0 else np.uint64).tobytes()
            buf[off:off + len(raw)] = np.frombuffer(raw, np.uint8)
        return buf.tobytes()

    # ---- writes
    def mark_stored(self, cntr: int, n: int) -> None:
        """The rows a store of n rows at count ``cntr`` writes get max_leaf."""
        M = self.M
        first = max(n - M, 0)
        for j in range(n - first):
            self.leaf[(cntr + first + j) % M] = self.max_leaf

    def set(self, idx, leaves) -> None:
        """Explicit leaves, clamped; an idx outside the ring is skipped; of equal idx the highest
        position wins; max_leaf follows the leaves written."""
        win = {}
        for i, v in zip(idx, leaves):
            i = int(i)
            if 0 <= i < self.M:
                win[i] = min(max(int(v), 1), CAP)       # (a later position replaces an earlier one)
        for i, v in win.items():
            self.leaf[i] = v
        if win:
            self.max_leaf = max(self.max_leaf, max(win.values()))

    def update_td(self, idx, sq1, sq2, alpha: float, eps: float) -> None:
        self.set(idx, td_leaves(sq1, sq2, alpha, eps))

    # ---- the draw
    def draw(self, B: int, call: int, m: int, seed: int, descend: bool = True, total: int | None = None):
        """(idx [B] i64, leaf [B] u32, t [B] python ints) of one sample. ``descend=False`` finds
        each row in the running sum of the leaves instead of walking the levels: the same rows,
        since every node is the exact sum of its children (tests/test_prioritized_replay_cpu.py
        holds the two against each other), and much faster for a population's worth of draws.
        ``total``: the header's total where it is not the leaves' sum (a tree that does not add up);
        a slot whose t reaches past the leaves' sum finds no child at the top level: idx -1, leaf 0."""
        levels, real = self.levels(), self.total()
        T = real if total is None else int(total)
        idx, leaf, ts = np.full(B, -1, np.int64), np.zeros(B, np.uint32), []
        if T == 0 or B == 0:
            return idx, leaf, ts
        ctr = np.zeros((B, 4), np.uint64)
        ctr[:, 0] = np.arange(B, dtype=np.uint64)
        ctr[:, 1] = np.uint64(call)
        ctr[:, 2] = np.uint64(m)
        words = ctr_sampler.philox4x64_10(ctr, np.uint64(seed), np.uint64(KEY1))[:, 0]
        for j in range(B):
            lo, hi = stratum(T, B, j)
            t = lo + ((int(words[j]) * (hi - lo)) >> 64)
            ts.append(t)
            if not descend or t >= real:
                continue
            node = 0
            for lv in reversed(levels):
                acc = 0
                for f, v in enumerate(lv[node * FAN:(node + 1) * FAN]):
                    if acc + v > t:
                        break
                    acc += v
                else:
                    raise AssertionError("t >= the node's sum")
                t -= acc
                node = node * FAN + f
            idx[j], leaf[j] = node, self.leaf[node]
        if not descend:
            run = np.cumsum(np.array(self.leaf, np.uint64))          # (exact: T < 2^62)
            at = np.searchsorted(run, np.array(ts, np.uint64), side="right").astype(np.int64)
            hit = at < self.M                                         # (t < the leaves' sum)
            idx[hit], leaf[hit] = at[hit], np.array(self.leaf, np.uint32)[at[hit]]
        return idx, leaf, ts


def stratum(T: int, B: int, j: int):
    """(lo_j, hi_j) as the device forms them: no product wider than 64 bits."""
    q, r = divmod(T, B)
    lo = q * j + (r * j) // B
    hi = q * (j + 1) + (r * (j + 1)) // B
    assert r * (j + 1) < 1 << 64 and hi < 1 << 64
    return lo, hi


def td_leaves(sq1, sq2, alpha: float, eps: float) -> np.ndarray:
    """leaf = clamp(floor(pow(0.5 (sqrt(sq1) + sqrt(sq2)) + eps, alpha) 65536), 1, 2^31 - 1) in f64;
    NaN gives 1, +inf the cap. ``sq2`` None: sqrt(sq1) + eps."""
    with np.errstate(invalid="ignore", over="ignore"):
        r1 = np.sqrt(np.asarray(sq1, np.float32).astype(np.float64))
        a = (r1 if sq2 is None else 0.5 * (r1 + np.sqrt(np.asarray(sq2, np.float32).astype(np.float64)))) + np.float64(eps)
        s = np.power(a, np.float64(alpha)) * 65536.0
        s = np.where(np.isnan(a), np.nan, s)             # (before the pow: pow(NaN, 0) is 1)
    out = np.ones(s.shape, np.uint32)
    ok = s >= 1.0                                        # (False for NaN)
    big = ok & (s >= float(CAP))
    out[big] = CAP
    mid = ok & ~big
    out[mid] = np.floor(s[mid]).astype(np.uint32)
    return out


def td_leaves_mp(sq1, sq2, alpha: float, eps: float, prec: int = 160):
    """(leaf u32 [n], decided bool [n]): ``td_leaves``' rule on the exact real numbers, in mpmath at
    ``prec`` >= 160 bits. The f32 inputs are taken exactly, ``alpha`` and ``eps`` as the f64 values
    passed; a = 0.5 (sqrt(sq1) + sqrt(sq2)) + eps (``sq2`` None: sqrt(sq1) + eps), s = a^alpha 65536,
    leaf = clamp(floor(s), 1, 2^31 - 1). A NaN or negative input (-0.0 is not negative) gives 1;
    alpha == 0 gives 65 536 for every other a, 0 and +inf included; a +inf input the cap; a == 0 gives 1.

    A row is undecided where s lies within s 2^-44 of an integer of [1, 2^31] (the thresholds 1 and
    2^31 - 1 among them): a chain of two square roots, two adds and a pow in f64, each within about
    an ulp and amplified by alpha <= 2, stays within a few 2^-52 s of s, and 2^-44 is more than 100
    times that. On a decided row every such chain gives this leaf; on the others it may give the
    next integer. alpha == 0 rows are decided: pow(x, 0) is exactly 1."""
    import mpmath
    assert prec >= 160
    x1 = np.asarray(sq1, np.float32).astype(np.float64).ravel()
    x2 = None if sq2 is None else np.asarray(sq2, np.float32).astype(np.float64).ravel()
    alpha, eps = float(alpha), float(eps)
    assert alpha >= 0 and eps >= 0 and (x2 is None or x2.shape == x1.shape)
    leaf, decided = np.ones(x1.size, np.uint32), np.ones(x1.size, bool)
    with mpmath.workprec(prec):
        al, ep, margin = mpmath.mpf(alpha), mpmath.mpf(eps), mpmath.ldexp(1, -44)
        for i in range(x1.size):
            xs = [float(x1[i])] + ([] if x2 is None else [float(x2[i])])
            if any(np.isnan(x) or x < 0 for x in xs):
                continue                                             # 1
            if alpha == 0:
                leaf[i] = ONE
                continue
            if any(np.isinf(x) for x in xs):
                leaf[i] = CAP
                continue
            a = sum(mpmath.sqrt(mpmath.mpf(x)) for x in xs) / len(xs) + ep
            if a == 0:
                continue                                             # 1
            s = mpmath.power(a, al) * ONE
            n = int(mpmath.nint(s))
            decided[i] = not (1 <= n <= 1 << 31 and abs(s - n) <= s * margin)
            leaf[i] = min(max(int(mpmath.floor(s)), 1), CAP)
    return leaf.reshape(np.shape(sq1)), decided.reshape(np.shape(sq1))


def weights(leaf, beta: float) -> np.ndarray:
    """(min leaf / leaf)^beta in f64, rounded once to f32; 0 where the leaf is 0."""
    leaf = np.asarray(leaf, np.uint32)
    out = np.zeros(leaf.shape, np.float32)
    if leaf.size == 0:
        return out
    mn = np.float64(leaf.min())
    nz = leaf != 0
    out[nz] = np.power(mn / leaf[nz].astype(np.float64), np.float64(beta)).astype(np.float32)
    return out


def ulp_distance_f32(a, b) -> np.ndarray:
    """Distance in f32 units in the last place (finite values of one sign)."""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


__all__ = ["Tree", "layout", "level_counts", "stratum", "td_leaves", "td_leaves_mp", "weights", "ulp_distance_f32", "FAN", "ONE",
           "CAP", "KEY1"]
