"""The inputs of the prioritized replay's edge tests (TEST INFRASTRUCTURE ONLY), shared by
tests/test_prioritized_edges_cpu.py and tests/test_prioritized_edges_gpu.py so that what the CPU
tests establish about the oracle (undecided rows <= 1 %, the bar's teeth, where a batch's smallest
leaf sits) holds for exactly the inputs the GPU tests run. See tests/prio_oracle.py for the oracle.
"""
from __future__ import annotations

import numpy as np

import prio_oracle

FLT_MIN, FLT_MAX = np.float32(2.0 ** -126), np.finfo(np.float32).max

# squared TD errors at the edges of prio_td_leaf: zeros of both signs, the least subnormal, values whose
# leaf is below 1, exact squares, values past the cap, the non-finite and the negative, and 2^-32
# (sqrt x 65536 = 1 exactly, the lower threshold)
EDGES = np.array([0.0, -0.0, 1e-45, FLT_MIN, 1e-30, 1e-12, 1e-6, 0.25, 1.0, 4.0, 16.0, 1e4, 1e9, 1e19, FLT_MAX,
                  np.inf, np.nan, -1.0, -np.inf, 2.0 ** -32], np.float32)

# (alpha, eps). alpha = 2 only with eps = 1e-3: with eps = 0 and one critic sqrt(x)^2 x 65536 is an
# integer for many f32 x, and 214 of 1 520 rows are undecided.
ALPHA_EPS = tuple((a, e) for a in (0.0, 0.3, 0.5, 0.6, 1.0, 1.7) for e in (0.0, 1e-3)) + ((2.0, 1e-3),)
UNDECIDED_CAP = 0.01                   # at most this share of an input set's rows may be undecided

TD_ROWS = 1500                         # two chunks of the writing workgroup (1 024 positions each)
TD_M, TD_P = 4097, 2


def log_range(alpha: float):
    """(lo, hi) of the log-uniform squared TD errors: [1e-6, 1e14] at alpha = 0.6 and the matching
    ends for other exponents, sqrt(hi)^alpha x 65536 = 10^4.2 x 65536 = 1.04e9 < 2^31 (nothing is
    capped) and a fifth of the range above the 2^26 of a leaf (of two critics' mean: a third)."""
    a = alpha if alpha > 0 else 0.6
    return 10.0 ** (-3.6 / a), 10.0 ** (8.4 / a)


def log_uniform(alpha: float, n: int, rng) -> np.ndarray:
    lo, hi = log_range(alpha)
    return (10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)).astype(np.float32)


def td_inputs(alpha: float, eps: float, member: int = 0, rows: int = TD_ROWS):
    """(sq1, sq2) f32 [rows] of one member: EDGES first in sq1, reversed in sq2, then log-uniform."""
    rng = np.random.default_rng([round(alpha * 10), round(eps * 1e4), member, rows])
    sq1, sq2 = log_uniform(alpha, rows, rng), log_uniform(alpha, rows, rng)
    sq1[: EDGES.size], sq2[: EDGES.size] = EDGES, EDGES[::-1]
    return sq1, sq2


def td_rows(member: int, rows: int = TD_ROWS, M: int = TD_M) -> np.ndarray:
    """Distinct ring rows for the batch's positions: position i writes row td_rows[i]."""
    return np.random.default_rng([77, member]).permutation(M)[:rows]


def td_case(alpha: float, eps: float, two: bool, member: int = 0):
    """(sq1, sq2 or None, leaf, decided) of one input set, the exact oracle's."""
    sq1, sq2 = td_inputs(alpha, eps, member)
    leaf, decided = prio_oracle.td_leaves_mp(sq1, sq2 if two else None, alpha, eps)
    return sq1, (sq2 if two else None), leaf, decided


def td_leaves_variant(sq1, sq2, alpha: float, eps: float, pow32: bool = False, rint: bool = False) -> np.ndarray:
    """``prio_oracle.td_leaves`` with one thing wrong: the pow carried out in float32, or a
    round-to-nearest in place of the floor (what the bar must notice)."""
    with np.errstate(invalid="ignore", over="ignore"):
        r1 = np.sqrt(np.asarray(sq1, np.float32).astype(np.float64))
        a = (r1 if sq2 is None else 0.5 * (r1 + np.sqrt(np.asarray(sq2, np.float32).astype(np.float64)))) + eps
        if pow32:
            s = np.power(a.astype(np.float32), np.float32(alpha)).astype(np.float64) * 65536.0
        else:
            s = np.power(a, np.float64(alpha)) * 65536.0
        s = np.where(np.isnan(a), np.nan, s)
    out = np.ones(s.shape, np.uint32)
    ok = s >= 1.0
    big = ok & (s >= float(prio_oracle.CAP))
    out[big] = prio_oracle.CAP
    mid = ok & ~big
    out[mid] = (np.rint(s[mid]) if rint else np.floor(s[mid])).astype(np.uint32)
    return out


# ---- the draws at the size edges

BIG_M, BIG_P = 4097, 2
BIG_BATCHES = (1025, 2048, 2500)       # past one stride of prio_finish_body's 1 024 threads
BIG_SEEDS = (1000, 1007)
# (B, the sample's number) of every big draw the GPU tests make: two host-numbered and two
# device-counted samples per B on one replay, whose counts run on; four annealed ones at 2 048
BIG_DRAWS = tuple((B, 2 * i + k) for i, B in enumerate(BIG_BATCHES) for k in (0, 1))
ANNEALED_DRAWS = tuple((2048, k) for k in range(4))


def big_fill(member: int, M: int = BIG_M) -> np.ndarray:
    """Leaves in [2^20, 2^21) below M // 2 and in [1000, 2000) from there on: the small leaves hold
    a thousandth of the total, so a batch's last stratum or two fall among them and its smallest
    leaf sits at the end of the batch."""
    rng = np.random.default_rng([5, member])
    leaf = rng.integers(1 << 20, 1 << 21, M)
    leaf[M // 2:] = rng.integers(1000, 2000, M - M // 2)
    return leaf


def cap_fill(member: int, M: int = BIG_M) -> np.ndarray:
    """Leaves in [2^30, 2^31), every third the cap, every seventh from row 1 equal to 1: level-1
    sums of 37 bits and a total of 43."""
    leaf = np.random.default_rng([6, member]).integers(1 << 30, 1 << 31, M)
    leaf[::3] = prio_oracle.CAP
    leaf[1::7] = 1
    return leaf


def weights_first_stride(leaf, beta: float, stride: int = 1024) -> np.ndarray:
    """``prio_oracle.weights`` with the minimum taken over the first ``stride`` positions only."""
    leaf = np.asarray(leaf, np.uint32)
    mn = np.float64(leaf[:stride].min())
    return np.power(mn / leaf.astype(np.float64), np.float64(beta)).astype(np.float32)


def tree_of(leaves) -> prio_oracle.Tree:
    t = prio_oracle.Tree(len(leaves))
    t.set(np.arange(len(leaves)), leaves)
    return t
