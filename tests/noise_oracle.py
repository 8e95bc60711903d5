"""The policy-noise contract of include/sacenv_noise.h, restated twice (a helper of
test_policy_noise_cpu.py / test_policy_noise_gpu.py, not a test; never imported by the product).

Element i of call c of stream s under seed S: w = Philox4x64-10 of counter (i div 4, c, s, 0)
under key (S, 0x6E6F697365); p = (i mod 4) div 2; u1 = ((w[2p] >> 11) + 1) 2^-53,
u2 = (w[2p+1] >> 11) 2^-53; z = sqrt(-2 log u1) x (cospi(2 u2) for even i, sinpi(2 u2) for odd i),
in f64; the value is (float)z.

* ``normal_np``: numpy f64 on ``ctr_sampler.philox4x64_10`` (oracle/, itself pinned to numpy's
  Philox), for bulk checks. cospi / sinpi reduce their argument exactly (to a multiple of 1/2
  plus a remainder in [-1/4, 1/4]) before they meet pi, so the relative error stays at a few f64
  ulp next to a zero.
* ``normal_mp``: mpmath at 120 bits, rounded ONCE to f32 (24 bits, to nearest even): the exact
  value.

``ulp_distance`` counts f32 steps between two arrays; ``statistics`` gives the eleven statistics
the tests bound, each in units of its own sampling error under N(0, 1).
"""
from __future__ import annotations

import math

import numpy as np

from ctr_sampler import philox4x64_10

KEY1 = 0x6E6F697365
ACT, LEARN1, LEARN2 = 0, 1, 2
BOUND = 8.58          # |z| <= sqrt(106 ln 2) = 8.5717...
_2M53 = 2.0 ** -53


def words(seed: int, stream: int, call: int, n: int) -> np.ndarray:
    """The Philox blocks of a row of n values: uint64 [ceil(n / 4), 4]."""
    nb = (int(n) + 3) // 4
    ctr = np.zeros((nb, 4), np.uint64)
    ctr[:, 0] = np.arange(nb, dtype=np.uint64)
    ctr[:, 1] = np.uint64(call)
    ctr[:, 2] = np.uint64(stream)
    return philox4x64_10(ctr, np.uint64(seed), np.uint64(KEY1))


def _sincospi(x: np.ndarray):
    """(sinpi(x), cospi(x)) for f64 x in [0, 2), argument reduction exact."""
    q = np.floor(2.0 * x + 0.5)                 # nearest multiple of 1/2, as a count: 0 .. 4
    f = x - 0.5 * q                             # exact, in [-1/4, 1/4]
    s, c = np.sin(np.pi * f), np.cos(np.pi * f)
    k = q.astype(np.int64) & 3
    sin = np.choose(k, [s, c, -s, -c])
    cos = np.choose(k, [c, -s, -c, s])
    return sin, cos


def normal_np(seed: int, stream: int, call: int, n: int) -> np.ndarray:
    """f32 [n]: the contract in numpy f64."""
    w = words(seed, stream, call, n)
    out = np.empty((w.shape[0], 4), np.float64)
    for p in (0, 1):
        u1 = ((w[:, 2 * p] >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * _2M53
        u2 = (w[:, 2 * p + 1] >> np.uint64(11)).astype(np.float64) * _2M53
        r = np.sqrt(-2.0 * np.log(u1))
        s, c = _sincospi(2.0 * u2)
        out[:, 2 * p] = r * c
        out[:, 2 * p + 1] = r * s
    return out.reshape(-1)[: int(n)].astype(np.float32)


def normal_mp(seed: int, stream: int, call: int, n: int) -> np.ndarray:
    """f32 [n]: the contract in mpmath at 120 bits, rounded once to f32."""
    import mpmath
    w = words(seed, stream, call, n)
    out = np.empty(int(n), np.float32)
    with mpmath.workprec(120):
        for i in range(int(n)):
            p = (i % 4) // 2
            u1 = mpmath.mpf(int(w[i // 4, 2 * p] >> np.uint64(11)) + 1) / (1 << 53)
            u2 = mpmath.mpf(int(w[i // 4, 2 * p + 1] >> np.uint64(11))) / (1 << 53)
            r = mpmath.sqrt(-2 * mpmath.log(u1))
            z = r * (mpmath.cospi(2 * u2) if i % 2 == 0 else mpmath.sinpi(2 * u2))
            with mpmath.workprec(24):           # one rounding, to f32's 24 bits (|z| is 0 or far
                z32 = +z                        # above f32's subnormals: >= 2^-52 x 1e-8)
            out[i] = np.float32(float(z32))
            assert float(out[i]) == float(z32)
    return out


def _ordered(x: np.ndarray) -> np.ndarray:
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)     # monotone in the value; +0 and -0 coincide


def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """f32 steps between a and b, elementwise (int64)."""
    return np.abs(_ordered(a) - _ordered(b))


STATISTICS = ("mean", "variance", "third moment", "fourth moment", "tail 0.5", "tail 1", "tail 2", "tail 3",
              "sign", "lag-1 correlation", "even/odd correlation")


def statistics(x: np.ndarray) -> dict:
    """{name: (value - expectation) / sampling error} of the eleven statistics over N values of
    a row (N even). Expectations and errors are N(0, 1)'s own: Var x^2 = 2, Var x^3 = 15,
    Var x^4 = 105 - 9; a fraction p has error sqrt(p (1 - p) / N); a product of two independent
    normals has variance 1, and so has the product of a Box-Muller pair (E r^4 E cos^2 sin^2 =
    8 x 1/8)."""
    x = np.asarray(x, np.float64)
    N = x.size
    out = {"mean": x.mean() * math.sqrt(N),
           "variance": (x.var() - 1.0) / math.sqrt(2.0 / N),
           "third moment": (x ** 3).mean() / math.sqrt(15.0 / N),
           "fourth moment": ((x ** 4).mean() - 3.0) / math.sqrt(96.0 / N)}
    for t in (0.5, 1, 2, 3):
        p = math.erfc(t / math.sqrt(2.0))
        out[f"tail {t}"] = ((np.abs(x) > t).mean() - p) / math.sqrt(p * (1 - p) / N)
    out["sign"] = ((x > 0).mean() - 0.5) / math.sqrt(0.25 / N)
    out["lag-1 correlation"] = (x[:-1] * x[1:]).mean() * math.sqrt(N - 1)
    out["even/odd correlation"] = (x[0::2] * x[1::2]).mean() * math.sqrt(N // 2)
    assert tuple(out) == STATISTICS
    return out
