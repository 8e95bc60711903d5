"""The wind curves of experiments 4, 5 and 6 in mpmath -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

``oracle/boat_oracle.py`` restates ``Wind`` (wind.py:12-99) in float64 numpy
through scipy's ``interp1d``. This module restates the same curve exactly
(mpmath at ``PREC`` bits), from float64 knot values taken as exact:

* the not-a-knot cubic through ``nk`` uniform knots, second derivatives from
  the (1, 4, 1) system with the two not-a-knot rows, sample ``i`` of ``L`` at
  knot coordinate ``i (nk - 1) / (L - 1)`` formed as an exact rational
  (wind.py:76-84 with no rounding of ``linspace``);
* the exact min and max over the L grid samples, their indices and the two
  renormalisation margins ``max - 1`` and ``0 - min`` (wind.py:86-90);
* the table: renormalised iff a sample is < 0 or > 1 (the branch can be forced),
  scaled by ``max_velocity`` (exp 4, exp 6 curve 0) or ``2 pi`` (exp 6 curve 1);
  exp 5 keeps the unit curve and rectifies it at 0.25 (wind.py:92-99);
* the exact value of a stored ``(y0, m0, y1, m1)`` piece at an exact ``t`` in the
  form of the kernel's ``spline_piece``, so a fit can be judged from the
  coefficients it stored.

``m`` is the second derivative over 6 in the knot coordinate, as the kernel
stores it. Everything is cached per process by the knots' bytes.
"""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

from boat_step_mp import PREC, err_units, mp, mpf, ulp  # noqa: F401  (re-exported)

EPS = float(np.finfo(np.float64).eps)
TWO_PI = mpf(float(np.pi)) * 2      # the reference's ``curve * np.pi * 2`` on the float64 np.pi
QUARTER = mpf(0.25)                 # the rectifier's bar, 0.5 / 2


# ---------------------------------------------------------------- the spline
@functools.lru_cache(maxsize=None)
def g_matrix(nk: int):
    """G with m = G y (rows of mpf): the (1, 4, 1) system, not-a-knot end rows."""
    A, R = mp.zeros(nk, nk), mp.zeros(nk, nk)
    A[0, 0], A[0, 1], A[0, 2] = 1, -2, 1
    A[nk - 1, nk - 3], A[nk - 1, nk - 2], A[nk - 1, nk - 1] = 1, -2, 1
    for j in range(1, nk - 1):
        A[j, j - 1], A[j, j], A[j, j + 1] = 1, 4, 1
        R[j, j - 1], R[j, j], R[j, j + 1] = 1, -2, 1
    cols = [mp.lu_solve(A, R[:, k]) for k in range(nk)]
    return [[cols[k][i] for k in range(nk)] for i in range(nk)]


def second_derivs(y):
    """m = G y for a list of mpf knot values."""
    G = g_matrix(len(y))
    return [mp.fsum(g * v for g, v in zip(row, y)) for row in G]


def knot_coord(i: int, nk: int, L: int):
    """(j, t) of sample i: interval and exact offset in it (t in [0, 1]; the last sample has t = 1)."""
    s = Fraction(i * (nk - 1), L - 1)
    j = min(int(s), nk - 2)
    r = s - j
    return j, mpf(r.numerator) / r.denominator


def piece(y0, m0, y1, m1, t):
    """spline_piece: u y0 + t y1 + (u^3 - u) m0 + (t^3 - t) m1, exactly."""
    y0, m0, y1, m1, t = (v if isinstance(v, mp.mpf) else mpf(float(v)) for v in (y0, m0, y1, m1, t))
    u = 1 - t
    return u * y0 + t * y1 + (u ** 3 - u) * m0 + (t ** 3 - t) * m1


def _key(kv) -> bytes:
    return np.ascontiguousarray(kv, np.float64).tobytes()


class Curve:
    """The exact unit curve of one knot vector on an L-sample grid."""

    def __init__(self, kv, L: int):
        self.kv = np.array(kv, np.float64)
        self.nk, self.L = len(self.kv), int(L)
        self.y = [mpf(float(v)) for v in self.kv]
        self.m = second_derivs(self.y)
        self._val: dict = {}
        self._ext = None

    def value(self, i: int):
        """The exact unit curve at grid index i."""
        v = self._val.get(i)
        if v is None:
            j, t = knot_coord(i, self.nk, self.L)
            v = self._val[i] = piece(self.y[j], self.m[j], self.y[j + 1], self.m[j + 1], t)
        return v

    def value_on(self, j: int, s):
        """The piece of interval j continued to knot coordinate s (mpf), inside it or not."""
        return piece(self.y[j], self.m[j], self.y[j + 1], self.m[j + 1], s - j)

    def approx(self) -> np.ndarray:
        """The whole curve in float64 (within ~1e-13 of exact for knots in [-2, 2]): only
        ever used to choose which samples ``extremes`` evaluates exactly."""
        nk, L = self.nk, self.L
        i = np.arange(L, dtype=np.int64)
        num = i * (nk - 1)
        j = np.minimum(num // (L - 1), nk - 2)
        t = (num - j * (L - 1)) / (L - 1)
        y = self.kv
        m = np.array([float(v) for v in self.m])
        u = 1 - t
        return u * y[j] + t * y[j + 1] + (u ** 3 - u) * m[j] + (t ** 3 - t) * m[j + 1]

    def extremes(self):
        """(min, argmin, max, argmax) over the L samples, exact; the first index on ties.
        Samples the float64 curve puts within 1e-9 of the scale of an extreme are
        evaluated exactly; the others cannot be extreme (the float64 curve's error is
        orders below that)."""
        if self._ext is None:
            a = self.approx()
            guard = 1e-9 * max(float(np.abs(self.kv).max()), float(np.abs(a).max()))
            lo = np.flatnonzero(a <= a.min() + guard)
            hi = np.flatnonzero(a >= a.max() - guard)
            mn, imn = min((self.value(int(i)), int(i)) for i in lo)
            mx, imx = max((self.value(int(i)), -int(i)) for i in hi)
            self._ext = (mn, imn, mx, -imx)
        return self._ext

    # -- wind.py:86-90
    def margins(self):
        """(max - 1, 0 - min): the curve is renormalised iff either is > 0."""
        mn, _, mx, _ = self.extremes()
        return mx - 1, -mn

    def renorm(self) -> bool:
        a, b = self.margins()
        return a > 0 or b > 0

    def decision_margin(self):
        """How far the renormalisation decision is from flipping (>= 0)."""
        return abs(max(self.margins()))

    def span(self):
        mn, _, mx, _ = self.extremes()
        return mx - mn

    def fold(self, v, branch=None):
        """The final unit curve from a raw value: min-max renormalised on ``branch``
        (None: the exact decision)."""
        if self.renorm() if branch is None else branch:
            mn, _, mx, _ = self.extremes()
            return (v - mn) / (mx - mn)
        return v

    def unit_value(self, i: int, branch=None):
        return self.fold(self.value(i), branch)

    def pairs(self, top, branch=None):
        """The exact folded, scaled (y, m) pairs [nk] the fit should store."""
        ren = self.renorm() if branch is None else branch
        span = self.span() if ren else mpf(1)
        return [(self.fold(y, branch) * top, m / span * top) for y, m in zip(self.y, self.m)]


_CURVES: dict = {}


def curve(kv, L: int) -> Curve:
    k = (_key(kv), int(L))
    if k not in _CURVES:
        _CURVES[k] = Curve(kv, L)
    return _CURVES[k]


def top_of(experiment: int, c: int, max_velocity: float):
    """The table scaling of curve c: max_velocity, 2 pi, or 1 for exp 5's unit curve."""
    if experiment == 4 or (experiment == 6 and c == 0):
        return mpf(float(max_velocity))
    if experiment == 6 and c == 1:
        return TWO_PI
    return mpf(1)


def table_value(cv: Curve, i: int, top, branch=None):
    """The exact table entry of sample i (exp 5: the unit curve the rectifier reads)."""
    return cv.unit_value(i, branch) * top


def rectifier(cv: Curve, i: int, branch=None):
    """Exp 5 (wind.py:92-99): (rect, margin): rect 0 where the final unit curve is <= 0.25,
    else 1; margin = curve - 0.25."""
    d = cv.unit_value(i, branch) - QUARTER
    return (0 if d <= 0 else 1), d


def stored_value(pairs, i: int, nk: int, L: int):
    """The exact value at sample i of stored float64 pairs [nk, 2] = (y, m)."""
    j, t = knot_coord(i, nk, L)
    return piece(pairs[j][0], pairs[j][1], pairs[j + 1][0], pairs[j + 1][1], t)


def critical_points(cv: Curve, j: int):
    """The roots of the derivative of piece j in [0, 1] (mpf offsets t), exact to PREC."""
    a, b = cv.m[j], cv.m[j + 1]
    qa, qb, qc = 3 * (b - a), 6 * a, cv.y[j + 1] - cv.y[j] - 2 * a - b
    if qa == 0:
        roots = [-qc / qb] if qb != 0 else []
    else:
        disc = qb * qb - 4 * qa * qc
        if disc < 0:
            return []
        sq = mp.sqrt(disc)
        roots = [(-qb - sq) / (2 * qa), (-qb + sq) / (2 * qa)]
    return [r for r in roots if 0 <= r <= 1]
