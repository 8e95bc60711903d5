"""The committed case list of the wind fit's parity tests, its units and bars, and the
one function that measures a fit against oracle/wind_fit_mp.py.
TEST INFRASTRUCTURE, NOT PRODUCT CODE.

One env per case, deterministic, no filter: every listed case is checked. A case
holds the knot values [2, nk] of one env (experiments 4 and 5 read curve 0 only).

Configs (``CONFIGS``): ``(experiment, nk, L)`` with ``L = int(t_max / dt)`` at dt 0.25:
the default (8 knots, 10 000 samples) for experiments 6, 4 and 5, and for experiment 6
few samples per interval (L 20, 37), intervals with no grid sample (L 5), one cubic
over all pieces (4 knots), the 8-lane group not full (5), 8 and 9 intervals (9 and
10 knots: four lanes or one per interval in the wave fit) and the 16-lane group, not
full (12) and full (16). At most 16 curves per config at L = 10 000.

Families: ``random`` (``RandomState.random_sample`` knots), ``renorm_edge`` (the exact
grid max at 1 + k ulp(1) and / or the exact grid min at 0 - k 2^-53, k in +-1, +-2, +-8,
+-64, +-2^20; knots rounded to float64 and the margin re-measured; end knots of exactly
0.0 and 1.0), ``shape`` (constants, exact linear ramps, unit spikes, alternating 0/1, a
flat interval in a monotone curve, mirror-symmetric knots, knots of 2^-53 and 1e-300,
an all-zero curve whose every m[j] is exactly 0, and cubic knots s (x^3 - x) + 1/2 whose
float64 m[1] is exactly 0 with the host's G, so qb == 0 beside qa, qc != 0; the device
forms its own G, so there qb may be a rounding away from 0), ``critical`` (one knot tuned so that
the critical point that is the curve's grid extreme lies a chosen fraction of a grid
step from a sample; the extreme is far outside [0, 1]) and ``rectifier`` (exp 5: a grid
sample of the final unit curve at 0.25 +- k ulp).

Rungs left out. The budget of 16 curves at L = 10 000 does not hold a whole ladder, and
half of a near-tie family must be decisive, which only the 2^20 rungs are at these bars:
exp 6 and 4 at L = 10 000 carry the renorm_edge rungs listed in ``build``; exp 5 carries
the rectifier rungs +1, -1, +8, -64 and +-2^20 (seven of the latter) and lacks +-2, -8 and
+64. Every config at L <= 400 carries the whole renorm_edge ladder in all three modes.

Units and bars: the absolute error in ``eps x top`` (top: max_velocity, 2 pi, or 1 for
exp 5's unit curve), for a renormalised curve divided by the exact span max - min where
that is below 1 (the condition number of the renormalisation: the reference pays it
too). ``C_REF`` is the numpy reference's (boat_oracle.wind_from_knots) worst error per
config over the decisive cases, written here by tools/wind_fit_margins.py; the kernel's
bar is ``BAR_FACTOR x C_REF`` at each of its two stages (the reference has none):
``fit``, the stored (y, m) pairs evaluated exactly at the exact t against the exact
table, and ``eval``, ``wind_eval``'s value against the exact value of the stored piece.

Near ties: a renormalisation (or rectifier) decision is decisive when its exact margin
exceeds the bar in absolute terms; a decisive case must take the exact branch, any
other may take either but is then held to that branch's exact table.
"""
from __future__ import annotations

import numpy as np

import wind_fit_mp as W
from boat_oracle import OracleConfig, wind_from_knots
from boat_step_cases import BAR_FACTOR

MAX_VELOCITY = 0.5
K_RUNGS = (1, -1, 2, -2, 8, -8, 64, -64, 2 ** 20, -2 ** 20)
DISTANCES = (0.0, 1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3, 0.5)
STAGES = ("fit", "eval")
NEAR_TIE = ":near_tie"
SMALL_L = 400          # up to here every index is judged

CONFIGS = {
    "e6_k8_L10000": (6, 8, 10000),
    "e4_k8_L10000": (4, 8, 10000),
    "e5_k8_L10000": (5, 8, 10000),
    "e6_k8_L20": (6, 8, 20),
    "e6_k8_L37": (6, 8, 37),
    "e6_k8_L5": (6, 8, 5),
    "e6_k4_L400": (6, 4, 400),
    "e6_k5_L120": (6, 5, 120),
    "e6_k9_L120": (6, 9, 120),
    "e6_k10_L120": (6, 10, 120),
    "e6_k12_L120": (6, 12, 120),
    "e6_k16_L37": (6, 16, 37),
    "e6_k16_L10000": (6, 16, 10000),
}

# The numpy reference's worst error per config over the decisive cases, in eps x top
# (tools/wind_fit_margins.py writes this block; tests/test_wind_fit_mp_cpu.py checks it
# against profiles/wind_fit_margins.json).
# --- C_REF begin
C_REF = {'e6_k8_L10000': 12.726793275229936,
 'e4_k8_L10000': 11.588844525723859,
 'e5_k8_L10000': 8.682159451391989,
 'e6_k8_L20': 3.629576879523121,
 'e6_k8_L37': 4.665178788025812,
 'e6_k8_L5': 1.7973515023752369,
 'e6_k4_L400': 4.498251115993571,
 'e6_k5_L120': 4.404638823348529,
 'e6_k9_L120': 6.4487336461704166,
 'e6_k10_L120': 5.9662043294632205,
 'e6_k12_L120': 7.608307625508982,
 'e6_k16_L37': 13.269861105885862,
 'e6_k16_L10000': 19.34150232745729}
# --- C_REF end


def bar(config: str) -> float:
    return BAR_FACTOR * C_REF[config]


def oracle_config(name: str) -> OracleConfig:
    exp, nk, L = CONFIGS[name]
    return OracleConfig(experiment=exp, fixed_points=nk, t_max=L * 0.25, max_velocity=MAX_VELOCITY)


def env_config(name: str) -> dict:
    """The same config in the reference's YAML layout (sacenv.BoatConfig.from_any)."""
    c = oracle_config(name)
    return {"base_settings": {"experiment": c.experiment, "test_mode": 0, "dt": c.dt, "t_max": c.t_max},
            "wind": {"fixed_points": c.fixed_points, "max_velocity": c.max_velocity}}


# ---------------------------------------------------------------- building blocks
def _round(vals) -> np.ndarray:
    return np.array([float(v) for v in vals], np.float64)


def affine(kv, L, lo=None, hi=None) -> np.ndarray:
    """``a kv + b`` rounded to float64, with the exact grid min at ``lo`` and / or the exact
    grid max at ``hi`` before the rounding (the spline is affine in its knots); with one
    target the other extreme keeps its distance to it."""
    cv = W.curve(kv, L)
    mn, _, mx, _ = cv.extremes()
    if lo is not None and hi is not None:
        a = (W.mpf(hi) - W.mpf(lo)) / (mx - mn)
        b = W.mpf(lo) - a * mn
    elif hi is not None:
        a, b = W.mpf(1), W.mpf(hi) - mx
    else:
        a, b = W.mpf(1), W.mpf(lo) - mn
    return _round(a * y + b for y in cv.y)


def inside(kv, L, lo=0.125, hi=0.875) -> np.ndarray:
    """The curve mapped to have its grid extremes at [lo, hi]: decisively not renormalised."""
    return affine(kv, L, lo, hi)


def edge_targets(mode: str, k: int):
    """(lo, hi) of a renorm_edge curve: max at 1 + k ulp(1) and / or min at 0 - k 2^-53."""
    hi = W.mpf(1) + k * W.mpf(2) ** -52
    lo = -k * W.mpf(2) ** -53
    return {"max": (W.mpf(0.125), hi), "min": (lo, W.mpf(0.875)), "both": (lo, hi)}[mode]


def smooth_end_knots(nk: int) -> np.ndarray:
    """A monotone curve from exactly 0.0 to exactly 1.0: the first and last samples sit on
    the end knots, so the grid min and max are exactly 0 and 1."""
    x = np.arange(nk) / (nk - 1)
    kv = x.copy()
    kv[0], kv[-1] = 0.0, 1.0
    return kv


def shapes(nk: int, rng) -> list:
    """(label, knots, tie_ok) of the shape family at nk knots."""
    out = []
    below1 = float(np.nextafter(1.0, 0.0))
    out.append(("all knots 0.0 (every m[j] exactly 0: qb == 0; end knots 0.0: every sample on the bar)",
                np.zeros(nk), True))
    out.append(("all knots 0.5", np.full(nk, 0.5), False))
    out.append((f"all knots {below1!r} (every sample half an ulp under the bar)", np.full(nk, below1), True))
    ramp = np.arange(nk) / 16.0
    out.append(("exact linear ramp up (m = 0, qa noise)", ramp + 1 / 32, False))
    out.append(("exact linear ramp down", ramp[::-1] + 1 / 32, False))
    for k in range(nk):
        out.append((f"unit spike e_{k}", np.eye(nk)[k], False))
    alt = (np.arange(nk) % 2).astype(np.float64)
    out.append(("alternating 0/1", alt, False))
    out.append(("alternating 1/0", 1 - alt, False))
    mono = np.sort(0.2 + 0.6 * rng.random_sample(nk))
    mono[nk // 2] = mono[nk // 2 - 1]
    out.append(("a flat interval inside a monotone curve", mono, False))
    half = 0.1 + 0.8 * rng.random_sample((nk + 1) // 2)
    sym = np.concatenate([half, half[::-1][nk % 2:]])
    out.append(("mirror-symmetric knots (critical point at the centre)", sym, False))
    sym2 = sym.copy()
    sym2[(nk - 1) // 2] = sym2[nk // 2] = 1.5
    out.append(("mirror-symmetric knots, peak 1.5 at the centre", sym2, False))
    # (tiny knots: the whole curve lies within the bar of 0, a near tie by its size)
    out.append(("spike of 2^-53 (tiny: a near tie by its size)", np.eye(nk)[nk // 2] * 2.0 ** -53, True))
    out.append(("spike of 1e-300 (tiny: a near tie by its size)", np.eye(nk)[1] * 1e-300, True))
    pat = rng.random_sample(nk)
    out.append(("knots of 1e-300 x random (tiny: a near tie by its size)", pat * 1e-300, True))
    out.append(("cubic knots with m[1] exactly 0 (qb == 0, roots +-sqrt(1/3))", inflection_knots(nk), False))
    assert all(len(k) == nk for _, k, _ in out)
    return out


def inflection_knots(nk: int) -> np.ndarray:
    """``s (x^3 - x) + 1/2`` at x = j - 1, s the largest power of two that keeps the cubic
    part within 1: the inflection sits on knot 1, and the float64 m = G y (the host's
    sacenv.config.spline_g) has m[1] == 0 exactly and no other zero, so interval 1's
    derivative is qa t^2 + qc with qb == 0: roots +-sqrt(1/3)."""
    from sacenv.config import spline_g
    x = np.arange(nk) - 1.0
    s = 2.0 ** -int(np.ceil(np.log2(np.abs(x ** 3).max())))
    y = (x ** 3 - x) * s + 0.5
    m = spline_g(nk) @ y
    assert m[1] == 0.0 and np.count_nonzero(m == 0.0) == 1, "no exact zero: search another scale"
    return y


def _peak(cv, p: int, want_max: bool):
    """(knot coordinate, value) of the critical point next to knot p that is the curve's
    peak (want_max) or trough."""
    best = None
    for j in (p - 1, p):
        for t in W.critical_points(cv, j):
            v = cv.value_on(j, j + t)
            if best is None or (v > best[1] if want_max else v < best[1]):
                best = (j + t, v)
    return best


def critical_case(nk: int, L: int, d: float, rng, want_max: bool):
    """Knots whose peak (or trough) critical point lies ``d`` grid steps from a grid sample;
    the knot after the peak is tuned by bisection, then rounded. Returns (knots, info) with
    the re-measured distance."""
    p = nk // 2
    kv = 0.3 + 0.4 * rng.random_sample(nk)
    kv[p] = 1.6
    if not want_max:
        kv = 1.0 - kv
    q = p + 1
    inv = W.mpf(L - 1) / (nk - 1)

    def loc(x):
        k2 = kv.copy()
        k2[q] = float(x)
        cvq = W.Curve(k2, L)
        cvq.y[q] = W.mpf(x)           # the tuned knot at full precision while bisecting
        cvq.m = W.second_derivs(cvq.y)
        return _peak(cvq, p, want_max)[0]

    xa, xb = (W.mpf(0.0), W.mpf(1.55)) if want_max else (W.mpf(-0.55), W.mpf(1.0))
    la, lb = loc(xa), loc(xb)
    rising = lb > la
    s_lo, s_hi = (la, lb) if rising else (lb, la)
    cands = [i for i in range(L) if s_lo * inv < i + d < s_hi * inv]
    assert cands, "no grid sample within the peak's reach"
    i0 = cands[len(cands) // 2]
    target = (i0 + W.mpf(d)) / inv
    for _ in range(90):
        xm = (xa + xb) / 2
        if (loc(xm) < target) == rising:
            xa = xm
        else:
            xb = xm
    kv[q] = float((xa + xb) / 2)
    s, _ = _peak(W.Curve(kv, L), p, want_max)
    return kv, dict(i0=i0, target=d, dist=float(s * inv - i0), want_max=want_max)


def rectifier_case(kv, L: int, k: int):
    """Exp 5: the curve shifted so that one grid sample of the (not renormalised) unit curve
    sits at 0.25 + k ulp(0.25); returns (knots, index, re-measured margin to 0.25)."""
    base = inside(kv, L, 0.0625, 0.9375)
    cv = W.curve(base, L)
    a = cv.approx()
    slope = np.abs(np.gradient(a))
    ok = np.flatnonzero((slope > 0.25 * slope.max()) & (np.arange(L) > 0) & (np.arange(L) < L - 1))
    i = int(ok[np.argmin(np.abs(a[ok] - 0.25))])
    want = W.QUARTER + k * W.mpf(2) ** -54
    shift = want - cv.value(i)
    out = _round(y + shift for y in cv.y)
    return out, i, float(W.curve(out, L).value(i) - W.QUARTER)


# ---------------------------------------------------------------- the list
class CaseList:
    """The cases of one config: ``knots`` [N, 2, nk], per case a family, a label, whether a
    near tie is allowed in a decisive family (``tie_ok``), extra judged indices and notes
    (``info``); ``idx`` [N, n_idx]: the judged grid indices per case (padded with 0)."""

    def __init__(self, name: str):
        self.name = name
        self.exp, self.nk, self.L = CONFIGS[name]
        self.cfg = oracle_config(name)
        self.ncurves = 2 if self.exp == 6 else 1
        self.rows: list[dict] = []
        self._pending = None

    def add(self, family, label, kv, tie_ok=False, extra=(), **info):
        """One curve; in experiment 6 two consecutive curves of a family share an env."""
        kv = np.array(kv, np.float64)
        if not tie_ok and (kv[0] in (0.0, 1.0) or kv[-1] in (0.0, 1.0)) and W.curve(kv, self.L).decision_margin() == 0:
            tie_ok, label = True, label + " (an end knot of exactly 0.0 or 1.0 is the grid extreme: on the bar)"
        row = dict(family=family, label=label, kv=kv, tie_ok=bool(tie_ok),
                   extra=tuple(int(i) for i in extra), info=info)
        if self.ncurves == 1:
            self.rows.append(dict(family=family, curves=[row]))
        elif self._pending is not None and self._pending["family"] == family:
            self.rows.append(dict(family=family, curves=[self._pending, row]))
            self._pending = None
        else:
            self.flush()
            self._pending = row

    def flush(self):
        if self._pending is not None:     # an odd curve: its env's second curve is plain
            fill = dict(self._pending, label="filler: " + self._pending["label"], info={},
                        kv=inside(np.linspace(0.2, 0.7, self.nk) ** 2, self.L), tie_ok=False, extra=())
            self.rows.append(dict(family=self._pending["family"], curves=[self._pending, fill]))
            self._pending = None

    def finish(self):
        self.flush()
        self.N = len(self.rows)
        nk, L = self.nk, self.L
        self.knots = np.zeros((self.N, 2, nk), np.float64)
        self.family = np.array([r["family"] for r in self.rows])
        judged = []
        for n, r in enumerate(self.rows):
            for c, cu in enumerate(r["curves"]):
                self.knots[n, c] = cu["kv"]
            if len(r["curves"]) == 1:
                self.knots[n, 1] = self.knots[n, 0][::-1]     # never read (exp 4, 5)
            judged.append(self._judged(r))
        width = max(len(j) for j in judged)
        self.idx = np.zeros((self.N, width), np.int32)
        self.n_idx = np.array([len(j) for j in judged])
        for n, j in enumerate(judged):
            self.idx[n, :len(j)] = j
        return self

    def _judged(self, r) -> list:
        nk, L = self.nk, self.L
        if L <= SMALL_L:
            return list(range(L))
        s = {0, L - 1} | set(range(0, L, 97))
        for j in range(1, nk - 1):
            i = (j * (L - 1)) // (nk - 1)
            s |= {i - 1, i, i + 1, i + 2}
        for cu in r["curves"]:
            _, imn, _, imx = W.curve(cu["kv"], L).extremes()
            for i in (imn, imx) + cu["extra"]:
                s |= set(range(i - 2, i + 3))
        return sorted(i for i in s if 0 <= i < L)

    def curves(self):
        """(case number, curve number, curve dict) of every judged curve."""
        for n, r in enumerate(self.rows):
            for c, cu in enumerate(r["curves"]):
                yield n, c, cu


def _add_random(cl, n, rng):
    for i in range(n):
        cl.add("random", f"random {i}", rng.random_sample(cl.nk))


def _add_edges(cl, rng, ladder):
    """``ladder``: (mode, k) rungs; every rung from its own random base curve."""
    for mode, k in ladder:
        lo, hi = edge_targets(mode, k)
        kv = affine(rng.random_sample(cl.nk), cl.L, lo, hi)
        cv = W.curve(kv, cl.L)
        a, b = cv.margins()
        cl.add("renorm_edge", f"{mode} k={k:+d}", kv, mode=mode, k=k, margin_max=float(a), margin_min=float(b))
    kv = smooth_end_knots(cl.nk)
    cl.add("renorm_edge", "end knots exactly 0.0 and 1.0", kv, tie_ok=True, mode="end", k=0)


def full_ladder():
    """Every rung in every mode, and 2^20 three more times per mode: the decisive share."""
    out = []
    for mode in ("max", "min", "both"):
        out += [(mode, k) for k in K_RUNGS]
        out += [(mode, k) for k in (2 ** 20, -2 ** 20) * 3]
    return out


def _add_shapes(cl, rng, only=None):
    for i, (label, kv, tie_ok) in enumerate(shapes(cl.nk, rng)):
        if only is None or i in only:
            cl.add("shape", label, kv, tie_ok=tie_ok)


def _add_critical(cl, rng, distances=DISTANCES):
    for n, d in enumerate(distances):
        kv, info = critical_case(cl.nk, cl.L, d, rng, want_max=n % 2 == 0)
        cl.add("critical", f"critical point {d:+g} grid steps from sample {info['i0']}", kv,
               extra=(info["i0"],), **info)


def _add_rectifier(cl, rng, rungs):
    for k in rungs:
        kv, i, margin = rectifier_case(rng.random_sample(cl.nk), cl.L, k)
        cl.add("rectifier", f"sample {i} at 0.25 {k:+d} ulp", kv, extra=(i,), index=i, k=k, margin=margin)


_CACHE: dict = {}


def build(name: str) -> CaseList:
    """The case list of config ``name`` (built once per process; treat as read only)."""
    if name in _CACHE:
        return _CACHE[name]
    cl = CaseList(name)
    exp, nk, L = CONFIGS[name]
    rng = np.random.RandomState(20261 + 100 * nk + L % 97 + exp)
    big = 2 ** 20
    if L > SMALL_L and exp == 6 and nk == 8:        # 16 curves
        _add_random(cl, 2, rng)
        _add_edges(cl, rng, [("max", 1), ("min", -big), ("both", big)])
        _add_shapes(cl, rng, only=(13, 14))         # alternating 0/1, 1/0
        _add_critical(cl, rng)
    elif L > SMALL_L and exp == 6:                  # 16 knots: 16 curves
        _add_random(cl, 4, rng)
        _add_edges(cl, rng, [("max", 1), ("max", -big), ("min", 2), ("min", big), ("both", big)])
        _add_shapes(cl, rng, only=(0, 5, 21, 22))
        _add_critical(cl, rng, (0.0, 0.5))
    elif exp == 4:
        _add_random(cl, 3, rng)
        _add_edges(cl, rng, [("max", -1), ("max", big), ("min", 1), ("min", -big), ("both", 8), ("both", -big),
                             ("both", big)])
        _add_shapes(cl, rng, only=(1, 3, 6, 13, 19))
    elif exp == 5:
        _add_random(cl, 2, rng)
        _add_edges(cl, rng, [("max", big), ("min", 1)])
        _add_rectifier(cl, rng, (1, -1, 8, -64) + (big, -big) * 3 + (big,))
    else:
        _add_random(cl, 8 if L <= 120 else 4, rng)
        _add_edges(cl, rng, full_ladder())
        _add_shapes(cl, rng)
        if name == "e6_k8_L37":
            _add_critical(cl, rng)
    _CACHE[name] = cl.finish()
    return _CACHE[name]


# ---------------------------------------------------------------- the step's wind
STEP_L = 120     # 8 knots: 17 steps per interval


def step_knots(nk: int = 8, n: int = 16) -> np.ndarray:
    """Knots [n, 2, nk] of the episodes whose every step is held to the evaluated wind:
    alternating 0/1 and unit spikes (large third-derivative jumps at the knots, so the
    neighbouring piece differs visibly one sample past a knot)."""
    alt = (np.arange(nk) % 2).astype(np.float64)
    pool = [alt, 1 - alt] + [np.eye(nk)[k] for k in range(nk)]
    return np.array([[pool[e % len(pool)], pool[(e + 3) % len(pool)]] for e in range(n)])


def neighbour_piece_wind(kv, top, i: int, L: int):
    """(wind at sample i, wind of the piece before sample i's continued to it): exact, from
    the exact folded pairs. None where sample i lies in the first interval."""
    cv = W.curve(kv, L)
    nk = len(kv)
    j, t = W.knot_coord(i, nk, L)
    if j == 0:
        return None
    pr = cv.pairs(top)
    here = W.piece(pr[j][0], pr[j][1], pr[j + 1][0], pr[j + 1][1], t)
    before = W.piece(pr[j - 1][0], pr[j - 1][1], pr[j][0], pr[j][1], t + 1)
    return here, before


# ---------------------------------------------------------------- the numpy reference
def numpy_reference(cl: CaseList) -> dict:
    """boat_oracle.wind_from_knots at every case's judged indices: what ``measure`` reads
    with ``is_reference``."""
    out = dict(wv=np.zeros(cl.idx.shape), wa=np.zeros(cl.idx.shape),
               unit=np.zeros((cl.N, cl.ncurves) + cl.idx.shape[1:]), renorm=np.zeros((cl.N, cl.ncurves), bool))
    with np.errstate(all="ignore"):
        for n in range(cl.N):
            r = wind_from_knots(cl.cfg, cl.knots[n], cl.idx[n])
            out["wv"][n], out["wa"][n] = r["wv"], r["wa"]
            out["unit"][n], out["renorm"][n] = np.array(r["unit"]), r["renorm"]
    return out


# ---------------------------------------------------------------- measuring a fit
def unit_of(cv, top, branch: bool) -> float:
    """eps x top, over the exact span of a renormalised curve where that is below 1."""
    u = W.mpf(W.EPS) * top
    if branch:
        span = cv.span()
        if span < 1:
            u = u / span
    return float(u)


def kernel_branch(cv, top, pairs) -> bool:
    """The branch stored pairs took: the one whose exact knot values they are nearer to."""
    if cv.span() == 0:
        return False
    err = []
    for b in (False, True):
        ex = cv.pairs(top, b)
        err.append(max(abs(W.mpf(float(p[0])) - e[0]) if np.isfinite(p[0]) else W.mpf("inf")
                       for p, e in zip(pairs, ex)))
    if err[0] == err[1]:
        return cv.renorm()
    return bool(err[1] < err[0])


def measure(cl: CaseList, out: dict, bars: float | None, is_reference: bool = False, tie_bar: float | None = None,
            report: list | None = None) -> tuple[dict, list]:
    """Every judged curve of ``cl`` against the mpmath wind. ``out``: the kernel's ``pairs``
    [N, 2, nk, 2] with ``wv`` and ``wa`` [N, n_idx] (``wind_eval`` at ``cl.idx``), or with
    ``is_reference`` boat_oracle's ``numpy_reference``. Returns (worst, failures):
    ``worst[stage][family]`` the largest error in units (the reference has one stage,
    ``table``; near ties are kept apart as ``<family>:near_tie``), ``failures`` one
    (case, line) per violation of the bar (``bars`` None: none applied) or of a decisive
    decision. ``tie_bar``: the bar that says which decisions are decisive (default
    ``bars``; None and no ``bars``: every nonzero margin is decisive). ``report`` collects
    one dict per near tie: which branch was taken and what the exact decision is."""
    exp, nk, L = cl.exp, cl.nk, cl.L
    stages = ("table",) if is_reference else STAGES
    worst = {s: {} for s in stages}
    fails: list = []
    tb = bars if tie_bar is None else tie_bar
    tie_abs = (tb or 0.0) * W.EPS

    def note(stage, n, cu, fam, e):
        worst[stage][fam] = max(worst[stage].get(fam, 0.0), e)
        limit = tb if is_reference and fam.endswith(NEAR_TIE) and tb else bars   # (the reference's near ties: the kernel's bar)
        if bars is not None and not e <= limit:
            fails.append((n, f"{cl.name}[{n}] {cu['label']}: {stage} off by {e:.4g} units (bar {limit:.4g})"))

    for n, c, cu in cl.curves():
        cv = W.curve(cu["kv"], L)
        top = W.top_of(exp, c, cl.cfg.max_velocity)
        exact_b, margin = cv.renorm(), cv.decision_margin()
        decisive = margin > tie_abs
        pairs = None if is_reference else np.asarray(out["pairs"][n][c], np.float64)
        if not is_reference and not np.isfinite(pairs).all():
            fails.append((n, f"{cl.name}[{n}] {cu['label']}: stored pairs are not finite"))
            continue
        took = bool(out["renorm"][n][c]) if is_reference else kernel_branch(cv, top, pairs)
        fam = cu["family"] + ("" if decisive else NEAR_TIE)
        if not decisive and report is not None:
            report.append(dict(config=cl.name, case=n, curve=c, label=cu["label"], what="renormalise",
                               margin=float(margin), exact=exact_b, took=took))
        if took != exact_b and decisive:
            fails.append((n, f"{cl.name}[{n}] {cu['label']}: renormalised={took}, the exact decision is {exact_b} "
                             f"by a margin of {float(margin):.3g}"))
            continue
        if took and cv.span() == 0:
            fails.append((n, f"{cl.name}[{n}] {cu['label']}: renormalised a constant curve"))
            continue
        unit = unit_of(cv, top, took)
        got_tab = None if exp == 5 else out["wv" if c == 0 else "wa"][n]
        for q in range(int(cl.n_idx[n])):
            i = int(cl.idx[n, q])
            T = W.table_value(cv, i, top, took)
            if is_reference:
                g = out["unit"][n][c][q] if exp == 5 else got_tab[q]
                note("table", n, cu, fam, W.err_units(g, T, unit))
                ref_val = T
            else:
                P = W.stored_value(pairs, i, nk, L)
                note("fit", n, cu, fam, float(abs(P - T) / W.mpf(unit)))
                if exp != 5:
                    note("eval", n, cu, fam, W.err_units(got_tab[q], P, unit))
                ref_val = P
            if exp == 5:      # the rectifier's decision (wind.py:92-99), from the curve it reads
                d = ref_val - W.QUARTER
                want = 0.0 if d <= 0 else 1.0
                wa = float(out["wa"][n][q])
                got = 0.0 if wa == np.pi / 2 else 1.0 if wa == (1.0 * np.pi) + np.pi / 2 else None
                sure = abs(d) > (tb or 0.0) * unit
                if got is None or float(out["wv"][n][q]) != cl.cfg.max_velocity:
                    fails.append((n, f"{cl.name}[{n}] {cu['label']}: exp 5 wind ({out['wv'][n][q]!r}, {wa!r}) "
                                     f"at sample {i} is no rectifier output"))
                elif got != want and sure:
                    fails.append((n, f"{cl.name}[{n}] {cu['label']}: rectifier {got} at sample {i}, the curve is "
                                     f"{float(d):+.3g} from 0.25"))
                if not sure and report is not None:
                    report.append(dict(config=cl.name, case=n, curve=c, label=cu["label"], what="rectifier",
                                       index=i, margin=float(d), exact=want, took=got))
    return worst, fails


def tie_key(t: dict) -> tuple:
    return (t["case"], t["curve"], t["what"], t.get("index"))


def tie_summary(ties: list, other: list | None = None) -> dict:
    """What a profile keeps of ``measure``'s near-tie report: the count per kind, how many
    took the exact branch, and the ones that did not; with ``other`` (another report of
    the same list) how many near ties both hold and how many of those were decided alike."""
    out = {"count": len(ties), "by_kind": {k: sum(t["what"] == k for t in ties) for k in sorted({t["what"] for t in ties})},
           "took_exact": sum(t["took"] == t["exact"] for t in ties),
           "not_exact": [t for t in ties if t["took"] != t["exact"]]}
    if other is not None:
        theirs = {tie_key(t): t["took"] for t in other}
        both = [t for t in ties if tie_key(t) in theirs]
        out["shared_with_numpy"] = len(both)
        out["decided_as_numpy"] = sum(t["took"] == theirs[tie_key(t)] for t in both)
    return out


def knots_digest(cl: CaseList) -> str:
    """sha256 of the list's knots and judged indices: ties a measured profile to its cases."""
    import hashlib
    return hashlib.sha256(cl.knots.tobytes() + cl.idx.tobytes()).hexdigest()


def overall(worst: dict, for_c_ref: bool = False) -> dict:
    """The largest figure per stage over the families; ``for_c_ref`` leaves out the near ties."""
    return {s: max((v for k, v in f.items() if not (for_c_ref and k.endswith(NEAR_TIE))), default=0.0)
            for s, f in worst.items()}


def c_ref_of(cl: CaseList) -> tuple[float, dict]:
    """The reference's worst error over the decisive cases and its worst per family. Which
    cases are decisive depends on the bar, BAR_FACTOR x this figure: iterated from
    "every nonzero margin decides" to the fixed point."""
    out = numpy_reference(cl)
    bar_ = None
    for _ in range(8):
        worst, _ = measure(cl, out, None, is_reference=True, tie_bar=bar_)
        c = overall(worst, for_c_ref=True)["table"]
        if bar_ == BAR_FACTOR * c:
            return c, worst
        bar_ = BAR_FACTOR * c
    raise RuntimeError(f"{cl.name}: the decisive set did not settle (last c_ref {c})")
