"""The wind fit's oracle, case list and bars, checked without a GPU.

* oracle/wind_fit_mp.py against the numpy reference (scipy's interp1d basis) and against
  the reference's own wind tables (tests/golden/wind_exp*.npz);
* the numpy reference stays within its own C_REF, and the committed C_REF block is the
  one tools/wind_fit_margins.py measured (profiles/wind_fit_margins.json);
* every family of oracle/wind_fit_cases.py holds what it claims;
* the kernel's ten-candidate rule (its Python mirror, oracle/interval_extrema.py) finds
  the exact grid extremes of every ``shape`` and ``critical`` curve;
* the step test of tests/test_wind_fit_mp_gpu.py has the power to see a step that reads
  the neighbouring spline piece at an interval boundary.
"""
import json
import os

import numpy as np
import pytest

import boat_step_cases as SK
import boat_step_mp as SM
import wind_fit_cases as K
import wind_fit_mp as W
from boat_oracle import OracleConfig, OracleVecBoat, spline_basis, wind_from_knots
from conftest import ROOT, golden
from interval_extrema import interval_extrema_py

PROFILE = os.path.join(ROOT, "profiles", "wind_fit_margins.json")


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize("nk,L", [(8, 10000), (8, 20), (8, 5), (4, 400), (5, 120), (10, 120), (16, 37), (16, 10000)])
def test_oracle_agrees_with_the_scipy_basis(nk, L):
    rng = np.random.RandomState(nk * L)
    B = spline_basis(L, nk)
    idx = range(L) if L <= 400 else list(range(0, L, 211)) + [L - 1]
    for _ in range(4):
        kv = rng.random_sample(nk)
        c = B @ kv
        cv = W.curve(kv, L)
        err = max(abs(float(cv.value(i) - W.mpf(float(c[i])))) for i in idx)
        assert err <= 1e-13, err
        mn, imn, mx, imx = cv.extremes()
        assert abs(float(mn) - c.min()) <= 1e-13 and abs(float(mx) - c.max()) <= 1e-13
        assert abs(c[imn] - c.min()) <= 1e-13 and abs(c[imx] - c.max()) <= 1e-13


@pytest.mark.parametrize("name", ["wind_exp4.npz", "wind_exp5.npz", "wind_exp6.npz", "wind_exp6_tmax5.npz"])
def test_oracle_agrees_with_the_reference_tables(name):
    """The full table, renormalised and scaled, against the reference's own (the 1e-12 of
    test_wind_tables_vs_reference); knots re-drawn as Boat.__init__ draws them."""
    z = golden(name)
    exp, L = int(z["experiment"]), int(z["L"])
    maxv = float(z["max_velocity"])
    idx = [int(i) for i in z["idx"]]
    for e in range(0, len(z["seeds"]), 8 if L > 400 else 2):
        rs = np.random.RandomState(int(z["seeds"][e]))
        assert rs.randint(-640, 640) == z["start_y"][e]
        curves = [W.curve(rs.random_sample(8), L) for _ in range(2 if exp == 6 else 1)]
        if exp == 5:
            ang = [float(W.rectifier(curves[0], i)[0]) * np.pi + np.pi / 2 for i in idx]
            sure = np.array([abs(float(W.rectifier(curves[0], i)[1])) > 1e-12 for i in idx])
            assert sure.all()
            np.testing.assert_allclose(ang, z["ang"][e], rtol=0, atol=1e-12)
            np.testing.assert_array_equal(z["vel"][e], maxv)
            continue
        vel = [float(W.table_value(curves[0], i, W.top_of(exp, 0, maxv))) for i in idx]
        np.testing.assert_allclose(vel, z["vel"][e], rtol=0, atol=1e-12)
        if exp == 6:
            ang = [float(W.table_value(curves[1], i, W.top_of(exp, 1, maxv))) for i in idx]
            np.testing.assert_allclose(ang, z["ang"][e], rtol=0, atol=1e-12)


def test_wind_from_knots_is_what_the_oracle_env_computes():
    """boat_oracle.wind_from_knots is OracleVecBoat's drawn wind as a function of the knots."""
    for exp in (4, 5, 6):
        cfg = OracleConfig(experiment=exp, t_max=30.0)
        o = OracleVecBoat(cfg, [3, 4, 5])
        for e in range(3):
            r = wind_from_knots(cfg, o.knots[e])
            assert r["renorm"] == list(o.renorm[e][: len(r["renorm"])])
            for i in (0, 17, 60, cfg.L - 1):
                wv, wa = o.wind(np.full(3, i))
                np.testing.assert_allclose([r["wv"][i], r["wa"][i]], [wv[e], wa[e]], rtol=0, atol=1e-15)


# ---------------------------------------------------------------- the reference and its margins
def test_committed_c_ref_is_the_measured_one():
    with open(PROFILE) as f:
        doc = json.load(f)
    ref = doc["reference"]["configs"]
    assert set(ref) == set(K.CONFIGS) == set(K.C_REF)
    for name in K.CONFIGS:
        assert K.C_REF[name] == ref[name]["c_ref"], name
        assert ref[name]["knots_sha256"] == K.knots_digest(K.build(name)), f"{name}: measured on other cases"
        assert ref[name]["bar"] == K.BAR_FACTOR * K.C_REF[name]
        assert not ref[name]["reference_failures"]
    assert doc["reference"]["bar_factor"] == K.BAR_FACTOR == SK.BAR_FACTOR and doc["reference"]["bits"] == SM.PREC


@pytest.mark.parametrize("name", list(K.CONFIGS))
def test_reference_within_its_own_margin(name):
    """The numpy reference, measured as the kernel is: within C_REF on every decisive case,
    where it also takes the exact branch; the committed C_REF is reached, so it is the
    reference's error, not a guess. Its near ties are held to the kernel's bar."""
    cl = K.build(name)
    out = K.numpy_reference(cl)
    c_ref = K.C_REF[name]
    worst, fails = K.measure(cl, out, c_ref * (1 + 1e-9), is_reference=True, tie_bar=K.bar(name))
    assert not fails, "\n".join(m for _, m in fails[:8])
    assert K.overall(worst, for_c_ref=True)["table"] == pytest.approx(c_ref, rel=1e-9)
    for fam, v in worst["table"].items():
        assert v <= (K.bar(name) if fam.endswith(K.NEAR_TIE) else c_ref * (1 + 1e-9)), (fam, v)


# ---------------------------------------------------------------- the families
def _decisive(cl, cv):
    return cv.decision_margin() > K.bar(cl.name) * W.EPS


def test_configs_and_budget():
    want = {(6, 8, 10000), (4, 8, 10000), (5, 8, 10000), (6, 8, 20), (6, 8, 37), (6, 8, 5), (6, 4, 400),
            (6, 5, 120), (6, 9, 120), (6, 10, 120), (6, 12, 120), (6, 16, 37), (6, 16, 10000)}
    assert set(K.CONFIGS.values()) == want
    for name, (exp, nk, L) in K.CONFIGS.items():
        cl = K.build(name)
        assert cl.cfg.L == L and cl.knots.shape == (cl.N, 2, nk)
        n = sum(1 for _ in cl.curves())
        assert n <= 16 if L == 10000 else 40 <= n <= 400, (name, n)
        assert (cl.idx >= 0).all() and (cl.idx < L).all()
        if L <= K.SMALL_L:
            assert (cl.n_idx == L).all()
        else:       # the extremes +-2, the samples around every knot, both ends, every 97th
            for n_, c, cu in cl.curves():
                got = set(cl.idx[n_, :cl.n_idx[n_]].tolist())
                _, imn, _, imx = W.curve(cu["kv"], L).extremes()
                must = {0, L - 1} | set(range(0, L, 97))
                for i in (imn, imx):
                    must |= {k for k in range(i - 2, i + 3) if 0 <= k < L}
                for j in range(1, nk - 1):
                    i = (j * (L - 1)) // (nk - 1)
                    must |= {i - 1, i, i + 1, i + 2}
                assert must <= got


@pytest.mark.parametrize("name", list(K.CONFIGS))
def test_families_hold_what_they_claim(name):
    cl = K.build(name)
    exp, nk, L = K.CONFIGS[name]
    edge, rect = [], []
    for n, c, cu in cl.curves():
        cv, info, fam = W.curve(cu["kv"], L), cu["info"], cu["family"]
        if fam in ("random", "shape", "critical") and not cu["tie_ok"]:
            assert _decisive(cl, cv), f"{name}[{n}.{c}] {cu['label']}: a near tie ({float(cv.decision_margin()):.3g})"
        if fam == "renorm_edge" and info.get("mode") in ("max", "min", "both"):
            k, mode = info["k"], info["mode"]
            a, b = cv.margins()
            assert float(a) == info["margin_max"] and float(b) == info["margin_min"]     # the stored, measured margins
            if mode in ("max", "both"):     # the rounding of the knots moves the target by an ulp or two
                assert abs(float(a) - k * 2.0 ** -52) <= 4 * 2.0 ** -52, (cu["label"], float(a))
            if mode in ("min", "both"):
                assert abs(float(b) - k * 2.0 ** -53) <= 4 * 2.0 ** -52, (cu["label"], float(b))
            if mode == "max":
                assert float(b) < -0.1
            if mode == "min":
                assert float(a) < -0.1
            edge.append(_decisive(cl, cv))
            if abs(k) == 2 ** 20:
                assert edge[-1] and cv.renorm() == (k > 0)
        if info.get("mode") == "end":
            mn, imn, mx, imx = cv.extremes()
            assert cu["kv"][0] == 0.0 and cu["kv"][-1] == 1.0 and mn == 0 and mx == 1 and imn == 0 and imx == L - 1
            assert not cv.renorm()
        if fam == "critical":
            d = info["dist"]
            assert abs(d - info["target"]) <= 1e-10, (cu["label"], d)
            mn, imn, mx, imx = cv.extremes()
            i_ext, far = (imx, mx - 1) if info["want_max"] else (imn, -mn)
            assert abs(i_ext - (info["i0"] + d)) <= 1.0 and far > 0.25      # the critical point is the grid extreme
        if fam == "rectifier":
            i, k = info["index"], info["k"]
            rect_, d = W.rectifier(cv, i)
            assert float(d) == info["margin"] and not cv.renorm()
            assert abs(float(d) - k * 2.0 ** -54) <= 8 * 2.0 ** -54, (cu["label"], float(d))
            rect.append(abs(float(d)) > K.bar(name) * W.EPS)
            if abs(k) == 2 ** 20:
                assert rect[-1] and rect_ == (1 if k > 0 else 0)
            others = [abs(float(W.rectifier(cv, j)[1])) for j in cl.idx[n, :cl.n_idx[n]] if j != i]
            assert min(others) > 1e-9       # no other judged sample comes near the rectifier's bar
    assert edge and 2 * sum(edge) >= len(edge), (sum(edge), len(edge))
    assert (exp == 5) == bool(rect)
    if rect:
        assert 2 * sum(rect) >= len(rect)
    fams = set(cl.family)
    assert {"random", "renorm_edge"} <= fams and (exp == 5 or "shape" in fams)
    if name in ("e6_k8_L10000", "e6_k8_L37"):
        dists = sorted(cu["info"]["target"] for _, _, cu in cl.curves() if cu["family"] == "critical")
        assert dists == sorted(K.DISTANCES)


def test_shapes_hold_their_degenerate_quadratics():
    """The all-zero curve's float64 m is exactly 0 (qb == 0) and the ramps' is noise or 0
    (|qa| under the degenerate branch's threshold); L = 5 leaves intervals without a sample."""
    from sacenv.config import spline_g
    for nk in (4, 5, 8, 9, 10, 12, 16):
        G = spline_g(nk)
        sh = {label: kv for label, kv, _ in K.shapes(nk, np.random.RandomState(1))}
        zero = next(kv for label, kv in sh.items() if label.startswith("all knots 0.0"))
        assert (G @ zero == 0.0).all()
        ramp = next(kv for label, kv in sh.items() if label.startswith("exact linear ramp up"))
        m = G @ ramp
        assert np.abs(m).max() <= 1e-15 and (np.diff(ramp, 2) == 0).all()
        sym = next(kv for label, kv in sh.items() if label.startswith("mirror-symmetric knots (critical"))
        assert np.array_equal(sym, sym[::-1])
        cv = W.Curve(sym, 121)
        j = (nk - 1) // 2 if nk % 2 else nk // 2 - 1
        want = W.mpf(0) if nk % 2 else W.mpf(0.5)      # on the centre knot, or on the centre interval's midpoint
        roots = W.critical_points(cv, j) + (W.critical_points(cv, j - 1) if nk % 2 else [])
        assert any(abs(r - want) < 1e-60 or abs(r - 1 - want) < 1e-60 for r in roots), (nk, roots)
        cub = next(kv for label, kv in sh.items() if label.startswith("cubic knots with m[1] exactly 0"))
        m = G @ cub
        assert m[1] == 0.0 and m[2] != m[1] and cub[2] - cub[1] - 2 * m[1] - m[2] != 0      # qb == 0, qa, qc != 0
        cand, _ = interval_extrema_py(cub, m, nk, 121, 1)
        i0 = int((1 + 3 ** -0.5) * 120 / (nk - 1))     # the root +sqrt(1/3) (the other lies before the interval)
        assert len(cand) == 6 and {i0, i0 + 1} <= set(cand)
    empty = [j for j in range(7) if not interval_extrema_py(np.zeros(8), np.zeros(8), 8, 5, j)[0]]
    assert len(empty) >= 2
    # subnormal knots: the scaling's exponent passes 1023, the mirror still answers
    tiny = np.eye(8)[3] * 2.0 ** -1060
    assert len(interval_extrema_py(tiny, spline_g(8) @ tiny, 8, 121, 3)[0]) > 2


# ---------------------------------------------------------------- the candidate rule
@pytest.mark.parametrize("name", list(K.CONFIGS))
def test_candidate_rule_on_adversarial_curves(name):
    """The kernel's ten candidates per interval (the float64 mirror) contain the exact grid
    argmin and argmax of every shape and critical curve."""
    from sacenv.config import spline_g
    cl = K.build(name)
    exp, nk, L = K.CONFIGS[name]
    G = spline_g(nk)
    seen = 0
    for n, c, cu in cl.curves():
        if cu["family"] not in ("shape", "critical"):
            continue
        seen += 1
        kv = cu["kv"]
        m = G @ kv
        cands, cover = [], 0
        for j in range(nk - 1):
            cand, rng_ = interval_extrema_py(kv, m, nk, L, j)
            cands += cand
            if rng_:
                cover += rng_[1] - rng_[0] + 1
        assert cover == L
        cv = W.curve(kv, L)
        mn, _, mx, _ = cv.extremes()
        vals = [cv.value(i) for i in set(cands)]
        tol = max(abs(mn), abs(mx)) * W.mpf(2) ** -280    # (a constant curve is constant to the oracle's own rounding)
        assert min(vals) - mn <= tol, f"{name}[{n}.{c}] {cu['label']}: the candidates miss the grid min"
        assert mx - max(vals) <= tol, f"{name}[{n}.{c}] {cu['label']}: the candidates miss the grid max"
    assert seen or exp == 5


# ---------------------------------------------------------------- power of the step test
def test_step_test_sees_a_neighbouring_piece():
    """tests/test_wind_fit_mp_gpu.py::test_step_uses_the_evaluated_wind holds every step's
    a_x to the wind of the step's own sample. Were the step to read the piece before the
    sample's own (a refresh one step late at an interval crossing), the oracle's a_x would
    move by more than that test's bar at a boundary step of every env."""
    knots, L = K.step_knots(), K.STEP_L
    nk = knots.shape[2]
    c = SK.oracle_config("dt025")
    bar = SK.bar("dt025", "a_x")
    step = (nk - 1) / (L - 1)
    jf = lambda i: min(int(i * step), nk - 2)  # noqa: E731  (the kernel's knot_coord)
    boundary = [i for i in range(1, L) if jf(i) != jf(i - 1)]
    assert len(boundary) == nk - 2
    for e in range(len(knots)):
        cfg = OracleConfig(experiment=6, test_mode=1, t_max=L * 0.25, fixed_points=nk)
        table = wind_from_knots(cfg, knots[e])
        o = OracleVecBoat(cfg, [0], wind_table=np.stack([table["wv"], table["wa"]]), start_y=[0])
        seen = 0.0
        for i in range(max(boundary) + 2):
            if i in boundary or i - 1 in boundary:
                v = (o.v_x[0], o.v_y[0], o.v_r[0])
                w = [K.neighbour_piece_wind(knots[e, k], W.top_of(6, k, cfg.max_velocity), i, L) for k in (0, 1)]
                if None not in w:
                    here, u = SM.a_x(c, *v, float(w[0][0]), float(w[1][0]))
                    for wv, wa in ((w[0][1], w[1][0]), (w[0][0], w[1][1])):      # either curve's piece late
                        late, _ = SM.a_x(c, *v, float(wv), float(wa))
                        seen = max(seen, float(abs(late - here) / u))
            o.step(np.zeros(1, np.float32))
        assert seen > bar, f"env {e}: the neighbouring piece moves a_x by {seen:.3g} units (bar {bar:.3g})"
