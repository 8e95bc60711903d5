"""The mpmath stages of the boat step, the case list's invariants, and a source guard
on the step kernel's hand-written polynomials. No GPU.

* oracle/boat_step_mp.py against ``OracleVecBoat.step`` on every config's case list:
  every stage within the committed ``C_REF``, the exact rules and the classes equal;
* the termination chain against ``np.select``'s priority, all 32 combinations;
* the case list: both placements of every fast-path case, every index inside the wind
  table, no accidental terminations, a padded last wave;
* ``C_REF`` in oracle/boat_step_cases.py equals profiles/r14_boat_step_margins.json;
* the source guard (``test_kernel_polynomials``): the ``sn``, ``cs``, ``ex`` and ``ec``
  literals and the three Cody-Waite constants are read out of
  sac-agent_amd/csrc/sacenv_boat_math.h by regex, the kernel's Horner schemes are
  evaluated operation for operation with a correctly rounded fma (exact mpmath
  product and sum, rounded once), and compared with mpmath's sin / cos / exp.
  Bars: a one-off run of this check on the literals of the commit that introduced
  it measured, in ulps of the exact value,

      sin_taylor  |x| <= 1.25            1.013          (bar 1.1)
      sincos_fast |x| <= 1e5, sin / cos  1.253 / 1.340  (bar 1.45)
      exp_v       [-708, 709]            0.835          (bar 0.95)

  on 3 000 points per range plus the k pi/2 neighbours of the case list; the bars
  are those figures with a margin of about a tenth of an ulp. A coefficient wrong in
  its 10th digit moves sin_taylor by 1e5 ulps or more.
"""
import json
import math
import os
import re

import mpmath
import numpy as np
import pytest

import boat_step_cases as K
import boat_step_mp as M
from boat_oracle import (TERM_FUEL, TERM_GOAL, TERM_NONE, TERM_OOB, TERM_RUDDER, TERM_TIMEOUT)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "sac-agent_amd", "csrc", "sacenv_boat_math.h")

SIN_TAYLOR_BAR, SINCOS_BAR, EXP_BAR = 1.1, 1.45, 0.95


# ---------------------------------------------------------------- stages against the numpy reference
@pytest.fixture(scope="module")
def reference_figures():
    out = {}
    for name in K.CONFIGS:
        cl = K.build(name)
        out[name] = K.measure(cl, K.numpy_step(cl), dict(K.C_REF[name]), obs_f32=False, is_reference=True)
    return out


@pytest.mark.parametrize("name", list(K.CONFIGS))
def test_stages_against_numpy_reference(name, reference_figures):
    """Within c_ref on every family (the ordinary one included), classes and term codes
    equal; the committed c_ref is reached, so it is the reference's error, not a guess."""
    worst, fails = reference_figures[name]
    assert not fails, "\n".join(m for _, m in fails[:10])
    got = K.overall(worst, for_c_ref=True)
    for s in K.STAGES:
        assert got[s] == pytest.approx(K.C_REF[name][s], rel=1e-9), s
    # the ordinary family: a few units, on every stage
    for s in K.STAGES:
        if name != "wide" or s != "reward":
            assert worst[s]["ordinary"] <= 5.0, (s, worst[s]["ordinary"])
    # past |s_r'| = pi the reference's drift - s_r form is measured but not a bar
    if name != "wide":
        assert worst["s_x"]["trig" + K.LARGE_S_R] > 1e6


def test_c_ref_constants_match_the_profile():
    with open(os.path.join(ROOT, "profiles", "r14_boat_step_margins.json")) as f:
        doc = json.load(f)["reference"]
    assert doc["bar_factor"] == K.BAR_FACTOR == 4.0
    assert set(doc["configs"]) == set(K.C_REF) == set(K.CONFIGS)
    for name, c in doc["configs"].items():
        assert c["cases"] == K.build(name).N
        for s in K.STAGES:
            assert c["c_ref"][s] == K.C_REF[name][s], (name, s)
            assert c["bar"][s] == 4.0 * K.C_REF[name][s] == K.bar(name, s)


def test_chain_priority_all_combinations():
    c = K.oracle_config("dt01")
    codes = [TERM_GOAL, TERM_OOB, TERM_FUEL, TERM_TIMEOUT, TERM_RUDDER]
    for bits in range(32):
        for oob_form in ("s_y", "s_x"):
            goal, oob, fuel, tout, rud = [(bits >> k) & 1 for k in (4, 3, 2, 1, 0)]
            if oob_form == "s_x" and (goal or not oob):
                continue
            s_x = c.goal_line + 1 if goal else (-1.0 if oob and oob_form == "s_x" else 10.0)
            s_y = -900.0 if oob and oob_form == "s_y" else 5.0
            conds = [np.array([s_x >= c.goal_line]), np.array([abs(s_y) > 800 or s_x < 0]), np.array([bool(fuel)]),
                     np.array([bool(tout)]), np.array([bool(rud)])]
            want = int(np.select(conds, codes, TERM_NONE)[0])
            got = M.chain(c, s_x, s_y, -1 if fuel else 3, c.t_max if tout else 7.0, -1.2 if rud else 0.3)
            assert got == want, bits
    # truncation only where the chain found nothing; 1..5 overwrite last_term, 0 and 6 keep it
    assert M.episode_end(TERM_NONE, 10, 10, 3) == (6, 1, None, 3)
    assert M.episode_end(TERM_NONE, 9, 10, 3) == (0, 0, None, 3)
    assert M.episode_end(TERM_RUDDER, 10, 10, 1) == (TERM_RUDDER, 1, 3, TERM_RUDDER)
    assert M.episode_end(TERM_TIMEOUT, 1, 0, 0) == (TERM_TIMEOUT, 1, 4, TERM_TIMEOUT)


# ---------------------------------------------------------------- the case list
def _ranges(cl):
    """Per case: are J, rudder', wa and s_r' (numpy reference) inside the fast paths' bounds."""
    a, ref = cl.arrays, K.numpy_step(cl)
    with np.errstate(invalid="ignore"):
        return np.stack([np.abs(K.advance_ratio(cl.cfg, a["v_x"])) <= 1.25, np.abs(ref["rudder"]) <= 1.25,
                         np.abs(a["wa"]) <= 1.0e5, np.abs(ref["s_r"]) <= 1.0e5], axis=1)


@pytest.mark.parametrize("name", ["dt025", "dt01"])
def test_case_list_placements(name):
    cl = K.build(name)
    assert cl.N % 64 != 0                        # the last wave has padding lanes
    inr = _ranges(cl)
    fast_in = [i for i in range(cl.N) if cl.family[i] == "trig" and cl.label[i].endswith("[in]")]
    assert len(fast_in) == cl.n_fast >= 400
    by_kind = {"mixed": {}, "single": {}}
    for i, j, kind in cl.pairs:
        by_kind[kind][i] = j
        for k in K.FIELDS + ("wv", "wa", "action", "index", "last_term"):     # the same case, bit for bit
            assert cl.arrays[k][i].tobytes() == cl.arrays[k][j].tobytes()
    assert sorted(by_kind["mixed"]) == fast_in and len(by_kind["single"]) == 63
    for i in fast_in:                            # a wave of in-range lanes only
        w = slice(i // 64 * 64, i // 64 * 64 + 64)
        assert inr[w].all(), cl.label[i]
    for j in by_kind["mixed"].values():          # its other lanes: out of range for each argument
        w = slice(j // 64 * 64, j // 64 * 64 + 64)
        assert inr[j].all() and (~inr[w]).any(axis=0).all(), cl.label[j]
    waves = {j // 64 for j in by_kind["single"].values()}
    assert len(waves) == 1
    w = waves.pop()
    out = ~inr[w * 64: w * 64 + 64]
    assert out.any(axis=1).sum() == 1 and out.all(axis=1).sum() == 1      # one lane, out for all four
    # the values the issue lists are there, on both sides of each bound
    labels = set(cl.label)
    for arg in ("J", "rudder"):
        for v in (1.25, -1.25, K._nb(1.25, 1), 1.3, 3.0, 100.0, 0.0, -0.0, K.SUB):
            assert any(lab.startswith(f"{arg}={v!r} ") for lab in labels), (arg, v)
    for arg in ("wa", "s_r"):
        for v in K.large_values() + K.half_pi_values() + [1.25, K._nb(1.25, -1)]:
            assert any(lab.startswith(f"{arg}={v!r} ") for lab in labels), (arg, v)


@pytest.mark.parametrize("name", list(K.CONFIGS))
def test_case_list_indices_and_terminations(name):
    cl = K.build(name)
    a, c = cl.arrays, cl.cfg
    assert cl.table.shape == (2, c.L)
    assert (a["index"] >= 0).all() and (a["index"] <= c.L - 1).all()       # no index out of the table
    assert (cl.table[0, a["index"]] == a["wv"]).all() and (cl.table[1, a["index"]] == a["wa"]).all()
    quiet = ~cl.may_end
    assert (a["index"][quiet] + 1 < K.FUEL0).all()
    ref = K.numpy_step(cl)
    assert (ref["term"][quiet] == TERM_NONE).all(), [cl.label[i] for i in np.flatnonzero(quiet & (ref["term"] != 0))][:5]
    assert quiet.sum() >= 32 and {"ordinary"} <= set(cl.family[quiet])
    if name != "wide":
        assert {"ordinary", "cancel", "filler", "trig"} <= set(cl.family[quiet])
        chain = cl.family == "chain"
        # every code, truncation included (t from the index: a timeout lies past fuel0, so the
        # chain answers out_of_fuel first)
        assert set(ref["term"][chain]) == set(range(7)) - ({TERM_TIMEOUT} if K.t_from_index(c.dt) else set())
        # all 32 combinations are listed where the config can form them
        combos = [lab for lab in cl.label if lab.startswith("combo ")]
        assert len(combos) == (40 if not K.t_from_index(c.dt) else 30)
        assert np.isnan(a["action"]).sum() == 2 and np.isinf(a["action"]).sum() == 4


# ---------------------------------------------------------------- the source guard
def _literals():
    with open(HIP) as f:
        src = f.read()
    num = r"[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?"

    def table(name, n):
        m = re.search(r"constexpr double %s\[%d\] = \{([^}]*)\};" % (name, n), src)
        assert m, name
        vals = [float(v) for v in re.findall(num, m.group(1))]
        assert len(vals) == n, name
        return vals
    cw = re.findall(r"rint\(\w+ \* (%s)\);\s*double \w+ = fma\(-\w+, (%s), \w+\);\s*\w+ = fma\(-\w+, (%s), \w+\);"
                    r"\s*\w+ = fma\(-\w+, (%s), \w+\);" % (num, num, num, num), src)
    assert len(cw) == 2 and cw[0] == cw[1], "sincos_fast and trig3 reduce with the same constants"
    bounds = {k: float(re.search(r"constexpr double %s = (%s);" % (k, num), src).group(1))
              for k in ("kSinBound", "kCwBound")}
    return table("sn", 10), table("cs", 7), table("ex", 10), table("ec", 5), [float(v) for v in cw[0]], bounds


def fma(a: float, b: float, c: float) -> float:
    """RN(a b + c): the exact product and sum in mpmath, rounded once."""
    r = float(mpmath.fadd(mpmath.fmul(a, b, exact=True), c, exact=True))
    return r if r != 0.0 else a * b + c      # (mpmath has no -0.0: IEEE's zero-sum sign)


def sin_taylor(x, sn):
    z = x * x
    q = fma(z, sn[0], sn[1])
    for i in range(2, 10):
        q = fma(q, z, sn[i])
    return fma(x * z, q, x)


def sincos_fast(x, sn, cs, cw):
    k = float(round(x * cw[0]))          # rint: ties to even
    r = fma(-k, cw[1], x)
    r = fma(-k, cw[2], r)
    r = fma(-k, cw[3], r)
    z = r * r
    ps = fma(z, sn[2], sn[3])
    for i in range(4, 10):
        ps = fma(ps, z, sn[i])
    pc = fma(z, cs[0], cs[1])
    for i in range(2, 7):
        pc = fma(pc, z, cs[i])
    sr = fma(r * z, ps, r)
    cr = 1.0 - fma(-(z * z), pc, 0.5 * z)
    q = int(k)
    a, b = (cr, sr) if q & 1 else (sr, cr)
    return (-a if q & 2 else a), (-b if (q + 1) & 2 else b)


def exp_v(x, ex, ec):
    n = float(round(x * ec[0]))
    r = fma(ec[1], n, x)
    r = fma(ec[2], n, r)
    q = fma(ex[0], r, ex[1])
    for i in range(2, 10):
        q = fma(r, q, ex[i])
    q = fma(r, q, 1.0)
    q = fma(r, q, 1.0)
    try:
        e = math.ldexp(q, int(n))
    except OverflowError:
        e = math.inf
    e = math.inf if ec[3] < x else e
    return 0.0 if ec[4] > x else e


def _ulps(got: float, exact) -> float:
    return float(abs(M.mpf(got) - exact) / M.mpf(M.ulp(float(exact))))


def test_kernel_polynomials():
    sn, cs, ex, ec, cw, bounds = _literals()
    assert bounds == {"kSinBound": 1.25, "kCwBound": 1.0e5}
    # the series' coefficients are the doubles nearest +-1/n!
    for i, v in enumerate(sn):
        n = 21 - 2 * i
        assert v == float((-1) ** ((n - 1) // 2) / M.mpf(math.factorial(n))), f"sn[{i}]"
    for i, v in enumerate(cs):
        n = 16 - 2 * i
        assert v == float((-1) ** (n // 2) / M.mpf(math.factorial(n))), f"cs[{i}]"
    # 2/pi, and pi/2 in three Cody-Waite terms: each the double nearest what is left
    assert cw[0] == float(2 / M.mp.pi)
    rest = M.mp.pi / 2
    for v in cw[1:]:
        assert v == float(rest)
        rest -= M.mpf(v)
    assert ec[0] == float(1 / M.mp.log(2)) and ec[1] == -float(M.mp.log(2)) and ec[3:] == [1024.0, -1075.0]
    assert ec[2] == float(-M.mp.log(2) - M.mpf(ec[1]))

    rng = np.random.default_rng(7)
    hp = K.half_pi_values()
    # sin_taylor on |x| <= 1.25
    xs = list(rng.uniform(-1.25, 1.25, 3000)) + [1.25, -1.25, K._nb(1.25, -1), 1e-8, 0.5, K.SUB, 1e-300]
    worst = max(_ulps(sin_taylor(float(x), sn), M.mp.sin(M.mpf(float(x)))) for x in xs)
    print(f"sin_taylor worst {worst:.3f} ulp")
    assert worst <= SIN_TAYLOR_BAR
    # (x = -0.0 gives +0.0, fma(-0 z, q < 0, -0) = +0 + -0, where sin(-0.0) is -0.0: equal values)
    assert sin_taylor(0.0, sn) == 0.0 == sin_taylor(-0.0, sn)
    # sincos_fast on |x| <= 1e5: uniform, log-uniform, the k pi/2 neighbours, the bound
    xs = (list(rng.uniform(-1.0e5, 1.0e5, 1500)) + list(10 ** rng.uniform(-3, 5, 1500) * rng.choice([-1, 1], 1500))
          + [x for x in hp if abs(x) <= 1.0e5] + [1.0e5, -1.0e5, K._nb(1.0e5, -1), 0.0, K.SUB, 1.25])
    ws = wc = 0.0
    for x in xs:
        s, co = sincos_fast(float(x), sn, cs, cw)
        es, ecos = M.mp.sin(M.mpf(float(x))), M.mp.cos(M.mpf(float(x)))
        ws, wc = max(ws, _ulps(s, es)), max(wc, _ulps(co, ecos))
        assert (s > 0) == (es > 0) or s == 0.0 == float(es), x        # the quadrant's signs
        assert (co > 0) == (ecos > 0), x
    print(f"sincos_fast worst sin {ws:.3f} cos {wc:.3f} ulp")
    assert ws <= SINCOS_BAR and wc <= SINCOS_BAR
    # exp_v over the reward's exponents and to both range ends
    xs = list(rng.uniform(-8, 2, 1500)) + list(rng.uniform(-745, 709, 1500)) + [0.0, -0.0, 709.78, -745.13, 1.0, -1.0]
    worst = max(_ulps(exp_v(float(x), ex, ec), M.mp.exp(M.mpf(float(x)))) for x in xs if -708 < x)
    print(f"exp_v worst {worst:.3f} ulp")
    assert worst <= EXP_BAR
    assert exp_v(710.0, ex, ec) == math.inf and exp_v(1025.0, ex, ec) == math.inf
    assert exp_v(-746.0, ex, ec) == 0.0 and exp_v(-1076.0, ex, ec) == 0.0 and exp_v(0.0, ex, ec) == 1.0
    for x in xs:
        if x <= -708:        # subnormal results: within one subnormal spacing
            assert abs(M.mpf(exp_v(float(x), ex, ec)) - M.mp.exp(M.mpf(float(x)))) <= M.mpf(K.SUB)
