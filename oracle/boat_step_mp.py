"""The boat step's stages in mpmath -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

``oracle/boat_oracle.py`` restates ``BoatEnv.step`` (boat_env.py:67-115) in
float64 numpy. This module restates the same formulas, stage by stage, in
mpmath at ``PREC`` bits, so one stage of one step can be judged alone: each
stage function takes that stage's float64 inputs (for the GPU tests: the
kernel's own upstream outputs) and returns

* the stage's exact value (an ``mpf``: the formula evaluated on the float64
  inputs and the float64 config values without intermediate rounding), and
* the stage's UNIT (a float): one float64 ulp of the largest-magnitude term
  that enters the stage's final sum.

An error is then ``|got - exact| / unit``; the bars of the tests are multiples
of the numpy reference's own error in that measure (oracle/boat_step_cases.py,
tools/boat_step_margins.py). Nothing ill-conditioned enters: sin(1e5 +- 1 ulp)
is judged at the float64 argument the stage was given.

Non-finite inputs are not evaluated here: a stage's class (NaN, +inf, -inf,
finite) is what IEEE evaluation of the reference formula gives, i.e. what
``OracleVecBoat`` computes (``classify``).
"""
from __future__ import annotations

import math

import mpmath
import numpy as np

from boat_oracle import (TERM_FUEL, TERM_GOAL, TERM_NONE, TERM_OOB, TERM_RUDDER, TERM_TIMEOUT,
                         TERM_TRUNC, OracleConfig)

PREC = 320
mp = mpmath.mp.clone()
mp.prec = PREC
mpf = mp.mpf

NAN, PINF, NINF, FINITE = 0, 1, 2, 3


def classify(x) -> np.ndarray:
    """Class code per element: NAN, PINF, NINF or FINITE."""
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), NAN, np.where(np.isposinf(x), PINF, np.where(np.isneginf(x), NINF, FINITE)))


def ulp(x) -> float:
    """One float64 ulp at |x| (the spacing above |x|; the smallest subnormal at 0)."""
    return float(np.spacing(np.float64(abs(float(x)))))


def ulp32(x) -> float:
    """One float32 ulp at |x| (of the float32 nearest to it)."""
    with np.errstate(over="ignore"):
        f = np.abs(np.float32(float(x)))
    return float(np.spacing(f)) if np.isfinite(f) else float(np.spacing(np.finfo(np.float32).max))


def _sign(x: float) -> int:
    return (x > 0) - (x < 0)


def _m(x) -> "mpf":
    return x if isinstance(x, mp.mpf) else mpf(float(x))


N_RPM = 20  # boat_env.py:178


# ---------------------------------------------------------------- accelerations
def a_x(c: OracleConfig, v_x, v_y, v_r, wv, wa):
    """eom_longitudinal (boat_env.py:213-239) from the state before the step."""
    v_x, v_y, v_r, wv, wa = map(_m, (v_x, v_y, v_r, wv, wa))
    half = mpf(0.5)
    F_R = v_x ** 2 * _m(c.c_r_front) * half * _m(c.rho) * _m(c.boat_area_front)
    J = v_x * (1 - _m(c.wake_friction)) / (N_RPM * _m(c.propeller_diameter))
    F_T = mp.sin(J) * N_RPM ** 2 * _m(c.rho) * _m(c.propeller_diameter) ** 4 * (1 - _m(c.thrust_deduction))
    F_C = v_y * (_m(c.boat_m) + _m(c.boat_m_y)) * v_r
    F_W = wv ** 2 * _sign(wv) * _m(c.c_r_front) * half * _m(c.rho) * _m(c.boat_area_front) * mp.cos(wa)
    mass = _m(c.boat_m) + _m(c.boat_m_x)
    big = max(abs(F_R), abs(F_T), abs(F_C), abs(F_W)) / mass
    return (-F_R + F_T + F_C + F_W) / mass, ulp(big)


def a_y(c: OracleConfig, v_x_new, v_y, v_r, rudder_new, wv, wa):
    """eom_transverse (boat_env.py:241-265): the new v_x and rudder, the old v_y, v_r."""
    v_x, v_y, v_r, rud, wv, wa = map(_m, (v_x_new, v_y, v_r, rudder_new, wv, wa))
    half = mpf(0.5)
    F_R = v_y ** 2 * _m(c.c_r_side) * half * _m(c.rho) * _m(c.boat_area_side) * _sign(v_y)
    F_RU = mp.sin(rud) * (v_x ** 2 * _m(c.c_r_front) * half * _m(c.rho) * _m(c.rudder_area))
    F_C = v_x * (_m(c.boat_m) + _m(c.boat_m_x)) * v_r
    F_W = wv ** 2 * _sign(wv) * _m(c.c_r_side) * half * _m(c.rho) * _m(c.boat_area_side) * mp.sin(wa)
    mass = _m(c.boat_m) + _m(c.boat_m_y)
    big = max(abs(F_R), abs(F_RU), abs(F_C), abs(F_W)) / mass
    return (-F_R + F_RU + F_C + F_W) / mass, ulp(big)


def a_r(c: OracleConfig, v_x_new, v_r, rudder_new):
    """eom_yawning (boat_env.py:267-281): the new v_x and rudder, the old v_r."""
    v_x, v_r, rud = map(_m, (v_x_new, v_r, rudder_new))
    half = mpf(0.5)
    M_hull = (v_r ** 2 * _m(c.c_r_side) * half * _m(c.rho) * _m(c.boat_area_side) * _m(c.boat_l) * 5
              * _sign(v_r))
    M_rud = (v_x ** 2 * _m(c.c_r_side) * half * _m(c.rho) * _m(c.rudder_area) * mp.sin(rud)
             * (_m(c.boat_b) / 2) * _sign(v_x))
    inertia = _m(c.boat_I) + _m(c.boat_Iz)
    big = max(abs(M_hull), abs(M_rud)) / inertia
    return (-M_hull + M_rud) / inertia, ulp(big)


# ---------------------------------------------------------------- integrators
def integrate(a, v, dt, first: bool = False, initial: float = 0.0):
    """One Integrator step (control_blocks.py:16-36): ``a dt + v``, or the block's
    initial value while its counter is 0 (the v_x block starts at 3, :158-159)."""
    if first:
        return mpf(initial), ulp(initial)
    a, v, dt = map(_m, (a, v, dt))
    return a * dt + v, ulp(max(abs(v), abs(a * dt)))


def position(v_x_new, v_y_new, s_r_new, s_x, s_y, dt):
    """get_kinematics (boat_env.py:283-306) -> ((s_x', s_y'), (unit_x, unit_y)).

    The reference's sin(atan2(v_x, v_y) - s_r) hypot(v_x, v_y) equals
    v_x cos s_r - v_y sin s_r exactly (and the cosine v_y cos s_r + v_x sin s_r),
    for v = 0 too (atan2(0, 0) = 0 times v = 0): the form evaluated here."""
    vx, vy, sr, sx, sy, dt = map(_m, (v_x_new, v_y_new, s_r_new, s_x, s_y, dt))
    s, co = mp.sin(sr), mp.cos(sr)
    step = dt * mp.sqrt(vx ** 2 + vy ** 2)
    nx = (vx * co - vy * s) * dt + sx
    ny = (vy * co + vx * s) * dt + sy
    return (nx, ny), (ulp(max(abs(sx), step)), ulp(max(abs(sy), step)))


# ---------------------------------------------------------------- observation
def obs_spans(c: OracleConfig):
    """(lo, hi) of Boat.return_state's 11 entries (boat_env.py:308-326) as the float64
    values the reference forms them from."""
    return [(0.0, float(c.goal_line)), (0.0, 5.0), (0.0, 0.025),
            (-float(c.track_width), float(c.track_width)), (0.0, 2.0), (0.0, 0.37),
            (0.0, 2 * np.pi), (0.0, 8.5e-3), (0.0, 1.4e-5), (-np.pi / 3, np.pi / 3),
            (0.0, float(c.fuel))]


def obs(c: OracleConfig, values):
    """The 11 normalised entries from the 11 float64 values (s_x, v_x, a_x, s_y, v_y,
    a_y, s_r, v_r, a_r, rudder, fuel): (exact [11], unit [11]); the unit of an entry is
    an ulp of max(|v|, |lo|) / (hi - lo), the larger term of its difference."""
    ex, un = [], []
    for v, (lo, hi) in zip(values, obs_spans(c)):
        span = _m(hi) - _m(lo)
        ex.append((_m(v) - _m(lo)) / span)
        un.append(ulp(max(abs(_m(v)), abs(_m(lo))) / span))
    return ex, un


def obs_bar(exact, unit: float, c_bar: float) -> float:
    """The float32 entry's bar: half a float32 ulp plus the float64 stage's bar."""
    return 0.5 * ulp32(exact) + c_bar * unit


# ---------------------------------------------------------------- reward
def f_y(c: OracleConfig, s_y_new):
    """exponential_reward's f_y (reward_functions.py:42-57); unit: an ulp of itself."""
    W, ay = _m(c.track_width), abs(_m(s_y_new))
    f = (ay / W) / (1 + mp.exp((-_m(c.y_a) / _m(c.y_b)) * (ay - W * _m(0.2))))
    return f, ulp(f)


def reward_adds(c: OracleConfig, base, s_x_new, s_r_new, rudder_new) -> np.float64:
    """The float64 adds after ``0 - f_y`` (boat_env.py:84-111), each one IEEE add on the
    float64 ``base``: +1000 at the goal, the rudder penalty, the yaw penalty."""
    r = np.float64(base)
    rud, s_r = np.float64(rudder_new), np.float64(s_r_new)
    if np.float64(s_x_new) >= c.goal_line:
        r = r + 1000
    if rud > np.pi / 4 or rud < -np.pi / 4:
        r = r - np.abs(rud) * 100
    if np.abs(s_r) > np.pi / 2:
        r = r - 1
    return np.float64(r)


def reward_interval(c: OracleConfig, s_x_new, s_y_new, s_r_new, rudder_new, c_bar: float):
    """(lo, hi, exact base, unit): the float64 rewards a step may return when its
    ``0 - f_y`` lies within ``c_bar`` units of the exact one. The adds are monotone
    in the base, so the bounds are the add chain applied to the base's two ends
    (rounded outwards to float64)."""
    f, unit = f_y(c, s_y_new)
    base = -f
    lo = float(mp.mpf(base - c_bar * unit))
    hi = float(mp.mpf(base + c_bar * unit))
    if mpf(lo) > base - c_bar * unit:
        lo = float(np.nextafter(lo, -np.inf))
    if mpf(hi) < base + c_bar * unit:
        hi = float(np.nextafter(hi, np.inf))
    return (reward_adds(c, lo, s_x_new, s_r_new, rudder_new),
            reward_adds(c, hi, s_x_new, s_r_new, rudder_new), base, unit)


# ---------------------------------------------------------------- termination
def chain(c: OracleConfig, s_x_new, s_y_new, fuel_new, t_new, rudder_new) -> int:
    """The termination chain (boat_env.py:84-105) as the if / elif it is written as:
    goal > oob > fuel > timeout > rudder."""
    s_x, s_y, t, rud = (np.float64(v) for v in (s_x_new, s_y_new, t_new, rudder_new))
    oob = c.track_width + c.oob_offset
    if s_x >= c.goal_line:
        return TERM_GOAL
    if np.abs(s_y) > oob or s_x < 0:
        return TERM_OOB
    if int(fuel_new) < 0:
        return TERM_FUEL
    if c.t_max <= t:
        return TERM_TIMEOUT
    if rud > np.pi / 3 or rud < -np.pi / 3:
        return TERM_RUDDER
    return TERM_NONE


def episode_end(term: int, index_new: int, max_episode_steps: int, last_term: int):
    """(term with truncation, done, counter column or None, last_term after the step):
    truncation only where the chain found nothing; codes 1..5 overwrite
    ``info['termination']``, 0 and 6 keep it (MainLoopTerminal)."""
    col = {TERM_GOAL: 0, TERM_OOB: 1, TERM_FUEL: 2, TERM_RUDDER: 3, TERM_TIMEOUT: 4}.get(term)
    if term == TERM_NONE and max_episode_steps > 0 and index_new >= max_episode_steps:
        term = TERM_TRUNC
    lt = term if TERM_GOAL <= term <= TERM_TIMEOUT else last_term
    return term, int(term != TERM_NONE), col, lt


def err_units(got, exact, unit: float) -> float:
    """|got - exact| in units (inf for a non-finite ``got``)."""
    g = float(got)
    if not math.isfinite(g):
        return math.inf
    return float(abs(mpf(g) - exact) / mpf(unit))
