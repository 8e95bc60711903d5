"""The committed case list of the boat step's per-stage parity tests, its bars, and
the one function that measures a step's outputs against oracle/boat_step_mp.py.
TEST INFRASTRUCTURE, NOT PRODUCT CODE.

One env per case, deterministic, no filter: every listed case is checked.

Configs (``CONFIGS``): the default boat with a shared ``wind_table`` [2, L]
(t_max 2500) and ``boat.fuel = 6000``; dt 0.25 (``t`` derived from the index) and
dt 0.1 (``t`` carried); and a small "wide" one (track_width 1e6, |s_y| up to 1e7,
so the reward's exponent runs past exp's overflow and underflow bounds).
The step reads wind row min(index, L-1), so a case's ``index`` selects its
(wv, wa) pair: cases with the same pair share a row; rows nobody asked for are 0.

Families: ``ordinary`` (random physical states: the baseline of the units),
``trig`` (J, rudder, wa, s_r at the fast-path bounds, the k pi/2 neighbours and
large arguments), ``cancel`` (cancelling kinematics and force sums, zero
velocities, index 0), ``chain`` (the termination chain's combinations and the
edges of its comparisons), ``actions`` (finite extremes and non-finite actions),
``wide`` (the reward's exponent range), ``filler`` (in-range lanes that pad a wave).
With ``t`` derived from the index (dt 0.25) a timeout needs index + 1 >= L > fuel0, so
the chain's combinations with a timeout but fuel left exist only with carried ``t``
(dt 0.1: all of them; 40 cases against 30).

Lane placement: every trig case on the fast path sits once in a wave whose 64
lanes are all in range (section "in"), once in a wave whose other lanes are out of
range for each of J, rudder, wa and s_r ("mixed"), and the first 63 once more in a
wave with exactly one out-of-range lane ("single"); ``pairs`` lists them. A lane's
result depends on its own arguments only, so the placements must agree bit for bit.

Units and bars: a stage's error is measured in the stage's unit (boat_step_mp.py).
``C_REF`` is the numpy reference's (boat_oracle.OracleVecBoat) worst error per config
and stage over the finite cases, written here by tools/boat_step_margins.py; the
kernel's bar is ``BAR_FACTOR x C_REF`` (the multiple the SAC parity tests use over
their reference), never a figure of the kernel's own.
"""
from __future__ import annotations

import math

import numpy as np

import boat_step_mp as M
from boat_oracle import OracleConfig, OracleVecBoat

MAX_EPISODE_STEPS = 5995
FUEL0 = 6000
BAR_FACTOR = 4.0

CONFIGS = {
    "dt025": dict(dt=0.25),
    "dt01": dict(dt=0.1),
    "wide": dict(dt=0.25, track_width=1.0e6),
}

STAGES = ("a_x", "a_y", "a_r", "v_x", "v_y", "v_r", "s_r", "s_x", "s_y", "obs", "reward")

# The numpy reference's worst error per config and stage, in the stage's unit
# (tools/boat_step_margins.py writes this block; tests/test_boat_step_mp_cpu.py
# checks it against profiles/r14_boat_step_margins.json).
# --- C_REF begin
C_REF = {'dt025': {'a_x': 3.2100515291613467,
           'a_y': 2.8158263650165094,
           'a_r': 2.547628543717036,
           'v_x': 1.0,
           'v_y': 1.0,
           'v_r': 1.0,
           's_r': 0.900390625,
           's_x': 1.2973227361101596,
           's_y': 1.8139285501729192,
           'obs': 1.7167201878193032,
           'reward': 2.5246859106856747},
 'dt01': {'a_x': 3.2100515291613467,
          'a_y': 2.8043362671308794,
          'a_r': 2.8005951607021045,
          'v_x': 1.4554099316635465,
          'v_y': 1.246117804851377,
          'v_r': 1.361367164655746,
          's_r': 0.7243784693751518,
          's_x': 1.6975071149669105,
          's_y': 1.7676332720750243,
          'obs': 1.7167201878193032,
          'reward': 2.764037900374542},
 'wide': {'a_x': 2.231620912521815,
          'a_y': 2.5896607365572697,
          'a_r': 2.547628543717036,
          'v_x': 0.4755859375,
          'v_y': 0.484375,
          'v_r': 0.5,
          's_r': 0.37890625,
          's_x': 0.4964405786636792,
          's_y': 0.49007611508634513,
          'obs': 0.77952,
          'reward': 973.3631629296602}}
# --- C_REF end


def bar(config: str, stage: str) -> float:
    return BAR_FACTOR * C_REF[config][stage]


def oracle_config(name: str) -> OracleConfig:
    return OracleConfig(experiment=6, fuel=FUEL0, t_max=2500, **CONFIGS[name])


def env_config(name: str) -> dict:
    """The same config in the reference's YAML layout (sacenv.BoatConfig.from_any)."""
    c = oracle_config(name)
    return {"base_settings": {"experiment": c.experiment, "test_mode": 0, "dt": c.dt, "t_max": c.t_max},
            "boat_env": {"track_width": c.track_width, "goal_line": c.goal_line},
            "boat": {"fuel": c.fuel}}


def t_from_index(dt: float) -> bool:
    """The step's rule (sacenv.config.t_from_index): dt with at most 22 significand bits."""
    return int(np.array([dt], np.float64).view(np.uint64)[0]) & ((1 << 30) - 1) == 0


# ---------------------------------------------------------------- probe values
def _nb(x, k=1):
    """x moved k ulps away from zero (k < 0: towards zero)."""
    x = np.float64(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.copysign(np.inf, x) if k > 0 else np.float64(0.0))
    return float(x)


SUB = 5e-324
K_SPREAD = (100, 1000, 10000, 31830, 63660, 63661, 63662)


def half_pi_values():
    """The doubles nearest k pi/2 and their two neighbours: k = 1..64 and a spread of k
    up to 63 661 (and 63 662, the first past 1e5); every third k negated."""
    out = []
    for k in list(range(1, 65)) + list(K_SPREAD):
        x = float(M.mp.mpf(k) * M.mp.pi / 2)
        s = -1.0 if k % 3 == 0 else 1.0
        out += [s * _nb(x, -1), s * x, s * _nb(x, 1)]
    return out


def small_values():
    """0, -0.0, the smallest subnormal, +-1.25 and their neighbours, 1.3, 3, 100."""
    return [0.0, -0.0, SUB, 1.25, -1.25, _nb(1.25, -1), _nb(1.25, 1), _nb(-1.25, -1), _nb(-1.25, 1),
            1.3, 3.0, 100.0]


def large_values():
    """+-1e5, one ulp in and out, 1e5 + 1, 1e9, 1e13, 1e22."""
    return [1.0e5, -1.0e5, _nb(1e5, -1), _nb(1e5, 1), _nb(-1e5, -1), _nb(-1e5, 1), 1.0e5 + 1, 1.0e9,
            1.0e13, 1.0e22]


def advance_ratio(c: OracleConfig, v_x) -> np.float64:
    """J as boat_env.py:221-224 forms it in float64."""
    return (np.float64(v_x) * (1 - c.wake_friction)) / (M.N_RPM * c.propeller_diameter)


def vx_for_J(c: OracleConfig, x: float) -> float:
    """The v_x whose advance ratio is x, or where no double gives x exactly, the one
    whose J is nearest x without passing it (away from zero)."""
    if x == 0.0 or not np.isfinite(x):
        return x
    v0 = np.float64(x) * (M.N_RPM * c.propeller_diameter) / (1 - c.wake_friction)
    best = None
    for side in (1.0, -1.0):
        v = v0
        for _ in range(8):
            j = advance_ratio(c, v)
            if j == x:
                return float(v)
            if abs(j) <= abs(x) and (best is None or abs(j) > abs(advance_ratio(c, best))):
                best = v
            v = np.nextafter(v, np.copysign(np.inf, v0) * side)
    assert best is not None
    return float(best)


# ---------------------------------------------------------------- the list
FIELDS = ("s_x", "s_y", "s_r", "v_x", "v_y", "v_r", "rudder", "ep_reward", "t")
BASE = dict(s_x=100.0, s_y=10.0, s_r=0.4, v_x=2.0, v_y=0.3, v_r=0.002, rudder=0.1, ep_reward=-3.5,
            action=0.0, wv=0.3, wa=1.0, last_term=0, index=None)
ROW0 = (0.37, 2.1)   # wind row 0: the index == 0 cases' wind


class CaseList:
    """The cases of one config as arrays [N] (``arrays``), each with a family, a label
    and whether it may end its episode; ``pairs``: (i, j, kind) placements that must
    agree bit for bit; ``table``: the shared wind table [2, L]."""

    def __init__(self, name: str):
        self.name = name
        self.cfg = oracle_config(name)
        self.rows: list[dict] = []
        self.pairs: list[tuple[int, int, str]] = []
        self._wind_index: dict = {self._key(ROW0): 0}
        self._explicit: dict = {}

    @staticmethod
    def _key(wind):   # by bits: -0.0 and 0.0 are different rows
        return (np.float64(wind[0]).tobytes(), np.float64(wind[1]).tobytes())

    def add(self, family, label, may_end=False, **kw) -> int:
        r = dict(BASE)
        r.update(kw)
        r.update(family=family, label=label, may_end=bool(may_end))
        wind = (float(r["wv"]), float(r["wa"]))
        if r["index"] is None:
            r["index"] = self._wind_index.setdefault(self._key(wind), len(self._wind_index))
        else:
            want = ROW0 if r["index"] == 0 else (0.0, 0.0)
            assert wind == want, "a case with a written index reads that row's wind"
            r["wv"], r["wa"] = want
            self._explicit[int(r["index"])] = want
        self.rows.append(r)
        return len(self.rows) - 1

    def pad_wave(self):
        while len(self.rows) % 64:
            self.add("filler", "in-range pad")

    def finish(self):
        if len(self.rows) % 64 == 0:     # the last wave keeps padding lanes
            self.add("filler", "odd one")
        c, L = self.cfg, self.cfg.L
        n_dyn = len(self._wind_index)
        assert n_dyn + 1 < min([k for k in self._explicit if k] + [L, MAX_EPISODE_STEPS - 8])
        self.table = np.zeros((2, L), np.float64)
        self.table[:, 0] = ROW0
        for r in self.rows:
            i = min(int(r["index"]), L - 1)
            if i:
                assert tuple(self.table[:, i]) in ((0.0, 0.0), (r["wv"], r["wa"]))
                self.table[:, i] = (r["wv"], r["wa"])
        for r in self.rows:
            if "t" not in r:
                r["t"] = float(np.float64(r["index"]) * c.dt)
        a = self.arrays = {}
        for k in FIELDS + ("wv", "wa"):
            a[k] = np.array([r[k] for r in self.rows], np.float64)
        a["action"] = np.array([r["action"] for r in self.rows], np.float32)
        a["index"] = np.array([r["index"] for r in self.rows], np.int32)
        a["last_term"] = np.array([r["last_term"] for r in self.rows], np.int32)
        self.family = np.array([r["family"] for r in self.rows])
        self.label = [r["label"] for r in self.rows]
        self.may_end = np.array([r["may_end"] for r in self.rows])
        self.N = len(self.rows)
        return self


def _trig_rows(c: OracleConfig):
    """(fast, slow): the trig family's cases as (arg, label, state) by path; slow per arg."""
    small, large, hp = small_values(), large_values(), half_pi_values()
    fast, slow = [], {"J": [], "rudder": [], "wa": [], "s_r": []}
    for arg in ("J", "rudder", "wa", "s_r"):
        values = small + hp + (large if arg in ("wa", "s_r") else [])
        bound = 1.25 if arg in ("J", "rudder") else 1.0e5
        for x in values:
            if arg == "J":
                v = vx_for_J(c, x)
                st, x_eff = dict(v_x=v), float(advance_ratio(c, v))
            elif arg == "rudder":
                st, x_eff = dict(rudder=x), x
            elif arg == "wa":
                st, x_eff = dict(wa=x, wv=0.45, v_x=0.0, v_r=0.0), x
            else:
                st, x_eff = dict(s_r=x, v_r=0.0, rudder=0.0, v_x=2.1, v_y=0.4, s_x=1.0, s_y=0.25), x
            item = (arg, f"{arg}={x_eff!r}", st)
            if abs(x_eff) <= bound:
                fast.append(item)
            else:
                slow[arg].append(item)
    return fast, slow


def _add_trig(cl: CaseList):
    fast, slow = _trig_rows(cl.cfg)
    add = lambda it, where: cl.add("trig", f"{it[1]} [{where}]", may_end=it[0] in ("J", "rudder"), **it[2])  # noqa: E731
    first = [add(it, "in") for it in fast]            # waves with every lane in range
    cl.pad_wave()
    args = ("J", "rudder", "wa", "s_r")
    turn = {a: 0 for a in args}
    k = 0
    while k < len(fast):                              # 32 fast lanes + 8 slow lanes per argument
        for lane in range(64):
            if lane % 2 == 0 and k < len(fast):
                cl.pairs.append((first[k], add(fast[k], "mixed"), "mixed"))
                k += 1
            else:
                a = args[(lane // 2) % 4]
                add(slow[a][turn[a] % len(slow[a])], "mixed")
                turn[a] += 1
    cl.pad_wave()
    for k in range(63):                               # exactly one out-of-range lane
        cl.pairs.append((first[k], add(fast[k], "single"), "single"))
    cl.add("trig", "J=3, rudder=3, wa=1e9, s_r=1e9 [single]", may_end=True,
           v_x=vx_for_J(cl.cfg, 3.0), rudder=3.0, wa=1.0e9, s_r=1.0e9)
    for a in args:                                    # every slow case, once more, in order
        for it in slow[a]:
            add(it, "slow")
    cl.pad_wave()
    return len(fast)


def _add_ordinary(cl: CaseList, n: int, rng):
    c = cl.cfg
    for i in range(n):
        cl.add("ordinary", f"random {i}",
               s_x=rng.uniform(5, 3800), s_y=rng.uniform(-0.85, 0.85) * c.track_width,
               s_r=rng.uniform(-1.5, 1.5), v_x=rng.uniform(0, 6), v_y=rng.uniform(-1, 1),
               v_r=rng.uniform(-0.01, 0.01), rudder=rng.uniform(-0.9, 0.9), action=rng.uniform(-1, 1),
               ep_reward=rng.uniform(-400, 0), wv=rng.uniform(0, 0.5), wa=rng.uniform(0, 2 * np.pi),
               last_term=int(rng.integers(0, 6)))


def _add_cancel(cl: CaseList, rng):
    c = cl.cfg
    # v_x' cos s_r ~ v_y' sin s_r (the s_x increment cancels) and the mirror: s_r from the
    # numpy reference's new velocities; rudder 0 and v_r 0 keep s_r' = s_r
    for i in range(8):
        vx, vy, wv, wa = rng.uniform(0.5, 5), rng.uniform(-1, 1), rng.uniform(0, 0.5), rng.uniform(0, 6)
        step = OracleVecBoat(c, [0], wind_table=np.array([[wv] * c.L, [wa] * c.L]), start_y=[0])
        step.v_x[:], step.v_y[:], step.index[:] = vx, vy, 1
        out = step.step(np.zeros(1, np.float32))["state"]
        drift = float(np.arctan2(out["v_x"][0], out["v_y"][0]))
        for lab, s_r in (("s_x increment cancels", drift), ("s_y increment cancels", drift - np.pi / 2)):
            for d in (-1, 0, 1):
                cl.add("cancel", f"{lab} {i} ({d:+d} ulp)", s_r=_nb(s_r, d) if d else s_r, v_x=vx, v_y=vy,
                       v_r=0.0, rudder=0.0, wv=wv, wa=wa, s_x=1000.0, s_y=0.0)
    # force sums that nearly cancel. a_x: F_R = F_T at v_x ~ 3.16 (bisection on the float64 formula)
    f = lambda v: (-(np.square(v) * c.c_r_front * 0.5 * c.rho * c.boat_area_front)  # noqa: E731
                   + np.sin(advance_ratio(c, v)) * 400 * c.rho * (1 - c.thrust_deduction))
    lo, hi = np.float64(2.0), np.float64(4.0)
    while np.nextafter(lo, hi) < hi:
        mid = lo + (hi - lo) / 2
        lo, hi = (mid, hi) if f(mid) > 0 else (lo, mid)
    for d in (-2, -1, 0, 1, 2):
        cl.add("cancel", f"F_R = F_T ({d:+d} ulp)", v_x=_nb(lo, d) if d else float(lo), v_y=0.0, v_r=0.0, wv=0.0, wa=0.0)
    # a_y: the hull's drag against the wind, v_y = wv at sin(wa) ~ 1; rudder and v_r 0
    for wv in (0.45, 0.3):
        for wa in (float(np.pi / 2), _nb(np.pi / 2, 1), 1.5):
            cl.add("cancel", f"F_R = F_W side wv={wv} wa={wa!r}", v_y=wv, wv=wv, wa=wa, v_r=0.0, rudder=0.0)
    # a_x: the wind against the hull's drag, v_x^2 = wv^2 cos(wa) ~ wv^2 at wa = 0; F_T stays
    cl.add("cancel", "F_C = -F_W front", v_x=0.0, v_y=0.45 ** 2 * 3.1 / 700 / 0.002, v_r=-0.002, wv=0.45, wa=0.0)
    # a_r: hull moment against rudder moment
    for rud in (0.3, -0.6):
        vr = 2.0 * math.sqrt(30 * math.sin(abs(rud)) / 6750) * (1 if rud > 0 else -1)
        for d in (-1, 0, 1):
            cl.add("cancel", f"M_hull = M_rud rudder={rud} ({d:+d} ulp)", v_r=_nb(vr, d) if d else vr, rudder=rud)
    # zero velocities, with and without wind
    cl.add("cancel", "v = 0, no wind", v_x=0.0, v_y=0.0, v_r=0.0, wv=0.0, wa=0.0)
    cl.add("cancel", "v = 0, wind", v_x=0.0, v_y=0.0, v_r=0.0, wv=0.5, wa=4.0)
    cl.add("cancel", "v = -0.0, wind", v_x=-0.0, v_y=-0.0, v_r=-0.0, wv=0.5, wa=4.0)
    # index 0: the integrators hand out their initial values (3, 0, 0)
    for i in range(6):
        cl.add("cancel", f"index 0 ({i})", index=0, wv=ROW0[0], wa=ROW0[1], v_x=rng.uniform(0, 6),
               v_y=rng.uniform(-1, 1), v_r=rng.uniform(-0.01, 0.01), rudder=rng.uniform(-0.9, 0.9),
               action=rng.uniform(-1, 1), s_r=rng.uniform(-1.5, 1.5))


def _add_chain(cl: CaseList, rng):
    """Zero velocities, zero wind, action 0: positions do not move, so the written
    s_x, s_y, index, t and rudder are the values the chain compares."""
    c = cl.cfg
    carried = not t_from_index(c.dt)
    L, oobl = c.L, c.track_width + c.oob_offset
    still = dict(v_x=0.0, v_y=0.0, v_r=0.0, s_r=0.0, wv=0.0, wa=0.0, action=0.0, rudder=0.0)
    free = [20]

    def idx():   # a free index below the fuel and truncation marks, its wind row 0
        free[0] += 1
        return 5700 + free[0]

    def case(label, *, index=None, **kw):
        st = dict(still)
        st.update(kw)
        st.setdefault("ep_reward", float(rng.uniform(-400, 0)))
        st.setdefault("last_term", int(rng.integers(0, 6)))
        cl.add("chain", label, may_end=True, index=idx() if index is None else index, **st)

    # all 32 combinations; oob in both forms (s_x < 0 excludes the goal)
    for bits in range(32):
        goal, oob, fuel, tout, rud = (bits >> 4) & 1, (bits >> 3) & 1, (bits >> 2) & 1, (bits >> 1) & 1, bits & 1
        for form in (("s_y", "s_x") if oob else ("",)):
            if form == "s_x" and goal:
                continue
            st = dict(s_x=c.goal_line + 50.0 if goal else 100.0, s_y=30.0, rudder=1.1 if rud else 0.2)
            if form == "s_y":
                st["s_y"] = -(oobl + 100.0) if bits & 1 else oobl + 100.0
            if form == "s_x":
                st["s_x"] = -5.0
            if tout and not carried and not fuel:
                continue   # t = (index + 1) dt >= t_max needs index + 1 >= L > fuel0: only with fuel < 0
            if tout:
                index = L - 1 if not carried else (FUEL0 + 7 if fuel else idx())
                if carried:
                    st["t"] = c.t_max + 3.0
            else:
                index = FUEL0 + 7 if fuel else idx()
            case(f"combo goal={goal} oob={form or 0} fuel={fuel} timeout={tout} rudder={rud}", index=index, **st)
    # truncation, alone and with a real termination in the same step; fuel exactly 0
    M_ = MAX_EPISODE_STEPS
    case("one step before truncation", index=M_ - 2)
    case("truncation", index=M_ - 1)
    case("truncation with rudder broken", index=M_ - 1, rudder=1.2)
    case("truncation with goal", index=M_ - 1, s_x=c.goal_line + 1.0)
    case("index + 1 = fuel0 - 1", index=FUEL0 - 2)
    case("index + 1 = fuel0 (fuel 0: not out of fuel; truncated)", index=FUEL0 - 1)
    case("index + 1 = fuel0 + 1 (fuel -1)", index=FUEL0)
    # every comparison at equality and one ulp either side
    for d in (-1, 0, 1):
        tag = f"({d:+d} ulp)"
        case(f"s_x' at goal_line {tag}", s_x=_nb(c.goal_line, d) if d else c.goal_line)
        for s in (1.0, -1.0):
            case(f"s_y' at {s:+.0f} oob_limit {tag}", s_y=s * (_nb(oobl, d) if d else oobl))
            for name, v in (("pi/3", np.pi / 3), ("pi/4", np.pi / 4)):
                case(f"rudder at {s:+.0f} {name} {tag}", rudder=s * (_nb(v, d) if d else float(v)))
            case(f"s_r' at {s:+.0f} pi/2 {tag}", s_r=s * (_nb(np.pi / 2, d) if d else float(np.pi / 2)))
    case("s_x' = -0.0", s_x=-0.0)
    case("s_x' = -5e-324", s_x=-SUB)
    case("s_x' = 0.0", s_x=0.0)
    if carried:    # t + dt at t_max: the written t whose sum is t_max, and its neighbours
        t0 = np.float64(c.t_max) - np.float64(c.dt)
        cands = [float(t0)]
        for k in range(1, 4):
            cands += [_nb(t0, k), _nb(t0, -k)]
        for t in sorted(cands):
            s = np.float64(t) + np.float64(c.dt)
            case(f"t + dt = t_max {int((s - c.t_max) / np.spacing(np.float64(c.t_max))):+d} ulp (t={t!r})", t=t)
    else:          # (index + 1) dt at t_max: past fuel0, so the chain answers out_of_fuel
        for k in (L - 3, L - 2, L - 1):
            case(f"(index + 1) dt at t_max: index + 1 = {k + 1}", index=k)


ACTIONS = (1.0, -1.0, 10.0, -10.0, float(np.finfo(np.float32).max), -float(np.finfo(np.float32).max),
           0.0, -0.0, float("nan"), float("inf"), float("-inf"))


def _add_actions(cl: CaseList):
    for a in ACTIONS:
        for rud in (0.2, -0.0):
            cl.add("actions", f"action={a!r} rudder={rud!r}", may_end=True, action=a, rudder=rud)


def _add_wide(cl: CaseList, rng):
    c = cl.cfg
    k = 0.03 / 3.4
    centre = c.track_width * 0.2
    marks = [0.0, SUB, 1.0, 1.0e3, centre - 709.0 / k, centre - 709.78 / k, centre - 710.0 / k, centre - 744.0 / k,
             centre - 1024.0 / k, centre - 1.0, centre, centre + 1.0, centre + 36.0 / k, centre + 709.78 / k,
             centre + 745.13 / k, centre + 746.0 / k, centre + 1075.0 / k, centre + 1076.0 / k,
             c.track_width, _nb(c.track_width, 1), 1.0e7]
    still = dict(v_x=0.0, v_y=0.0, v_r=0.0, s_r=0.0, wv=0.0, wa=0.0, action=0.0, rudder=0.0)
    for y in marks:
        for s in (1.0, -1.0):
            cl.add("wide", f"s_y={s * y!r}", may_end=True, s_y=s * y, **still)
    for i in range(40):
        y = float(10 ** rng.uniform(0, 7)) * (1 if i % 2 else -1)
        cl.add("wide", f"s_y={y!r} moving", may_end=True, s_y=y)


_CACHE: dict = {}


def build(name: str) -> CaseList:
    """The case list of config ``name`` (built once per process; treat as read only)."""
    if name in _CACHE:
        return _CACHE[name]
    cl = CaseList(name)
    rng = np.random.default_rng(20251)
    if name == "wide":
        _add_ordinary(cl, 32, rng)
        _add_wide(cl, rng)
    else:
        cl.n_fast = _add_trig(cl)
        _add_ordinary(cl, 256, rng)
        _add_cancel(cl, rng)
        _add_chain(cl, rng)
        _add_actions(cl)
    _CACHE[name] = cl.finish()
    return _CACHE[name]


# ---------------------------------------------------------------- the numpy reference
OUT_F64 = ("a_x", "a_y", "a_r", "v_x", "v_y", "v_r", "s_r", "s_x", "s_y", "rudder", "t", "reward", "ep_reward")


def numpy_step(cl: CaseList) -> dict:
    """One ``OracleVecBoat.step`` from the written states: the outputs ``measure`` reads."""
    c, a = cl.cfg, cl.arrays
    sel = slice(None)
    n = cl.N
    o = OracleVecBoat(c, np.zeros(n, np.uint64), max_episode_steps=MAX_EPISODE_STEPS,
                      wind_table=cl.table, start_y=np.zeros(n, np.int64))
    for k in FIELDS:
        getattr(o, k)[:] = a[k][sel]
    o.index[:] = a["index"][sel]
    o.fuel[:] = c.fuel - o.index
    with np.errstate(all="ignore"):
        r = o.step(a["action"][sel])
    st = r["state"]
    out = {k: st[k] for k in ("a_x", "a_y", "a_r", "v_x", "v_y", "v_r", "s_r", "s_x", "s_y", "t")}
    out["rudder"], out["index"] = st["rudder_angle"], st["index"].astype(np.int64)
    out["obs"], out["reward"], out["ep_reward"] = r["obs"], r["reward"], r["ep_reward"]
    out["term"], out["done"] = r["term"].astype(np.int64), r["done"].astype(np.int64)
    lt0 = a["last_term"][sel].astype(np.int64)
    out["last_term"] = np.where((out["term"] >= 1) & (out["term"] <= 5), out["term"], lt0)
    out["counters"] = o.counters.T.copy()
    return out


# ---------------------------------------------------------------- measuring a step
# The reference forms sin(atan2(v_x, v_y) - s_r): its subtraction rounds at an ulp of
# |s_r|, so past |s_r'| = pi (drift's own range) its error measures the conditioning of
# that form (1e15 units at s_r = 1e22), not arithmetic. Those cases are measured and
# reported under "<family>:large_s_r" but stay out of C_REF: the kernel is held, at
# any s_r', to the bar the reference earns where its form is well conditioned.
LARGE_S_R = ":large_s_r"
TINY = float(np.finfo(np.float64).tiny)

def measure(cl: CaseList, out: dict, bars: dict | None, obs_f32: bool, is_reference: bool = False) -> tuple[dict, list]:
    """Every case of ``cl`` against the mpmath stages, each stage from ``out``'s own
    upstream values. Returns (worst, failures): ``worst[stage][family]`` the largest
    error in units over the finite cases (obs: the float64 part for a float64 obs,
    else the error over the entry's bar), ``failures`` one line per violation of a
    bar (``bars`` None: none are applied), of an exact rule, or of a class.
    ``is_reference``: ``out`` is the numpy reference's own step, which is not held to a
    bar where its form is ill conditioned (LARGE_S_R)."""
    c, a = cl.cfg, cl.arrays
    dt = c.dt
    carried = not t_from_index(dt)
    worst = {s: {} for s in STAGES}
    fails: list[str] = []
    ref = numpy_step(cl)

    def note(stage, i, e, tag=""):
        fam = cl.family[i] + tag
        worst[stage][fam] = max(worst[stage].get(fam, 0.0), e)
        if bars is not None and not e <= bars[stage] and not (is_reference and tag):
            fails.append((int(i), f"{cl.name}[{i}] {cl.label[i]}: {stage} off by {e:.3g} units (bar {bars[stage]:.3g})"))

    def exact(name, i, got, want):
        if not (got == want or (got != got and want != want)):
            fails.append((int(i), f"{cl.name}[{i}] {cl.label[i]}: {name} is {got!r}, the reference rule gives {want!r}"))

    g = {k: np.asarray(out[k], np.float64) for k in OUT_F64}
    finite_in = np.isfinite(a["action"].astype(np.float64))
    for k in OUT_F64 + ("obs",):     # the class of every output is the reference's
        bad = np.flatnonzero(~(M.classify(out[k]) == M.classify(ref[k])).reshape(cl.N, -1).all(axis=1))
        for i in bad:
            fails.append((int(i), f"{cl.name}[{i}] {cl.label[i]}: class of {k} {np.asarray(out[k])[i]!r} "
                         f"differs from the reference's {np.asarray(ref[k])[i]!r}"))
    for i in range(cl.N):
        if not finite_in[i]:
            exact("term", i, int(out["term"][i]), int(ref["term"][i]))
            continue
        first = int(a["index"][i]) == 0
        wv, wa = a["wv"][i], a["wa"][i]
        # rudder and t: one IEEE operation each on float64 inputs: the same double
        rud = np.float64(a["rudder"][i]) + np.float64(a["action"][i]) / 10
        exact("rudder", i, g["rudder"][i], rud)
        t_new = np.float64(a["index"][i] + 1) * dt if not carried else np.float64(a["t"][i]) + dt
        exact("t", i, g["t"][i], t_new)
        exact("index", i, int(out["index"][i]), int(a["index"][i]) + 1)
        ex, u = M.a_x(c, a["v_x"][i], a["v_y"][i], a["v_r"][i], wv, wa)
        note("a_x", i, M.err_units(g["a_x"][i], ex, u))
        ex, u = M.integrate(g["a_x"][i], a["v_x"][i], dt, first, 3.0)
        note("v_x", i, M.err_units(g["v_x"][i], ex, u))
        ex, u = M.a_y(c, g["v_x"][i], a["v_y"][i], a["v_r"][i], g["rudder"][i], wv, wa)
        note("a_y", i, M.err_units(g["a_y"][i], ex, u))
        ex, u = M.integrate(g["a_y"][i], a["v_y"][i], dt, first)
        note("v_y", i, M.err_units(g["v_y"][i], ex, u))
        ex, u = M.a_r(c, g["v_x"][i], a["v_r"][i], g["rudder"][i])
        note("a_r", i, M.err_units(g["a_r"][i], ex, u))
        ex, u = M.integrate(g["a_r"][i], a["v_r"][i], dt, first)
        note("v_r", i, M.err_units(g["v_r"][i], ex, u))
        ex, u = M.integrate(g["v_r"][i], a["s_r"][i], dt)
        note("s_r", i, M.err_units(g["s_r"][i], ex, u))
        (ex_x, ex_y), (ux, uy) = M.position(g["v_x"][i], g["v_y"][i], g["s_r"][i], a["s_x"][i], a["s_y"][i], dt)
        far = LARGE_S_R if abs(g["s_r"][i]) > np.pi else ""
        note("s_x", i, M.err_units(g["s_x"][i], ex_x, ux), far)
        note("s_y", i, M.err_units(g["s_y"][i], ex_y, uy), far)
        fuel = c.fuel - (int(a["index"][i]) + 1)
        vals = [g[k][i] for k in ("s_x", "v_x", "a_x", "s_y", "v_y", "a_y", "s_r", "v_r", "a_r", "rudder")] + [fuel]
        exs, uns = M.obs(c, vals)
        for j in range(11):
            got = float(out["obs"][i][j])
            if obs_f32:
                b = M.obs_bar(exs[j], uns[j], bars["obs"] if bars else 0.0)
                e = float(abs(M.mpf(got) - exs[j]) / M.mpf(b)) if math.isfinite(got) else math.inf
                fam = cl.family[i]
                worst["obs"][fam] = max(worst["obs"].get(fam, 0.0), e)
                if bars is not None and not e <= 1.0:
                    fails.append((int(i), f"{cl.name}[{i}] {cl.label[i]}: obs[{j}] {got!r} is {e:.4g} bars from {float(exs[j])!r}"))
            else:
                note("obs", i, M.err_units(got, exs[j], uns[j]))
        # the reward: 0 - f_y within the bar, then exact float64 adds
        lo, hi, base, u = M.reward_interval(c, g["s_x"][i], g["s_y"][i], g["s_r"][i], g["rudder"][i],
                                            bars["reward"] if bars else 0.0)
        plain = M.reward_adds(c, 0.0, g["s_x"][i], g["s_r"][i], g["rudder"][i]) == 0.0
        if abs(base) < TINY:
            # below the smallest normal double the reference's own 1 + exp(..) has overflowed
            # (it returns 0 for an exact 1e-310): the stage asks for the class and the size only
            exact("|0 - f_y| below the smallest normal", i, bool(abs(g["reward"][i] if plain else 0.0) <= TINY), True)
        elif plain:
            note("reward", i, M.err_units(g["reward"][i], base, u))
        elif bars is not None and not lo <= g["reward"][i] <= hi:
            fails.append((int(i), f"{cl.name}[{i}] {cl.label[i]}: reward {g['reward'][i]!r} outside [{lo!r}, {hi!r}]"))
        exact("ep_reward", i, g["ep_reward"][i], np.float64(a["ep_reward"][i]) + g["reward"][i])
        # the chain, truncation, last_term and the counters: exact, from the step's own values
        term = M.chain(c, g["s_x"][i], g["s_y"][i], fuel, g["t"][i], g["rudder"][i])
        term, done, col, lt = M.episode_end(term, int(a["index"][i]) + 1, MAX_EPISODE_STEPS, int(a["last_term"][i]))
        exact("term", i, int(out["term"][i]), term)
        exact("done", i, int(out["done"][i]), done)
        exact("last_term", i, int(out["last_term"][i]), lt)
        for k5 in range(5):
            exact(f"counter {k5}", i, int(out["counters"][k5][i]), int(k5 == col))
    return worst, fails


def overall(worst: dict, for_c_ref: bool = False) -> dict:
    """The largest figure per stage over the families; ``for_c_ref`` leaves out the
    position stages at |s_r'| > pi (LARGE_S_R)."""
    return {s: max((v for k, v in f.items() if not (for_c_ref and k.endswith(LARGE_S_R))), default=0.0)
            for s, f in worst.items()}
