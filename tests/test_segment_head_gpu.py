"""The head of the persistent segment's step loop: its one rare-event region.

The multi-step loop tests once, at the head of a step, whether any lane of the
wave refreshes its spline piece (``index == 0`` or the next step enters another
knot interval). The piece gathers and, nested behind a uniform test of their
own, the next-episode header gathers (``index == 0`` lanes) sit in that region;
the refresh copy at the step's end reuses the saved result. Every case here runs
a persistent launch (``sacenv_boat_segment``) against the same steps taken as
per-step launches (``sacenv_boat_step``, pinned to the reference by
tests/test_gpu_parity.py): bit for bit the same record, terminal obs, counters
and carried arena. The comparisons are on the bits, so NaN equals NaN.

Shape: 130 envs, two full owner waves and one with padding lanes; experiment 6
unless stated.
Reference: environment/boat_env.py:67-126.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 130
STATE = ("s_x", "s_y", "s_r", "v_x", "v_y", "v_r", "rudder", "ep_reward", "t", "index")
RECORD = ("obs", "reward", "done", "term", "final_obs", "final_ep_reward")
COUNTS = ("counters", "cons", "last_term")
NAMES = STATE + RECORD + COUNTS
RUDDER_BROKEN, TRUNCATED = 4, 6


def _env(gpu, exp=6, episode=0, test_mode=0, cfg=None, **kw):
    from sacenv import VecBoatEnv
    c = {"base_settings": {"experiment": exp, "test_mode": test_mode}}
    c.update(cfg or {})      # (a cfg with base_settings replaces them)
    return VecBoatEnv(c, N, seed=5, device=gpu, max_episode_steps=episode, n_helpers=64, auto_refill=False, **kw)


def _bits(x):
    x = x.contiguous()
    return x.view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[x.element_size()])


def _assert_same(a, b, where, names=NAMES):
    for name in names:
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), f"{name} differs ({where})"
    assert torch.equal(a.arena, b.arena), f"the carried arena differs ({where})"


def _actions(gpu, K, seed):
    g = torch.Generator(device=gpu)
    g.manual_seed(seed)
    return torch.rand((K, N), generator=g, device=gpu) * 2 - 1


def _stepped(ref, rows, names=("index",)):
    """Take rows as per-step launches on ref; per step, the named views BEFORE the step
    and (suffix _after) after it."""
    out = {n: [] for n in names}
    out.update({n + "_after": [] for n in names})
    for row in rows:
        for n in names:
            out[n].append(getattr(ref, n).clone())
        ref.step_async(row)
        for n in names:
            out[n + "_after"].append(getattr(ref, n).clone())
    torch.cuda.synchronize()
    return {n: torch.stack(v).cpu().numpy() for n, v in out.items()}


def _kinds(ref, index):
    """Per step and wave, from the per-step launches' index values [K, N]: does a lane of
    the wave start an episode (index 0), does one enter another knot interval next step."""
    p = ref.params
    last = int(p.wind_len) - 1

    def interval(i):  # knot_coord(p, min(i, wind_len - 1)).j
        j = (np.minimum(i, last).astype(np.float64) * float(p.knot_step)).astype(np.int64)
        return np.minimum(j, int(p.n_knots) - 2)

    first = index == 0
    change = interval(index + 1) != interval(index)
    waves = [slice(0, 64), slice(64, 128), slice(128, N)]
    return [(first[:, w].any(axis=1), change[:, w].any(axis=1)) for w in waves]


SHORT = {"base_settings": {"experiment": 6, "test_mode": 0, "t_max": 40.0}}   # 160 grid steps, 8 knots


@pytest.mark.parametrize("episode", [50, 7])
def test_refresh_combinations(episode, gpu, built_lib):
    """160 steps in one launch on a 160-step wind grid (t_max 40: a knot interval is 22.7
    steps, so every env crosses several; the default grid's is 1 428 steps).
    50-step episodes: the lanes step together, index 0 at steps 0, 50, 100, 150 and an
    interval change after indices 22 and 45, except one lane per wave whose rudder breaks
    at step 21: it starts an episode at step 22, the step in which its neighbours change
    interval. So each wave sees all four kinds of step: no refresh, a change alone, a start
    alone, both. 7-step episodes with the lanes spread over the seven phases: a header
    refresh in nearly every step."""
    K = 160
    acts = _actions(gpu, K, 11)
    if episode == 50:
        for lane in (9, 73, 129):
            acts[:21, lane] = 0.0
            acts[21, lane] = 12.0     # rudder 0 + 1.2 > pi / 3: broken
    else:
        acts[:7] = 0.0
        lanes = torch.arange(N, device=gpu)
        acts[lanes % 7, lanes] = 12.0
    seg, ref = _env(gpu, episode=episode, cfg=SHORT), _env(gpu, episode=episode, cfg=SHORT)
    seg.segment_async(acts, K)
    steps = _stepped(ref, acts)
    _assert_same(seg, ref, f"{episode}-step episodes, after {K} steps")
    # the carried piece and header copies feed the next launch: 24 steps more, per step on both
    for row in _actions(gpu, 24, 12):
        seg.step_async(row)
        ref.step_async(row)
    torch.cuda.synchronize()
    _assert_same(seg, ref, f"{episode}-step episodes, 24 steps after the launch")
    seg.check_status()
    ref.check_status()
    kinds = _kinds(ref, steps["index"])
    # steps per wave by kind: (none, change alone, start alone, both)
    tally = [[int(((first == a) & (change == b)).sum()) for a in (False, True) for b in (False, True)]
             for first, change in kinds]
    print("steps by kind (none, change, start, both) per wave:", tally)
    if episode == 50:
        assert all(min(t) > 0 for t in tally), f"a kind of step did not occur: {tally}"
    else:   # (the padded wave has two envs: two of the seven phases)
        assert all(t[2] + t[3] >= K - 8 for t in tally[:2]) and tally[2][2] + tally[2][3] >= 2 * (K // 7) - 2, \
            f"a header refresh in nearly every step: {tally}"


def _nonfinite_table(gpu):
    """40 steps. Lane 3: +inf at step 0 (its rudder breaks, it restarts) and -inf at step 1,
    the first step of its next episode. Lane 70: -inf at step 17. Lane 129 (the padded
    wave): NaN at step 9, which breaks nothing -- every comparison with NaN is false --
    so its episode goes on with a NaN state, and +inf at step 12 of the same episode.
    Lanes 40 and 100: +inf and NaN at step 8, the step after every lane's truncation."""
    t = _actions(gpu, 40, 21)
    inf, nan = float("inf"), float("nan")
    for k, e, v in ((0, 3, inf), (1, 3, -inf), (17, 70, -inf), (9, 129, nan), (12, 129, inf),
                    (8, 40, inf), (8, 100, nan)):
        t[k, e] = v
    return t


@pytest.mark.parametrize("autoreset", [True, False])
def test_non_finite_actions(autoreset, gpu, built_lib):
    """Non-finite actions in single lanes, their neighbours' finite: a lean launch
    (autoreset) and the general one (autoreset off). Five warm-up steps first, so the
    rudders are non-zero at the launch's step 0 (a restarting lane's is 0 by definition).
    One env takes the 40 steps in ONE launch; a second in launches cut after every event
    step and the step after it, so each event's termination code, the reset that follows
    and the last-termination word are compared where they happen; a third writes every
    step's staged row in one launch (term, last termination, reward, pre-reset obs of all
    40 steps)."""
    from sacenv import _lib
    K, WARM, EPISODE = 40, 5, 13
    table, warm = _nonfinite_table(gpu), _actions(gpu, WARM, 22)
    envs = [_env(gpu, episode=EPISODE, autoreset=autoreset) for _ in range(4)]
    one, cut, staged, ref = envs
    for e in envs[:3]:
        e.segment_async(warm, WARM)
    for row in warm:
        ref.step_async(row)
    torch.cuda.synchronize()
    _assert_same(one, ref, "after the warm-up")
    assert bool((ref.rudder[[3, 70, 129]] != 0).all())
    # the reference, per step: the record and the counters after each step
    names = ("term", "done", "last_term", "reward", "obs", "final_obs", "cons", "rudder")
    snaps = []
    for k in range(K):
        ref.step_async(table[k])
        snaps.append({n: getattr(ref, n).clone() for n in names})
    torch.cuda.synchronize()
    # what the table claims, on the reference itself
    term = torch.stack([s["term"] for s in snaps]).cpu().numpy()
    assert term[0, 3] == RUDDER_BROKEN and term[17, 70] == RUDDER_BROKEN and term[8, 40] == RUDDER_BROKEN
    if autoreset:     # (off: every env is past its 13 steps from step 7 on, truncated in every step)
        assert term[7, 40] == TRUNCATED and term[7, 100] == TRUNCATED and term[1, 3] == RUDDER_BROKEN
        assert term[9, 129] == 0 and term[8, 100] == 0, "a NaN action ends no episode"
        assert term[12, 129] == 0, "a NaN rudder stays NaN, whatever the action"
    # one launch
    one.segment_async(table, K)
    torch.cuda.synchronize()
    _assert_same(one, ref, f"one {K}-step launch, autoreset {autoreset}")
    # launches cut after each event and after the step that follows it
    k = 0
    for stop in (1, 2, 8, 9, 10, 12, 13, 14, 17, 18, 19, K):
        cut.segment_async(table[k:stop], stop - k)
        torch.cuda.synchronize()
        for n in names:
            assert torch.equal(_bits(getattr(cut, n)), _bits(snaps[stop - 1][n])), f"{n} after step {stop - 1}"
        k = stop
    _assert_same(cut, ref, f"cut launches, autoreset {autoreset}")
    # every step of one launch, through its staged rows
    NP = staged.n_pad
    stage = torch.zeros(NP * K * 64, dtype=torch.uint8, device=gpu)
    staged.segment_async(table, K, stage=stage)
    torch.cuda.synchronize()
    _assert_same(staged, ref, f"staged launch, autoreset {autoreset}")
    words = stage.view(torch.int32).view(NP, K, 16)[:N]
    codes = stage.view(NP, K, 64)[:N]
    for k, s in enumerate(snaps):
        ended = (s["done"] != 0) & autoreset          # a restarting env's s' is its terminal obs
        s_next = torch.where(ended[:, None], s["final_obs"], s["obs"])
        assert torch.equal(words[:, k, :_lib.OBS_DIM], _bits(s_next)), f"staged row {k}: s'"
        assert torch.equal(words[:, k, 11], _bits(s["reward"])), f"staged row {k}: reward"
        assert torch.equal(words[:, k, 12], _bits(table[k])), f"staged row {k}: action"
        assert torch.equal(codes[:, k, 52], s["term"]), f"staged row {k}: term"
        assert torch.equal(codes[:, k, 53].to(torch.int32), s["last_term"]), f"staged row {k}: last termination"
    for e in envs:
        e.check_status()


def _occupancy(lib, env):
    out = [ctypes.c_int32() for _ in range(4)]
    assert lib.sacenv_boat_segment_occupancy(ctypes.byref(env.params), 0, *[ctypes.byref(o) for o in out]) == 0
    return tuple(o.value for o in out)


GENERAL = {
    "test_mode": dict(test_mode=1),
    "out_flags": dict(record_reward64=True),
    "exp2": dict(exp=2),
    "no_fuel": dict(cfg={"boat": {"fuel": 0}}),
}


@pytest.mark.parametrize("option", sorted(GENERAL))
def test_general_options(option, gpu, built_lib):
    """test_mode = 1 (the action does not move the rudder; the loop tests it at run time,
    lean or not) and each option the lean instantiation excludes: 40 steps equal the
    per-step launches. The occupancy report carries resources, not a name: it must
    succeed, describe this grid, and be the one report of every launch of the same owner
    that one of the excluded options makes general."""
    K, kw = 40, GENERAL[option]
    acts = _actions(gpu, K, 31)
    acts[:, ::7] *= 12.0
    seg, ref = _env(gpu, episode=13, **kw), _env(gpu, episode=13, **kw)
    seg.segment_async(acts, K)
    steps = _stepped(ref, acts, names=("rudder",))
    names = NAMES + (("reward64",) if option == "out_flags" else ())
    _assert_same(seg, ref, option, names)
    seg.check_status()
    if option == "test_mode":
        assert not steps["rudder_after"].any(), "test_mode: the rudder stays where it is"
    assert (option == "test_mode" or int(ref.counters.sum()) > 0) and int(ref.cons.min()) >= K // 13
    per_cu, grid, vgprs, lds_bytes = _occupancy(built_lib, seg)
    assert grid == 3 and per_cu > 0 and 0 < vgprs <= 512 and lds_bytes > 0
    if option in ("out_flags", "no_fuel"):      # the same owner (two curves, t from the index)
        other = _env(gpu, episode=13, **GENERAL["out_flags" if option != "out_flags" else "no_fuel"])
        assert _occupancy(built_lib, other) == (per_cu, grid, vgprs, lds_bytes)


@pytest.mark.parametrize("case", ["exp4", "exp5", "exp1", "wind_table"])
def test_every_curve_count(case, gpu, built_lib):
    """One curve (experiments 4 and 5) and none (experiment 1; experiment 6 on a recorded
    wind table): the restructured head for every curve count, 40 steps."""
    K = 40
    acts = _actions(gpu, K, 41)
    acts[:, ::7] *= 12.0
    kw = dict(exp={"exp4": 4, "exp5": 5, "exp1": 1, "wind_table": 6}[case], episode=13)
    if case == "wind_table":
        from sacenv.config import BoatConfig
        L = BoatConfig().wind_len
        i = np.arange(L, dtype=np.float64)
        kw["wind_table"] = np.stack([0.5 * np.sin(i / 7.0) ** 2, np.pi / 2 + 0.3 * np.cos(i / 11.0)])
    seg, ref = _env(gpu, **kw), _env(gpu, **kw)
    seg.segment_async(acts, K)
    _stepped(ref, acts)
    _assert_same(seg, ref, case)
    seg.check_status()
    assert int(ref.counters.sum()) > 0 and int(ref.cons.min()) >= K // 13
