"""The wind fit, curve by curve, against a high-precision oracle at its edges.

The wind of experiments 4, 5 and 6 is a per-episode not-a-knot spline fit: second
derivatives, the grid min/max from the critical points, the min-max renormalisation,
the fold into (y, m) pairs and the evaluation from one piece. Every case of
oracle/wind_fit_cases.py goes through ``reset_explicit(..., knots=...)`` (the wave fit)
and is judged against oracle/wind_fit_mp.py (mpmath, 320 bits) at two stages, each with
the whole bar (4 x the numpy reference's own error per config, in eps x top over the
renormalisation's span): ``fit``, the stored pairs evaluated exactly against the exact
table, and ``eval``, ``wind_eval`` against the exact value of the stored piece.
Decisive renormalisation and rectifier decisions must be the exact ones.

* accuracy of the wave fit, per config (knot counts 4 to 16, L 5 to 10 000);
* the refill's group fit stores the wave fit's bits (8- and 16-lane groups, full and
  not), at construction and after a refill;
* the wind the step uses: a_x of every step of an episode, past the end-of-table clamp,
  against the mpmath a_x from ``wind_eval``'s wind; the rollout launch, with the piece
  in registers across interval crossings, ends in the same bits.

``SACENV_WIND_RECORD=<file>`` appends the measured figures (one JSON line per config)
for tools/wind_fit_margins.py --native.
Reference: environment/wind.py:12-99.
"""
import json
import os

import numpy as np
import pytest
import torch

import boat_step_cases as SK
import boat_step_mp as SM
import wind_fit_cases as K
import wind_fit_mp as W

pytestmark = pytest.mark.gpu


def explicit_env(name, gpu, n, **kw):
    from sacenv import VecBoatEnv
    return VecBoatEnv(K.env_config(name), n, seed=1, device=gpu, autoreset=False, **kw)


def fit_explicit(env, knots) -> np.ndarray:
    """``knots`` [n, 2, nk] through reset_explicit (n <= num_envs) -> the stored pairs [n, 2, nk, 2]."""
    n = len(knots)
    env.reset_explicit(np.arange(n, dtype=np.int32), np.zeros(n, np.int32), np.ascontiguousarray(knots))
    torch.cuda.synchronize(env.device)
    return env.wind_knots[:n, 0].cpu().numpy()


def wave_fit(cl, gpu) -> dict:
    """What ``measure`` reads: the pairs and ``wind_eval`` at the judged indices."""
    env = explicit_env(cl.name, gpu, cl.N)
    pairs = fit_explicit(env, cl.knots)
    ids = np.repeat(np.arange(cl.N, dtype=np.int32), cl.idx.shape[1])
    wv, wa = env.wind_eval(ids, cl.idx.reshape(-1))
    torch.cuda.synchronize(gpu)
    env.check_status()
    return dict(pairs=pairs, wv=wv.cpu().numpy().reshape(cl.idx.shape), wa=wa.cpu().numpy().reshape(cl.idx.shape))


def report(name, worst, bar, ties, cl):
    for s in K.STAGES:
        print(f"{name} {s:5s} worst {K.overall(worst)[s]:8.3f} (bar {bar:8.3f})  "
              + "  ".join(f"{f} {v:.3f}" for f, v in sorted(worst[s].items())))
    for t in ties:
        print(f"{name} near tie [{t['case']}.{t['curve']}] {t['label']}: {t['what']} margin {t['margin']:+.3g}, "
              f"exact {t['exact']}, kernel {t['took']}")
    rec = os.environ.get("SACENV_WIND_RECORD")
    if rec:
        ref_ties: list = []
        K.measure(cl, K.numpy_reference(cl), None, is_reference=True, tie_bar=bar, report=ref_ties)
        with open(rec, "a") as f:
            f.write(json.dumps({name: {"worst": K.overall(worst), "worst_by_family": worst, "cases": cl.N,
                                       "near_ties": K.tie_summary(ties, ref_ties),
                                       "device": torch.cuda.get_device_name(0)}}, sort_keys=True) + "\n")


# ---------------------------------------------------------------- accuracy
@pytest.mark.parametrize("name", list(K.CONFIGS))
def test_wave_fit_accuracy(name, gpu, built_lib):
    """Every case, both stages, within 4 x the numpy reference's own error (C_REF); every
    decisive renormalisation and rectifier decision is the exact one."""
    cl = K.build(name)
    out = wave_fit(cl, gpu)
    ties: list = []
    worst, fails = K.measure(cl, out, K.bar(name), report=ties)
    report(name, worst, K.bar(name), ties, cl)
    assert not fails, f"{len(fails)} violations, the first:\n" + "\n".join(m for _, m in fails[:12])


@pytest.mark.parametrize("name", ["e6_k4_L400", "e6_k8_L37", "e6_k10_L120", "e6_k16_L37"])
def test_tiny_curves_fit_like_their_scaled_twins(name, gpu, built_lib):
    """A renormalised curve does not depend on its scale: knots times a power of two scale
    every step of the fit exactly, so the tiny curves' order-one twins, scaled down by
    2^-800 (1e-241: their squares underflow, nothing else does), store the twins' bits.
    (The accuracy test's unit divides by the span and cannot see such curves: before the
    critical points' quadratic was scaled, its squares underflowed, the grid extremes were
    missed and the curve was left unrenormalised: "spike of 1e-300" at 4 knots, L = 400.)"""
    cl = K.build(name)
    rows = sorted({n for n, c, cu in cl.curves() if "1e-300" in cu["label"]})
    assert rows
    twin = cl.knots[rows] * 2.0 ** 996
    tiny = twin * 2.0 ** -800
    assert (tiny * 2.0 ** 800 == twin).all()
    env = explicit_env(name, gpu, len(tiny))
    a, b = fit_explicit(env, tiny), fit_explicit(env, twin)
    checked = 0
    for n in range(len(tiny)):
        for c in range(2):
            if 0 < np.abs(tiny[n, c]).max() < 1e-200 and W.curve(twin[n, c], cl.L).renorm():
                checked += 1
                assert a[n, c].tobytes() == b[n, c].tobytes(), (cl.rows[rows[n]]["curves"][c]["label"], a[n, c], b[n, c])
    assert checked >= 1


# ---------------------------------------------------------------- the group fit
GROUP = {5: "e6_k5_L120", 8: "e6_k8_L37", 12: "e6_k12_L120", 16: "e6_k16_L37"}


def _same_pairs(a, b, where):
    same = (a.view(np.uint64) == b.view(np.uint64)).reshape(len(a), -1).all(axis=1)
    bad = np.flatnonzero(~same)
    assert bad.size == 0, f"{bad.size} of {len(a)} fits differ {where}, first {bad[0]}: {a[bad[0]]!r} vs {b[bad[0]]!r}"


@pytest.mark.parametrize("nk", list(GROUP))
def test_group_fit_is_the_wave_fit(nk, gpu, built_lib):
    """k_refill_fit's lane groups store the bits fit_store_wave stores from the same knots:
    every slot drawn at construction, and the slots a refill replaces after a segment of
    short episodes; 32 of the curves are also held to the oracle."""
    from sacenv import VecBoatEnv, _lib
    name = GROUP[nk]
    n, batch = 256, 4096
    env = VecBoatEnv(K.env_config(name), n, seed=7, device=gpu, autoreset=True, record_knots=True,
                     max_episode_steps=7)
    wave = explicit_env(name, gpu, batch)

    def slots():
        torch.cuda.synchronize(gpu)
        return (env.knots_raw_slots[:n].cpu().numpy().reshape(-1, 2, nk),
                env.wind_knots[:n].cpu().numpy().reshape(-1, 2, nk, 2))

    def compare(raw, pairs, where):
        for a in range(0, len(raw), batch):
            _same_pairs(pairs[a:a + batch], fit_explicit(wave, raw[a:a + batch]), where)

    raw0, pairs0 = slots()
    assert len(raw0) == n * _lib.SLOTS
    compare(raw0, pairs0, "at construction")
    # a subsample against the oracle: the first 16 envs' slot 1 (a refill-launch fit)
    cl = K.CaseList(name)
    for e in range(16):
        for c in range(2):
            cl.add("random", f"drawn env {e} slot 1 curve {c}", raw0[e * _lib.SLOTS + 1, c])
    cl.finish()
    got = wave_fit(cl, gpu)
    _same_pairs(got["pairs"], pairs0[[e * _lib.SLOTS + 1 for e in range(16)]], "in the subsample")
    worst, fails = K.measure(cl, got, K.bar(name))
    assert not fails, "\n".join(m for _, m in fails[:12])
    # one segment of 7-step episodes consumes 36 slots per env; the refill replaces them
    env.segment_async(torch.zeros((256, n), dtype=torch.float32, device=gpu), 256)
    env.refill()
    raw1, pairs1 = slots()
    env.check_status()
    new = np.flatnonzero((raw1 != raw0).reshape(len(raw1), -1).any(axis=1))
    assert new.size >= 30 * n, new.size
    compare(raw1[new], pairs1[new], "after the refill")
    old = np.setdiff1d(np.arange(len(raw1)), new)
    _same_pairs(pairs1[old], pairs0[old], "in slots the refill left alone")


# ---------------------------------------------------------------- the wind the step uses
def test_step_uses_the_evaluated_wind(gpu, built_lib):
    """Every step's a_x is the mpmath a_x (boat_step_mp) of the state before the step and
    the wind ``wind_eval`` gives at min(index, L - 1), within the boat step's own a_x bar:
    a step reading a neighbouring piece at an interval boundary fails it
    (tests/test_wind_fit_mp_cpu.py::test_step_test_sees_a_neighbouring_piece). Then the
    same episode in one rollout launch ends in the same bits."""
    from sacenv import VecBoatEnv
    knots, L = K.step_knots(), K.STEP_L
    n = len(knots)
    cfg = SK.env_config("dt025")       # the boat constants of that list's bar
    cfg["base_settings"].update(test_mode=1, t_max=L * 0.25)
    cfg["wind"] = {"fixed_points": knots.shape[2]}
    c = SK.oracle_config("dt025")
    bar = SK.bar("dt025", "a_x")
    ids = np.arange(n, dtype=np.int32)
    zero = torch.zeros(n, dtype=torch.float32, device=gpu)
    state = ("s_x", "s_y", "s_r", "v_x", "v_y", "v_r", "rudder", "ep_reward", "index")

    env = VecBoatEnv(cfg, n, seed=1, device=gpu, autoreset=False, record_accel=True)
    env.reset_explicit(ids, np.zeros(n, np.int32), knots)
    worst, crossings = 0.0, 0
    last_j = np.zeros(n, np.int64)
    for k in range(L + 3):
        torch.cuda.synchronize(gpu)
        index = env.index.cpu().numpy()
        assert (index == k).all()
        before = {f: getattr(env, f).cpu().numpy() for f in ("v_x", "v_y", "v_r")}
        wv, wa = env.wind_eval(ids, np.minimum(index, L - 1).astype(np.int32))
        env.step_async(zero)
        torch.cuda.synchronize(gpu)
        a_x, wv, wa = env.accel[0].cpu().numpy(), wv.cpu().numpy(), wa.cpu().numpy()
        for e in range(n):
            ex, u = SM.a_x(c, before["v_x"][e], before["v_y"][e], before["v_r"][e], wv[e], wa[e])
            err = SM.err_units(a_x[e], ex, u)
            worst = max(worst, err)
            assert err <= bar, f"step {k} env {e}: a_x {a_x[e]!r} is {err:.4g} units from {float(ex)!r} (bar {bar:.4g})"
        j = np.minimum((np.minimum(index, L - 1) * ((knots.shape[2] - 1) / (L - 1))).astype(np.int64), knots.shape[2] - 2)
        crossings += int((j != last_j).sum())
        last_j = j
    print(f"a_x worst {worst:.3f} units (bar {bar:.3f}) over {L + 3} steps, {crossings} interval crossings")
    assert crossings == n * (knots.shape[2] - 2)
    env.check_status()
    final = {f: getattr(env, f).cpu().numpy() for f in state}

    roll = VecBoatEnv(cfg, n, seed=1, device=gpu, autoreset=False, record_accel=True)
    roll.reset_explicit(ids, np.zeros(n, np.int32), knots)
    roll.rollout(torch.zeros((L + 3, n), dtype=torch.float32, device=gpu))
    torch.cuda.synchronize(gpu)
    roll.check_status()
    for f in state:
        got = getattr(roll, f).cpu().numpy()
        assert got.tobytes() == final[f].tobytes(), f"{f} after the rollout differs from the one-step launches'"
