"""The boat step kernel, stage by stage, against a high-precision oracle at the edges.

One step of every case of oracle/boat_step_cases.py (states written through
``VecBoatEnv``'s arena views, wind through a shared ``wind_table`` row picked by the
written ``index``), each stage judged alone against oracle/boat_step_mp.py (mpmath,
320 bits) FROM THE KERNEL'S OWN UPSTREAM OUTPUTS: a_x from the written state, v_x'
from the kernel's a_x, a_y from the kernel's v_x', s_x' from the kernel's v_x', v_y',
s_r', the reward from the kernel's s_y', s_r' and rudder. Units and bars:
oracle/boat_step_cases.py (4 x the numpy reference's own error, per config and stage;
obs: half a float32 ulp plus the float64 stage's bar). The termination chain,
truncation, counters, ``last_term``, the rudder, t and ep_reward are exact.

* accuracy: the one-step launch (autoreset off, accel and reward64 recorded);
* lane placement: a fast-path case gives the same bits in a wave of in-range lanes,
  in a wave whose other lanes take the slow paths, and beside one slow lane;
* launch forms: rollout, the segment launch in general and lean form, the one-step
  launch with autoreset, and the list tiled past the dense threshold, against the
  one-step launch's bits;
* non-finite actions: the class of every output and the term code are the reference's.

``SACENV_STEP_RECORD=<file>`` appends the measured figures (one JSON line per config)
for tools/boat_step_margins.py --native.
Reference: environment/boat_env.py:67-115, :203-326, reward_functions.py:42-57.
"""
import json
import os

import numpy as np
import pytest
import torch

import boat_step_cases as K

pytestmark = pytest.mark.gpu

STATE = ("s_x", "s_y", "s_r", "v_x", "v_y", "v_r", "rudder", "ep_reward")
F64_OUT = ("a_x", "a_y", "a_r") + STATE + ("t", "reward")
ALL_OUT = F64_OUT + ("obs", "reward32", "term", "done", "last_term", "counters", "index", "final_ep_reward")


def make_env(name, gpu, tiles=1, **kw):
    """A VecBoatEnv holding the case list of ``name`` (``tiles`` times over), and its actions."""
    from sacenv import VecBoatEnv
    cl = K.build(name)
    env = VecBoatEnv(K.env_config(name), cl.N * tiles, seed=1, device=gpu, wind_table=cl.table,
                     max_episode_steps=K.MAX_EPISODE_STEPS, **kw)
    a = cl.arrays
    put = lambda view, arr: view.copy_(torch.from_numpy(np.tile(arr, tiles)).to(gpu))  # noqa: E731
    for k in STATE:
        put(getattr(env, k), a[k])
    put(env._t_view, a["t"])
    put(env.index, a["index"])
    put(env.last_term, a["last_term"])
    return env, torch.from_numpy(np.tile(a["action"], tiles)).to(gpu).contiguous()


def collect(env, names=ALL_OUT) -> dict:
    """Host copies of what a step left in the arena (numpy, contiguous)."""
    torch.cuda.synchronize(env.device)
    src = {"a_x": lambda: env.accel[0], "a_y": lambda: env.accel[1], "a_r": lambda: env.accel[2],
           "t": lambda: env.t, "reward": lambda: env.reward64, "reward32": lambda: env.reward}
    return {k: (src[k]() if k in src else getattr(env, k)).cpu().contiguous().numpy() for k in names}


def same_bits(a, b) -> np.ndarray:
    """Per env: are the two arrays' rows the same bytes (NaNs and signed zeros included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    n = a.shape[-1] if a.ndim == 2 and a.shape[0] == 5 else a.shape[0]
    if a.ndim == 2 and a.shape[0] == 5:      # counters [5, N]
        a, b = a.T.copy(), b.T.copy()
    return (a.view(np.uint8).reshape(n, -1) == b.view(np.uint8).reshape(n, -1)).all(axis=1)


def assert_same(got: dict, want: dict, names, where: str, rows=None, labels=None):
    for k in names:
        ok = same_bits(got[k], want[k])
        if rows is not None:
            ok = ok | ~rows
        bad = np.flatnonzero(~ok)
        assert bad.size == 0, (f"{k} differs {where} in {bad.size} envs, first {bad[0]}"
                               + (f" ({labels[bad[0]]})" if labels else ""))


@pytest.fixture(scope="module")
def one_step(gpu, built_lib):
    """The one-step launch's outputs per config (computed once, read only)."""
    cache = {}

    def get(name):
        if name not in cache:
            env, act = make_env(name, gpu, autoreset=False, record_accel=True, record_reward64=True)
            env.step_async(act)
            cache[name] = collect(env)
            env.check_status()
        return cache[name]
    return get


def inf_rows(cl) -> np.ndarray:
    return np.isinf(cl.arrays["action"])


# ---------------------------------------------------------------- accuracy
@pytest.mark.parametrize("name", list(K.CONFIGS))
def test_stage_accuracy(name, one_step):
    """Every case, every stage, within 4 x the numpy reference's own error (C_REF)."""
    cl, out = K.build(name), one_step(name)
    bars = {s: K.bar(name, s) for s in K.STAGES}
    worst, fails = K.measure(cl, out, bars, obs_f32=True)
    figures = K.overall(worst)
    for s in K.STAGES:
        print(f"{name} {s:7s} worst {figures[s]:9.3f} (bar {bars[s] if s != 'obs' else 1.0:9.3f})  "
              + "  ".join(f"{f} {v:.3f}" for f, v in sorted(worst[s].items())))
    rec = os.environ.get("SACENV_STEP_RECORD")
    if rec:
        with open(rec, "a") as f:
            f.write(json.dumps({name: {"worst": figures, "worst_by_family": worst, "cases": cl.N,
                                       "device": torch.cuda.get_device_name(0)}}, sort_keys=True) + "\n")
    skip = inf_rows(cl)      # (+-inf actions: test_infinite_action)
    fails = [m for i, m in fails if not skip[i]]
    assert not fails, f"{len(fails)} violations, the first:\n" + "\n".join(fails[:12])
    # the record's float32 reward is the float64 one rounded once; an ended env's
    # final_ep_reward is its ep_reward = RN(ep + reward) (checked in measure)
    with np.errstate(over="ignore"):
        assert same_bits(out["reward32"], out["reward"].astype(np.float32)).all()
    done = out["done"] != 0
    assert same_bits(out["final_ep_reward"], out["ep_reward"])[done].all()
    assert done.any()


# ---------------------------------------------------------------- lane placement
@pytest.mark.parametrize("name", ["dt025", "dt01"])
def test_lane_placement(name, one_step):
    """A lane's result depends on its own arguments only: the placements of each
    fast-path case (all lanes in range / other lanes on the slow paths / one slow
    lane) agree in every output, bit for bit."""
    cl, out = K.build(name), one_step(name)
    assert len(cl.pairs) >= cl.n_fast + 63
    i = np.array([p[0] for p in cl.pairs])
    j = np.array([p[1] for p in cl.pairs])
    for k in ALL_OUT:
        if k == "index":
            continue
        v = out[k].T if k == "counters" else out[k]
        ok = same_bits(np.ascontiguousarray(v[i]), np.ascontiguousarray(v[j]))
        bad = np.flatnonzero(~ok)
        assert bad.size == 0, (f"{k} depends on the other lanes in {bad.size} cases, first: {cl.label[j[bad[0]]]} "
                               f"{v[i[bad[0]]]!r} vs {v[j[bad[0]]]!r}")


# ---------------------------------------------------------------- launch forms
def _fresh(env, cl, ended, got, where):
    """An ended env after its restart: a fresh Boat (boat_env.py:152-198) and its first obs."""
    tmpl = env.first_obs_template().numpy()
    assert same_bits(got["obs"], np.broadcast_to(tmpl, got["obs"].shape).copy())[ended].all(), f"restart row {where}"
    for k in STATE + ("t",):
        assert (got[k][ended] == 0.0).all(), f"{k} after the restart {where}"
    assert (got["index"][ended] == 0).all()


@pytest.mark.parametrize("form", ["rollout", "segment", "segment_lean", "step_autoreset", "dense"])
@pytest.mark.parametrize("name", list(K.CONFIGS))
def test_launch_forms(name, form, gpu, one_step):
    """Everything each launch form exposes equals the one-step launch's bits."""
    cl, want = K.build(name), one_step(name)
    where = f"({name}, {form})"
    if form in ("rollout", "segment", "dense"):
        tiles = 1
        if form == "dense":     # more owner waves than 4 per CU: the dense instantiation
            cus = torch.cuda.get_device_properties(gpu).multi_processor_count
            tiles = (4 * cus * 64) // cl.N + 2
            assert (cl.N * tiles + 63) // 64 > 4 * cus
        env, act = make_env(name, gpu, tiles=tiles, autoreset=False, record_accel=True, record_reward64=True)
        names = [k for k in ALL_OUT]
        if form == "rollout":
            fin = torch.zeros((1, env.n_pad, 11), dtype=torch.float32, device=gpu)
            rec, _ = env.rollout(act[None], final_obs=fin)
            got = collect(env, [k for k in ALL_OUT if k not in ("obs", "reward32", "term", "done")])
            o, r, d, t = env.record_views(rec[0])
            got.update(obs=o.cpu().numpy(), reward32=r.cpu().numpy(), done=d.cpu().numpy(), term=t.cpu().numpy())
        else:
            env.segment_async(act[None], 1)
            got = collect(env)
        env.check_status()
        first = {k: (v[:, :cl.N] if k == "counters" else v[:cl.N]) for k, v in got.items()}
        assert_same(first, want, names, where, labels=cl.label)
        for tile in range(1, tiles):     # every tile equals the first
            s = slice(tile * cl.N, (tile + 1) * cl.N)
            part = {k: (v[:, s] if k == "counters" else v[s]) for k, v in got.items()}
            assert_same(part, first, names, f"between tile {tile} and tile 0 {where}", labels=cl.label)
        return
    # autoreset on, no optional outputs: the lean segment launch, and the one-step launch
    env, act = make_env(name, gpu, autoreset=True)
    if form == "segment_lean":
        env.segment_async(act[None], 1)
    else:
        env.step_async(act)
    names = STATE + ("t", "index", "obs", "reward32", "term", "done", "last_term", "counters", "final_ep_reward")
    got = collect(env, names + ("final_obs", "cons"))
    env.check_status()
    ended = want["done"] != 0
    assert_same(got, want, ("reward32", "term", "done", "last_term", "counters"), where, labels=cl.label)
    assert_same(got, want, STATE + ("t", "index", "obs"), f"for live envs {where}", rows=~ended, labels=cl.label)
    assert same_bits(got["final_obs"], want["obs"])[ended].all(), f"final_obs {where}"
    assert same_bits(got["final_ep_reward"], want["ep_reward"])[ended].all(), f"final_ep_reward {where}"
    assert (got["cons"] == ended).all()
    _fresh(env, cl, ended, got, where)


# ---------------------------------------------------------------- non-finite actions
def _class_failures(cl, out, rows):
    ref = K.numpy_step(cl)
    bad = []
    for k in K.OUT_F64 + ("obs", "term"):
        a, b = np.asarray(out[k], np.float64), np.asarray(ref[k], np.float64)
        same = (K.M.classify(a) == K.M.classify(b)).reshape(cl.N, -1).all(axis=1)
        if k == "term":
            same = a == b
        for i in np.flatnonzero(~same & rows):
            bad.append(f"{cl.label[i]}: {k} is {a[i]!r}, the reference's {b[i]!r}")
    return bad


@pytest.mark.parametrize("name", ["dt025", "dt01"])
def test_nan_action(name, one_step):
    """action = NaN: a NaN rudder and no termination, in the reference and here."""
    cl = K.build(name)
    rows = np.isnan(cl.arrays["action"])
    assert rows.sum() == 2
    assert not _class_failures(cl, one_step(name), rows)


@pytest.mark.parametrize("name", ["dt025", "dt01"])
def test_infinite_action(name, one_step):
    """action = +-inf: the reference's action / 10 is +-inf, so the rudder is +-inf and the
    episode ends with rudder_broken (s_y', and with it the reward, are NaN: sin(inf))."""
    cl, out = K.build(name), one_step(name)
    rows = inf_rows(cl)
    assert rows.sum() == 4
    bad = _class_failures(cl, out, rows)
    assert not bad, "\n".join(bad)
    assert np.isinf(out["rudder"][rows]).all() and (out["term"][rows] == 4).all() and out["done"][rows].all()
    assert (np.sign(out["rudder"][rows]) == np.sign(cl.arrays["action"][rows])).all()
