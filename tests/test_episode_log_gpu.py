"""The episode log on the GPU (sacenv_episodes.hip, sacenv/episodes.py).

The expected log of every case is ``numpy_scan``: the semantics of
include/sacenv_episodes.h restated in numpy and applied to the same records copied
to the host -- per step and env one f64 add of the record's f32 reward (from +0.0 at
an episode's first step) and one length increment; a set done byte emits
(end_step, score, env, length, term) and zeroes both. end_step, env, length, term
and the order must be equal and the score BIT-equal: the order of the adds is fixed.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from boat_oracle import OracleConfig, OracleVecBoat
from conftest import ROOT

pytestmark = pytest.mark.gpu

ENTRY = np.dtype([("end_step", "<i8"), ("score", "<f8"), ("env", "<i4"), ("length", "<i4"), ("term", "<u4"),
                  ("reserved", "<u4")])
EXACT = ("end_step", "env", "length", "term")


def numpy_scan(reward, done, term, n_envs, step0=0, env_base=0, score=None, length=None):
    """reward f32 [K, >= n_envs], done / term u8 alike -> (entries, carry score, carry length)."""
    score = np.zeros(n_envs, np.float64) if score is None else np.array(score, np.float64)
    length = np.zeros(n_envs, np.int32) if length is None else np.array(length, np.int32)
    out = []
    for k in range(reward.shape[0]):
        score = score + reward[k, :n_envs].astype(np.float64)
        length = length + 1
        for e in np.flatnonzero(done[k, :n_envs]):
            out.append((step0 + k, score[e], env_base + e, length[e], term[k, e], 0))
            score[e], length[e] = 0.0, 0
    return np.array(out, dtype=ENTRY), score, length


def assert_same_log(got, want):
    """Every field exactly, the score by its bits."""
    assert len(got) == len(want)
    for f in EXACT:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    np.testing.assert_array_equal(got["score"].view(np.uint64), want["score"].view(np.uint64), err_msg="score bits")


def full(entries):
    """A drained array (the 5 named fields of 32-B entries) as ENTRY with reserved = 0."""
    out = np.zeros(len(entries), ENTRY)
    for f in EXACT + ("score",):
        out[f] = entries[f]
    return out


# ---------------------------------------------------------------- 1. synthetic records, no env

def _synthetic(N, K, density, seed, filler=True):
    """Host records in a layout that is not the boat's: per step 16 B of filler | term u8
    [n_pad] | reward f32 [n_pad] | done u8 [n_pad] | 64 B of filler (rec_stride > the record).
    Padding lanes: done SET, reward NaN."""
    rng = np.random.default_rng(seed)
    NP = (N + 63) // 64 * 64
    offs = dict(term_off=16, reward_off=16 + NP, done_off=16 + 5 * NP, rec_stride=16 + 6 * NP + 64)
    reward = rng.normal(0, 30, (K, NP)).astype(np.float32)
    done = (rng.random((K, NP)) < density).astype(np.uint8)      # (density 1: every byte set, 0: none)
    term = rng.integers(0, 256, (K, NP)).astype(np.uint8)
    reward[:, N:] = np.nan
    done[:, N:] = 1
    rec = (rng.integers(0, 256, (K, offs["rec_stride"])).astype(np.uint8) if filler
           else np.zeros((K, offs["rec_stride"]), np.uint8))
    rec[:, offs["term_off"]: offs["term_off"] + NP] = term
    rec[:, offs["reward_off"]: offs["reward_off"] + 4 * NP] = reward.view(np.uint8)
    rec[:, offs["done_off"]: offs["done_off"] + NP] = done
    return NP, offs, reward, done, term, rec


def _raw_update(lib, dev, N, NP, offs, rec_dev, K, step0, carry, log, cap, env_base=0):
    from sacenv import _lib
    s = _lib.EpisodeScan(n_envs=N, n_pad=NP, n_steps=K, env_base=env_base, step0=step0, cap=cap, **offs)
    need = ctypes.c_int64()
    assert lib.sacenv_episodes_scratch_bytes(ctypes.byref(s), ctypes.byref(need)) == 0
    scratch = torch.empty(need.value, dtype=torch.uint8, device=dev)
    rc = lib.sacenv_episodes_update(ctypes.byref(s), rec_dev.data_ptr(), carry.data_ptr(), log.data_ptr(),
                                    scratch.data_ptr(), need.value, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize(dev)


def _read_log(log, cap):
    raw = log.cpu().numpy()
    total = int(raw[:8].view(np.int64)[0])
    return total, raw[32: 32 + 32 * min(total, cap)].view(ENTRY)


# The last two shapes are there for the scan launch: a workgroup scans tiles of 2 048 (step,
# wave) counts, at most 128 workgroups. 40 x 4 096 / 64 = 2 560 counts make two workgroups (the
# second sums the first's range before its own); 260 x 65 536 / 64 = 266 240 counts make 130
# tiles, so each workgroup walks two tiles with a running sum (few endings there, to keep
# the numpy restatement quick).
@pytest.mark.parametrize("N,K,density", [(1, 1, 0.5), (65, 130, 0.5), (200, 7, 0.5), (64, 64, 1), (64, 64, 0),
                                         (4096 - 3, 40, 0.5), (65536, 260, 0.001)])
def test_synthetic_records(gpu, built_lib, N, K, density):
    NP, offs, reward, done, term, rec = _synthetic(N, K, density, seed=N * 1000 + K, filler=N * K < 1 << 20)
    want, wscore, wlen = numpy_scan(reward, done, term, N, step0=1000, env_base=7)
    cap = int(done[:, :N].sum()) + 8
    rec_dev = torch.from_numpy(rec).to(gpu)
    carry = torch.zeros(12 * NP, dtype=torch.uint8, device=gpu)
    log = torch.zeros(32 + 32 * cap, dtype=torch.uint8, device=gpu)
    _raw_update(built_lib, gpu, N, NP, offs, rec_dev, K, 1000, carry, log, cap, env_base=7)
    total, got = _read_log(log, cap)
    assert total == len(want) == int(done[:, :N].sum())
    assert_same_log(got, want)
    assert not got["reserved"].any()
    assert np.all(got["env"] < 7 + N)                       # no padding lane was logged
    assert np.all(np.isfinite(got["score"]))                # nor did its NaN reach a score
    order = np.lexsort((got["env"], got["end_step"]))
    np.testing.assert_array_equal(order, np.arange(len(got)))
    c = carry.cpu().numpy()
    np.testing.assert_array_equal(c[: 8 * NP].view(np.uint64)[:N], wscore.view(np.uint64))
    np.testing.assert_array_equal(c[8 * NP:].view(np.int32)[:N], wlen)
    assert not c[: 8 * NP].view(np.uint64)[N:].any() and not c[8 * NP:].view(np.int32)[N:].any()


def test_two_calls_equal_one(gpu, built_lib):
    """K split 50 + 80 (the carry and the log's total go from call to call) = one call of 130."""
    N, K = 65, 130
    NP, offs, reward, done, term, rec = _synthetic(N, K, 0.5, seed=N * 1000 + K)
    cap = N * K + 8
    rec_dev = torch.from_numpy(rec).to(gpu)
    logs, carries = [], []
    for parts in ((130,), (50, 80)):
        carry = torch.zeros(12 * NP, dtype=torch.uint8, device=gpu)
        log = torch.zeros(32 + 32 * cap, dtype=torch.uint8, device=gpu)
        k0 = 0
        for kn in parts:
            _raw_update(built_lib, gpu, N, NP, offs, rec_dev[k0:], kn, k0, carry, log, cap)
            k0 += kn
        logs.append(log.cpu().numpy().tobytes())
        carries.append(carry.cpu().numpy().tobytes())
    assert logs[0] == logs[1] and carries[0] == carries[1]
    want, _, _ = numpy_scan(reward, done, term, N)
    assert_same_log(np.frombuffer(logs[1], np.uint8)[32: 32 + 32 * len(want)].view(ENTRY), want)


# ---------------------------------------------------------------- 2. boat rollouts

N_BOAT, MAX_STEPS, STEPS = 200, 40, 96


def _actions():
    rng = np.random.default_rng(3)
    rows = []
    for _ in range(STEPS):
        draw = rng.uniform(-1, 1, N_BOAT)
        rows.append(np.where(np.arange(N_BOAT) % 4 == 3, draw, np.linspace(-1, 1, N_BOAT)).astype(np.float32))
    return np.stack(rows)


def _make_env(gpu):
    from sacenv import VecBoatEnv
    return VecBoatEnv({"base_settings": {"experiment": 6, "test_mode": 0}}, N_BOAT,
                      seeds=np.arange(N_BOAT, dtype=np.uint64) + 11, device=gpu, max_episode_steps=MAX_STEPS)


def _columns(env, records_host):
    """(reward f32, done u8, term u8) [K, n_pad] of host copies of boat records."""
    from sacenv import _lib
    NP = env.n_pad
    r = np.ascontiguousarray(records_host[:, _lib.REC_REWARD * NP: _lib.REC_DONE * NP]).view(np.float32)
    return r, records_host[:, _lib.REC_DONE * NP: _lib.REC_TERM * NP], records_host[:, _lib.REC_TERM * NP: 50 * NP]


def _rollout_run(gpu, actions, **log_kw):
    """Case 2's run: 96 steps as rollouts of 32 and 64 with log.update(records) after each.
    -> (env, log, records on the host [96, 50 n_pad], the log buffer's bytes before any drain)."""
    from sacenv.episodes import EpisodeLog
    env = _make_env(gpu)
    log = EpisodeLog(env, **log_kw)
    recs = []
    a = torch.from_numpy(actions).to(gpu)
    for k0, k1 in ((0, 32), (32, 96)):
        records, _ = env.rollout(a[k0:k1])
        log.update(records)
        recs.append(records)
    torch.cuda.synchronize(gpu)
    return env, log, np.concatenate([r.cpu().numpy() for r in recs]), log.log.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def oracle_run():
    """The same seeds and actions through the CPU oracle: per ended episode (end_step, env,
    length, term, the oracle's f64 ep_reward at the ending, sum of |reward| over the episode)."""
    actions = _actions()
    ora = OracleVecBoat(OracleConfig(experiment=6, test_mode=0), np.arange(N_BOAT, dtype=np.uint64) + 11,
                        max_episode_steps=MAX_STEPS)
    length = np.zeros(N_BOAT, np.int64)
    abs_sum = np.zeros(N_BOAT, np.float64)
    eps = []
    for k in range(STEPS):
        r = ora.step(actions[k])
        length += 1
        abs_sum += np.abs(r["reward"])
        for e in np.flatnonzero(r["done"]):
            eps.append((k, e, length[e], int(r["term"][e]), r["ep_reward"][e], abs_sum[e]))
            length[e], abs_sum[e] = 0, 0.0
    eps = np.array(eps, dtype=[("end_step", "<i8"), ("env", "<i4"), ("length", "<i4"), ("term", "<u4"),
                               ("ep_reward", "<f8"), ("abs_sum", "<f8")])
    # the run must exercise the log: several codes, many distinct end steps, many episodes
    assert len(np.unique(eps["term"])) >= 2
    assert len(np.unique(eps["end_step"])) >= 50
    assert len(eps) >= 700
    return actions, eps


@pytest.fixture(scope="module")
def case2(gpu, built_lib, oracle_run):
    actions, _ = oracle_run
    env, log, records, raw = _rollout_run(gpu, actions, capacity=4096)
    entries = full(log.drain())
    return dict(actions=actions, raw=raw, entries=entries,
                columns=_columns(env, records), dropped=log.dropped)


def _episode_abs_sum(reward, entries):
    """sum of |record reward| over each entry's episode (its last `length` steps)."""
    return np.array([np.abs(reward[s - L + 1: s + 1, e].astype(np.float64)).sum()
                     for s, e, L in zip(entries["end_step"], entries["env"], entries["length"])])


def test_rollout_log_equals_numpy_scan_of_the_records(case2):
    reward, done, term = case2["columns"]
    want, _, _ = numpy_scan(reward, done, term, N_BOAT)
    assert_same_log(case2["entries"], want)
    assert case2["dropped"] == 0
    assert int(np.frombuffer(case2["raw"][:8], np.int64)[0]) == len(want)


def test_rollout_log_against_the_oracle(case2, oracle_run):
    _, eps = oracle_run
    got = case2["entries"]
    print(f"episodes {len(eps)}, end steps {len(np.unique(eps['end_step']))}, "
          f"codes {dict(zip(*np.unique(eps['term'], return_counts=True)))}")
    assert len(got) == len(eps)
    for f in EXACT:
        np.testing.assert_array_equal(got[f], eps[f], err_msg=f)
    # 1e-5 per step's reward (the project's bar on the oracle parity) + the f32 rounding of
    # each record's reward, 2^-24 relative, summed over the episode with a factor 2 of slack
    tol = got["length"] * 1e-5 + 2.0 ** -23 * eps["abs_sum"]
    err = np.abs(got["score"] - eps["ep_reward"])
    print(f"score vs oracle: max err {err.max():.3e}, max err / tol {np.max(err / tol):.3f}")
    assert np.all(err <= tol)


# ---------------------------------------------------------------- 3. step loop, final_ep_reward

@pytest.fixture(scope="module")
def case3(gpu, built_lib, case2):
    """48 steps with env.step and log.update() each; per step the new entries are checked
    against the env's own final_ep_reward and the steps since each env's last restart."""
    from sacenv.episodes import EpisodeLog
    env = _make_env(gpu)
    log = EpisodeLog(env, capacity=4096)
    a = torch.from_numpy(case2["actions"]).to(gpu)
    since = np.zeros(N_BOAT, np.int64)
    abs_sum = np.zeros(N_BOAT, np.float64)
    parts = []
    for k in range(48):
        _, reward, done, info = env.step(a[k])
        log.update()
        new = full(log.drain())                   # (synchronises)
        d = done.cpu().numpy()
        since += 1
        abs_sum += np.abs(reward.cpu().numpy().astype(np.float64))
        ended = np.flatnonzero(d)
        np.testing.assert_array_equal(new["env"], ended)
        assert np.all(new["end_step"] == k)
        np.testing.assert_array_equal(new["length"], since[ended])
        fin = info["final_ep_reward"].cpu().numpy()[ended]
        assert np.all(np.abs(new["score"] - fin) <= 2.0 ** -23 * abs_sum[ended]), k
        since[ended], abs_sum[ended] = 0, 0.0
        parts.append(new)
    return np.concatenate(parts)


def test_step_loop_log_equals_the_rollouts(case2, case3):
    want = case2["entries"][case2["entries"]["end_step"] < 48]
    assert len(want) > 0
    assert case3.tobytes() == want.tobytes()


# ---------------------------------------------------------------- 4. attaching in mid-run

def test_attach_in_mid_run(gpu, built_lib, case2, case3):
    from sacenv.episodes import EpisodeLog
    env = _make_env(gpu)
    a = torch.from_numpy(case2["actions"]).to(gpu)
    for k in range(20):
        env.step(a[k])
    log = EpisodeLog(env, capacity=4096, step0=20)
    for k in range(20, 48):
        env.step(a[k])
        log.update()
    got = full(log.drain())
    want = case3[case3["end_step"] >= 20]
    assert len(want) > 0 and np.any(want["end_step"] - want["length"] + 1 < 20)   # some were in flight
    for f in EXACT:                                       # the FULL length among them
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    tol = 2.0 ** -23 * _episode_abs_sum(case2["columns"][0], want)
    assert np.all(np.abs(got["score"] - want["score"]) <= tol)
    # episodes that started after the attachment are summed from the records alone: bit-equal
    fresh = want["end_step"] - want["length"] + 1 >= 20
    np.testing.assert_array_equal(got["score"][fresh].view(np.uint64), want["score"][fresh].view(np.uint64))


# ---------------------------------------------------------------- 5. overflow

def test_overflow_counts_and_writes_nothing_past_the_log(gpu, built_lib, case2):
    CAP, GUARD = 100, 4096
    buf = torch.full((32 + 32 * CAP + GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    env, log, records, raw = _rollout_run(gpu, case2["actions"], capacity=CAP, log_buffer=buf)
    everything = case2["entries"]
    assert int(np.frombuffer(raw[:8], np.int64)[0]) == len(everything)        # total counts them all
    got = full(log.drain())
    assert len(got) == CAP and log.dropped == len(everything) - CAP == 655
    assert got.tobytes() == everything[:CAP].tobytes()
    assert torch.all(buf[32 + 32 * CAP:] == 0xA5)
    # after the drain a further update appends from position 0
    score0 = log.carry_score.cpu().numpy()[:N_BOAT]
    len0 = log.carry_length.cpu().numpy()[:N_BOAT]
    more, _ = env.rollout(torch.zeros(40, N_BOAT, device=gpu))
    log.update(more)
    reward, done, term = _columns(env, more.cpu().numpy())
    want, _, _ = numpy_scan(reward, done, term, N_BOAT, step0=STEPS, score=score0, length=len0)
    got = full(log.drain())
    assert len(want) >= N_BOAT > CAP           # 40 more steps end every episode (max_episode_steps)
    assert log.dropped == len(want) - CAP
    assert_same_log(got, want[:CAP])
    assert torch.all(buf[32 + 32 * CAP:] == 0xA5)


# ---------------------------------------------------------------- 6. determinism

def test_log_bytes_are_the_same_run_to_run(gpu, built_lib, case2):
    """Case 2 again: the whole log buffer, header included, byte for byte."""
    _, _, _, raw = _rollout_run(gpu, case2["actions"], capacity=4096)
    assert raw == case2["raw"]


# ---------------------------------------------------------------- 7. toy env

def test_toy_env(gpu, built_lib):
    from sacenv.episodes import EpisodeLog
    from sacenv.toys import ParachuteEnv
    env = ParachuteEnv(num_envs=70, device=gpu, max_episode_steps=5)
    log = EpisodeLog(env)
    for _ in range(12):
        env.step()
        log.update()
    got = log.drain()
    assert len(got) == 140 and log.dropped == 0
    np.testing.assert_array_equal(got["end_step"], np.repeat([4, 9], 70))
    np.testing.assert_array_equal(got["env"], np.tile(np.arange(70), 2))
    assert np.all(got["length"] == 5) and np.all(got["term"] == 6)
    np.testing.assert_array_equal(got["score"].view(np.uint64), np.zeros(140, np.uint64))   # +0.0
    s = log.summary(lookback=10)
    assert s["episodes"] == 140 and s["terminations"]["truncated"] == 140 and s["avg_score"] == 0.0


# ---------------------------------------------------------------- 8. the example

def _example():
    spec = importlib.util.spec_from_file_location("train_vec_sac", os.path.join(ROOT, "examples", "train_vec_sac.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_reports_the_episodes_of_its_timed_loop(gpu, built_lib, monkeypatch):
    from sacenv import VecBoatEnv
    seen = []
    step = VecBoatEnv.step

    def counting_step(self, actions):
        out = step(self, actions)
        seen.append(int(out[2].sum().item()))
        return out

    monkeypatch.setattr(VecBoatEnv, "step", counting_step)
    out = _example().main(["--envs", "2048", "--iters", "20", "--episodes"])
    assert len(seen) == 25                                   # 5 warm-up iterations, then the timed 20
    ep = out["episodes"]
    print(f"done bytes per step {seen}, summary {ep}")
    assert ep["episodes"] == sum(seen[5:]) and ep["dropped"] == 0
    assert sum(ep["terminations"].values()) == ep["episodes"]
    plain = _example().main(["--envs", "2048", "--iters", "20"])
    assert set(plain) == {"pipeline", "agent", "envs", "iters", "env_steps_per_s", "ms_per_iter", "env_step_ms",
                          "losses"}
    assert set(out) == set(plain) | {"episodes"}
