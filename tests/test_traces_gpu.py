"""Episode traces on the device (include/sacenv_traces.h, sacenv/traces.py).

The synthetic cases drive the C entry points through ctypes with hand-built record bytes, so
endings can be made dense, and hold the whole member buffer, byte for byte, against the numpy
restatement (tests/traces_oracle.py), which tests/test_traces_cpu.py holds against first
principles. Shapes are the smallest at which each mechanism can still go wrong: a wave is 64
envs, the walk takes 4 steps at a time, the store wraps after max_steps + call_steps steps.
The real-env cases run ``BestEpisodes`` beside an ``EpisodeLog``, a ``MemberScoreboard`` and a
``VecRecorder``.
"""
import csv
import ctypes
import importlib.util
import json
import math
import os
import struct

import numpy as np
import pytest
import torch

import traces_oracle as to
from conftest import ROOT

pytestmark = pytest.mark.gpu

FIELDS = ("obs", "reward", "done", "term", "final_obs", "actions")


class Dev:
    """A member buffer and a working store on the device, driven through the C entry points."""

    def __init__(self, gpu, lib, n, P, N, R, Kmax, env_base=0, step0=0, obs0=None, carry_score=None, carry_length=None):
        from sacenv import _lib
        self._lib, self.lib, self.gpu, self.n, self.P, self.R = _lib, lib, gpu, n, P, R
        self.n_pad = -(-n // 64) * 64
        self.params = _lib.Traces(n_envs=n, n_pad=self.n_pad, members=P, envs_per_member=N, env_base=env_base,
                                  max_steps=R, call_steps=Kmax, step0=step0)
        mb, sb = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(lib.sacenv_traces_bytes(ctypes.byref(self.params), ctypes.byref(mb), ctypes.byref(sb)))
        assert mb.value == P * to.member_bytes(R) and sb.value == to.store_bytes(self.n_pad, R, Kmax)
        self.members = torch.full((mb.value,), 0xAB, dtype=torch.uint8, device=gpu)    # init must write all of it
        self.store = torch.full((sb.value,), 0xCD, dtype=torch.uint8, device=gpu)      # and what it reads of this
        self.step = step0
        dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(gpu)  # noqa: E731
        self._attach = (dev(obs0, np.float32), dev(carry_score, np.float64), dev(carry_length, np.int32))
        ptr = [None if t is None else t.data_ptr() for t in self._attach]
        _lib.check(lib.sacenv_traces_init(ctypes.byref(self.params), *ptr, self.members.data_ptr(),
                                          self.store.data_ptr(), self._stream()))

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.gpu).cuda_stream)

    def upload(self, st, k0, K):
        """Steps k0 .. k0 + K - 1 as device tensors: records, actions, final_obs and the descriptor."""
        NP = self.n_pad
        rec = torch.from_numpy(to.pack_records(st, k0, K, NP)).to(self.gpu)
        act = torch.from_numpy(np.ascontiguousarray(st["actions"][k0: k0 + K])).to(self.gpu)
        fin = torch.from_numpy(to.pad_final(st, k0, K, NP)).to(self.gpu)
        s = self._lib.TraceSteps(n_steps=K, step=self.step, rec_stride=50 * NP if K > 1 else 0, obs_off=0,
                                 reward_off=44 * NP, done_off=48 * NP, term_off=49 * NP,
                                 final_stride=44 * NP if K > 1 else 0)
        return s, rec, act, fin

    def update(self, s, rec, act, fin):
        self._lib.check(self.lib.sacenv_traces_update(
            ctypes.byref(self.params), ctypes.byref(s), rec.data_ptr(), act.data_ptr(), fin.data_ptr(),
            self.members.data_ptr(), self.store.data_ptr(), self._stream()))
        self._keep = (rec, act, fin)

    def feed(self, st, k0, K):
        self.update(*self.upload(st, k0, K))
        self.step += K

    def bytes(self):
        torch.cuda.synchronize(self.gpu)
        return self.members.cpu().numpy().tobytes()


def _diff(got: bytes, ora, R) -> str:
    want = to.pack(ora.members(), R)
    if got == want:
        return ""
    out = []
    for m, (g, w) in enumerate(zip(to.split(got, ora.P, R), ora.members())):
        if g != w:
            rows = [i for i, (a, b) in enumerate(zip(g[1], w[1])) if a != b]
            out.append(f"member {m}: {to.describe(g)} != {to.describe(w)}; rows that differ: {rows[:8]}")
    return "\n".join(out) or "bytes past the kept rows differ"


def _run(gpu, lib, st, n, P, N, R, Ks, Kmax=None, check_every=1, **attach):
    """The steps of ``st`` fed in calls of ``Ks`` steps; the buffer against the oracle after every
    ``check_every``-th call and the last."""
    dev = Dev(gpu, lib, n, P, N, R, Kmax or max(Ks), **attach)
    ora = to.TraceOracle(n, P, N, R, **attach)
    assert dev.bytes() == to.pack(ora.members(), R), "the empty state"
    k0 = 0
    for c, K in enumerate(Ks):
        dev.feed(st, k0, K)
        ora.feed(*(st[f][k0: k0 + K] for f in FIELDS))
        k0 += K
        if c % check_every == check_every - 1 or c == len(Ks) - 1:
            d = _diff(dev.bytes(), ora, R)
            assert not d, f"after call {c} ({K} steps up to step {k0}):\n{d}"
    return dev, ora


def _headers(ora):
    return [struct.unpack(to.HEADER_FORMAT, h) for h, _ in ora.members()]


@pytest.mark.parametrize("K", [1, 5, 37])
@pytest.mark.parametrize("P", [1, 2, 3])
def test_calls_against_the_oracle(gpu, built_lib, P, K):
    """n_envs = 64 P, max_steps = 8, 40 calls of K steps: the global step passes several wraps
    of the store (8 + K slots), episodes span a wrap and some are longer than max_steps."""
    n, calls = 64 * P, 40
    st = to.synthetic_steps(K * calls, n, seed=10 * P + K, p_end=0.15)
    _, ora = _run(gpu, built_lib, st, n, P, 64, 8, [K] * calls, check_every=13, env_base=7, step0=1000)
    h = _headers(ora)
    assert all(x[5] > 0 for x in h)
    lengths = [x[3] for x in ora.endings()]
    assert max(lengths) > 8 and min(lengths) == 1


def test_a_partial_wave(gpu, built_lib):
    """n_envs = 70, one member: envs 64..69 are kept; the padding's done bytes are set and its
    lanes never end. Only envs 64..69 ever end, so the kept episode is one of theirs."""
    n = 70
    rng = np.random.default_rng(3)
    done = np.zeros((30, n), bool)
    done[:, 64:] = rng.random((30, 6)) < 0.3
    st = to.synthetic_steps(30, n, seed=3, done=done)
    _, ora = _run(gpu, built_lib, st, n, 1, 70, 8, [1, 5, 4, 7, 13])
    assert 64 <= _headers(ora)[0][2] < 70
    # with 64 envs per member the same envs belong to nobody
    dev, ora = _run(gpu, built_lib, st, n, 1, 64, 8, [1, 5, 4, 7, 13])
    assert dev.bytes() == to.EMPTY + bytes(9 * 64)


def test_envs_past_the_last_member_belong_to_nobody(gpu, built_lib):
    """members = 2 x 64 of 192 envs: the third wave's episodes score highest and are never kept."""
    n = 192
    st = to.synthetic_steps(24, n, seed=4, p_end=0.2)
    st["reward"][:, 128:] += 50
    _, ora = _run(gpu, built_lib, st, n, 2, 64, 8, [6, 6, 6, 6])
    assert [x[2] // 64 for x in _headers(ora)] == [0, 1]


def test_two_endings_of_one_env_in_one_call(gpu, built_lib):
    """Env 5 ends at steps 3 and 9 of one 12-step call and the earlier episode scores higher: it
    is the winner and its rows are its own, although the walk appended the later episode's steps
    before anything was copied."""
    n, T = 64, 12
    done = np.zeros((T, n), bool)
    done[3, 5] = done[9, 5] = True
    reward = np.zeros((T, n), np.float32)
    reward[:4, 5], reward[4:10, 5] = 2.0, 1.0
    st = to.synthetic_steps(T, n, seed=5, done=done, reward=reward)
    dev, ora = _run(gpu, built_lib, st, n, 1, 64, 8, [T])
    assert _headers(ora)[0] == (3, 8.0, 5, 4, int(st["term"][3, 5]), 5, 0, 0, 1)
    row0 = to.split(dev.bytes(), 1, 8)[0][1][0]
    assert row0 == to.pack_row(np.zeros(11), 0, 0)          # the obs at attachment (zeros here), not step 3's
    # the other way round the later one wins, at the same call's last-but-two step
    reward[4:10, 5] = 3.0
    st = to.synthetic_steps(T, n, seed=5, done=done, reward=reward)
    _, ora = _run(gpu, built_lib, st, n, 1, 64, 8, [T])
    assert _headers(ora)[0][:4] == (9, 18.0, 5, 6)


@pytest.mark.parametrize("K", [1, 4, 9])
def test_endings_at_a_calls_first_and_last_step(gpu, built_lib, K):
    """Two calls of K steps. In the first an episode of length 1 ends at the call's first step
    (rows = 2); in the second a better one ends at the call's last step."""
    n = 128
    done = np.zeros((2 * K, n), bool)
    reward = np.zeros((2 * K, n), np.float32)
    done[0, 70], reward[0, 70] = True, 1.5
    done[2 * K - 1, 3], reward[2 * K - 1, 3] = True, 2.5
    st = to.synthetic_steps(2 * K, n, seed=6, done=done, reward=reward)
    dev = Dev(gpu, built_lib, n, 1, 128, 8, K)
    ora = to.TraceOracle(n, 1, 128, 8)
    dev.feed(st, 0, K)
    ora.feed(*(st[f][:K] for f in FIELDS))
    assert not _diff(dev.bytes(), ora, 8)
    assert _headers(ora)[0] == (0, 1.5, 70, 1, int(st["term"][0, 70]), 2, 0, 0, 1)
    dev.feed(st, K, K)
    ora.feed(*(st[f][K:] for f in FIELDS))
    assert not _diff(dev.bytes(), ora, 8)
    assert _headers(ora)[0][:4] == (2 * K - 1, 2.5, 3, 2 * K) and _headers(ora)[0][8] == 2


def test_tie_rules(gpu, built_lib):
    """Ties within a call go to the smallest (end_step, env); a tie with the stored best replaces
    nothing; a NaN never wins; -inf loses to any finite score; an empty member takes any score
    that is not NaN."""
    n, K = 128, 6
    nan, inf = np.float32("nan"), np.float32("inf")

    def steps(ends, seed):
        """ends: {(step, env): score}: the ending step's reward is the score, every other +0.0"""
        done, reward = np.zeros((K, n), bool), np.zeros((K, n), np.float32)
        for (k, e), s in ends.items():
            done[k, e], reward[k, e] = True, s
        return to.synthetic_steps(K, n, seed=seed, done=done, reward=reward)

    calls = [
        # member 0: NaN only -> stays empty; member 1: -inf only -> an empty member takes it
        steps({(1, 3): nan, (2, 70): -inf, (4, 90): -inf}, 1),
        # member 0: a NaN and ties of 2.0 at (3, 9), (3, 5), (2, 40) -> (2, 40); member 1: -inf again -> nothing
        steps({(0, 1): nan, (3, 9): 2.0, (3, 5): 2.0, (2, 40): 2.0, (5, 100): -inf}, 2),
        # member 0: a tie with the stored 2.0 -> nothing; member 1: -7 beats -inf
        steps({(0, 0): 2.0, (1, 63): 2.0, (2, 127): -7.0}, 3),
        # member 0: 2.0 again and the next f64 above it written as f32 -> that one; member 1: +inf
        steps({(0, 2): 2.0, (4, 8): np.nextafter(np.float32(2.0), inf), (4, 7): 2.0, (3, 64): inf, (5, 65): inf}, 4)]
    dev = Dev(gpu, built_lib, n, 2, 64, 8, K)
    ora = to.TraceOracle(n, 2, 64, 8)
    want = [[(-1, -1, 0), (2, 70, 1)], [(8, 40, 1), (2, 70, 1)], [(8, 40, 1), (14, 127, 2)], [(22, 8, 2), (21, 64, 3)]]
    for c, st in enumerate(calls):
        before = dev.bytes()
        dev.feed(st, 0, K)
        ora.feed(*(st[f] for f in FIELDS))
        got = dev.bytes()
        assert not _diff(got, ora, 8), c
        assert [(h[0], h[2], h[8]) for h in _headers(ora)] == want[c], c
        mb = to.member_bytes(8)
        for m in range(2):      # a member whose best did not change was not touched
            if c and want[c][m] == want[c - 1][m]:
                assert got[m * mb: (m + 1) * mb] == before[m * mb: (m + 1) * mb]
    assert _headers(ora)[1][1] == float("inf") and _headers(ora)[0][1] == float(np.nextafter(np.float32(2.0), inf))


def test_truncation(gpu, built_lib):
    """L > max_steps gives first_row = L - max_steps and the last rows; an episode in flight at
    attachment, its carry seeded non-zero, gives its full score and length with first_row > 0."""
    n, R = 64, 8
    done = np.zeros((20, n), bool)
    done[12, 9] = True                          # 13 steps
    reward = np.zeros((20, n), np.float32)
    reward[:13, 9] = 0.25
    st = to.synthetic_steps(20, n, seed=8, done=done, reward=reward)
    _, ora = _run(gpu, built_lib, st, n, 1, 64, R, [5, 5, 5, 5])
    assert _headers(ora)[0] == (12, 3.25, 9, 13, int(st["term"][12, 9]), 9, 5, 0, 1)
    # attached in mid-episode: env 9 had taken 3 steps worth 2.5, env 10 none
    rng = np.random.default_rng(8)
    carry_len, carry = np.zeros(n, np.int32), np.zeros(n)
    carry_len[9], carry[9] = 3, 2.5
    done = np.zeros((6, n), bool)
    done[4, 9] = True
    reward = np.zeros((6, n), np.float32)
    reward[:5, 9] = 0.5
    st = to.synthetic_steps(6, n, seed=9, done=done, reward=reward)
    obs0 = rng.random((n, 11), np.float32)
    for Ks in ([6], [1] * 6):
        _, ora = _run(gpu, built_lib, st, n, 1, 64, R, Ks, step0=50, obs0=obs0, carry_score=carry, carry_length=carry_len)
        assert _headers(ora)[0] == (54, 5.0, 9, 8, int(st["term"][4, 9]), 5, 4, 0, 1)
    # and an env at an episode's first step at attachment keeps row 0: the obs at attachment
    done[4, 9], done[2, 10] = False, True
    reward[:3, 10] = 1.0
    st = to.synthetic_steps(6, n, seed=9, done=done, reward=reward)
    dev, ora = _run(gpu, built_lib, st, n, 1, 64, R, [6], step0=50, obs0=obs0, carry_score=carry, carry_length=carry_len)
    assert _headers(ora)[0][:7] == (52, 3.0, 10, 3, int(st["term"][2, 10]), 4, 0)
    assert to.split(dev.bytes(), 1, R)[0][1][0] == to.pack_row(obs0[10], 0, 0)


def test_split_invariance_and_run_to_run(gpu, built_lib):
    """The same 74 steps as K = 1 calls, as K = 37 calls and as K = 37 calls again: byte-equal
    member buffers."""
    n, P, R, T = 192, 3, 8, 74
    st = to.synthetic_steps(T, n, seed=11, p_end=0.15)
    one, ora = _run(gpu, built_lib, st, n, P, 64, R, [1] * T, Kmax=37, check_every=T, step0=5)
    many, _ = _run(gpu, built_lib, st, n, P, 64, R, [37, 37], step0=5)
    again, _ = _run(gpu, built_lib, st, n, P, 64, R, [37, 37], step0=5)
    assert one.bytes() == many.bytes() == again.bytes()
    assert any(x[8] > 1 for x in _headers(ora))             # (a best was replaced along the way)


def test_a_captured_update(gpu, built_lib):
    """Three updates captured into one graph and replayed equal the eager result."""
    n, P, R, K = 128, 2, 8, 5
    st = to.synthetic_steps(3 * K, n, seed=12, p_end=0.2)
    eager, ora = _run(gpu, built_lib, st, n, P, 64, R, [K] * 3)
    dev = Dev(gpu, built_lib, n, P, 64, R, K)
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream(gpu)
    with torch.cuda.stream(stream):
        ups = []
        for c in range(3):
            ups.append(dev.upload(st, c * K, K))
            dev.step += K
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            for up in ups:
                dev.update(*up)
    empty = to.pack(to.TraceOracle(n, P, 64, R).members(), R)
    assert dev.bytes() == empty                              # capturing ran nothing
    graph.replay()
    assert dev.bytes() == eager.bytes() and not _diff(dev.bytes(), ora, R)


# ---- the real env

P_REAL, N_REAL, T_REAL, MAX_STEPS = 2, 64, 300, 40


def _real_env(gpu):
    from sacenv import VecBoatEnv
    env = VecBoatEnv({"base_settings": {"experiment": 6, "test_mode": 0}}, P_REAL * N_REAL, seed=0, device=gpu,
                     max_episode_steps=MAX_STEPS)
    env.reset()
    return env


def _real_actions(gpu, T=T_REAL):
    rng = np.random.default_rng(21)
    return torch.from_numpy(rng.uniform(-1, 1, (T, P_REAL * N_REAL)).astype(np.float32)).to(gpu)


@pytest.fixture(scope="module")
def real_run(gpu, built_lib):
    """300 steps through ``step()`` with a ``BestEpisodes``, an ``EpisodeLog`` and a ``MemberScoreboard``
    beside it, and the test's own copy of every step; shared, never changed."""
    from sacenv import BestEpisodes, MemberScoreboard
    from sacenv.episodes import EpisodeLog
    env = _real_env(gpu)
    n = env.num_envs
    log = EpisodeLog(env)
    board = MemberScoreboard(log, P_REAL, N_REAL, lookback=50)
    traces = BestEpisodes(env, members=P_REAL, envs_per_member=N_REAL)
    assert traces.R == MAX_STEPS and traces.nbytes == traces.members.numel() + traces.store.numel()
    acts = _real_actions(gpu)
    obs0 = env.obs.clone()
    obs = torch.empty((T_REAL, n, 11), dtype=torch.float32, device=gpu)
    final = torch.empty_like(obs)
    reward = torch.empty((T_REAL, n), dtype=torch.float32, device=gpu)
    done = torch.empty((T_REAL, n), dtype=torch.uint8, device=gpu)
    for k in range(T_REAL):
        o, r, d, info = env.step(acts[k])
        log.update()
        board.update()
        traces.update(acts[k])
        obs[k], final[k], reward[k], done[k] = o, info["final_obs"], r, d
    raw = traces.raw()
    best = board.records()["best"].copy()
    entries = log.drain().copy()
    return {"traces": traces, "raw": raw, "entries": entries, "board_best": best, "obs0": obs0.cpu().numpy(),
            "obs": obs.cpu().numpy(), "final": final.cpu().numpy(), "reward": reward.cpu().numpy(),
            "done": done.cpu().numpy(), "actions": acts.cpu().numpy()}


def test_real_env_against_the_log_and_the_board(real_run):
    """Each member's kept score, env and end_step are the first maximal entry of the drained log,
    bit for bit; the score is the board's best; every row is the test's own copy of that step,
    row 0 the reset obs."""
    r = real_run
    heads = r["traces"].headers()
    ent = r["entries"]
    for m in range(P_REAL):
        mine = ent[ent["env"] // N_REAL == m]
        assert len(mine) > N_REAL
        first = mine[np.flatnonzero(mine["score"] == mine["score"].max())[0]]
        h = heads[m]
        assert h["score"].tobytes() == first["score"].tobytes() == r["board_best"][m].tobytes()
        assert (h["env"], h["end_step"], h["length"], h["term"]) == \
            (first["env"], first["end_step"], first["length"], first["term"])
        b = r["traces"].best(m)
        t, L, e = b["end_step"], b["length"], b["env"]
        assert b["rows"] == L + 1 and b["first_row"] == 0 and b["replaced"] >= 1
        start = r["obs0"][e] if t - L < 0 else r["obs"][t - L, e]
        assert np.array_equal(b["obs"][0], start) and b["action"][0] == 0 and b["reward"][0] == 0
        for j in range(1, L):
            k = t - L + j
            assert np.array_equal(b["obs"][j], r["obs"][k, e]), j
            assert (b["action"][j], b["reward"][j]) == (r["actions"][k, e], r["reward"][k, e]), j
        assert np.array_equal(b["obs"][L], r["final"][t, e])
        assert (b["action"][L], b["reward"][L]) == (r["actions"][t, e], r["reward"][t, e])
        assert r["done"][t, e] and not r["done"][t - L + 1: t, e].any()
    table = r["traces"].table()
    assert [row["member"] for row in table] == [0, 1] and all(row["term"] in r["traces"].term_names for row in table)


def test_real_env_through_rollout(gpu, real_run):
    """The same 300 steps through ``rollout`` in chunks of 37 (call_steps = 37): byte-equal buffers."""
    from sacenv import BestEpisodes
    env = _real_env(gpu)
    traces = BestEpisodes(env, members=P_REAL, envs_per_member=N_REAL, call_steps=37)
    acts = _real_actions(gpu)
    final = torch.empty((37, env.n_pad, 11), dtype=torch.float32, device=gpu)
    for k0 in range(0, T_REAL, 37):
        a = acts[k0: k0 + 37].contiguous()
        K = a.shape[0]
        records, _ = env.rollout(a, final_obs=final)
        traces.update(a, records, final, n_steps=K)
    assert traces.step0 == T_REAL
    assert traces.raw() == real_run["raw"]
    with pytest.raises(ValueError, match="call_steps"):
        traces.update(acts[:38].contiguous(), torch.empty((38, 50 * env.n_pad), dtype=torch.uint8, device=gpu),
                      torch.empty((38, env.n_pad, 11), dtype=torch.float32, device=gpu))
    with pytest.raises(ValueError, match="final_obs is required"):
        traces.update(acts[:2].contiguous(), torch.empty((2, 50 * env.n_pad), dtype=torch.uint8, device=gpu))


def test_constructor_refusals(gpu, built_lib):
    from sacenv import BestEpisodes, VecBoatEnv
    cfg = {"base_settings": {"experiment": 6, "test_mode": 0}}
    with pytest.raises(ValueError, match="autoreset"):
        BestEpisodes(VecBoatEnv(cfg, 64, device=gpu, autoreset=False), members=1, envs_per_member=64, max_steps=8)
    env = VecBoatEnv(cfg, 64, device=gpu)
    with pytest.raises(ValueError, match="max_steps is required"):
        BestEpisodes(env, members=1, envs_per_member=64)
    with pytest.raises(ValueError, match=str(to.store_bytes(64, 500, 1))):
        BestEpisodes(env, members=1, envs_per_member=64, max_steps=500, max_bytes=1 << 20)
    with pytest.raises(ValueError):       # (the C side's refusal: a wave would straddle two members)
        BestEpisodes(VecBoatEnv(cfg, 128, device=gpu), members=2, envs_per_member=32, max_steps=8)


BOUNDS = {"boat_position_x": None, "boat_position_y": None, "boat_velocity_x": (0, 5), "boat_velocity_y": (0, 2),
          "boat_angle": (0, 2 * math.pi), "reward": (0, 0), "rudder_angle": (-math.pi / 3, math.pi / 3)}


def test_save_csv_against_the_recorder(gpu, real_run, tmp_path):
    """Member 0's best episode as ``save_csv`` writes it, against ``VecRecorder`` on the env that
    hosted it in a second run from the same seeds: the same columns and row count, action_rudder
    and n equal, every other value v within 4 * 2^-24 * (|v| + |min| + (max - min)) of the
    recorder's f64, min and max the column's normalisation bounds (one f32 rounding of the
    normalised value times the range; the factor 4 covers the denormalising arithmetic).

    Row 0 of an episode that is not its env's first: the reference's ``reset`` leaves
    ``BoatEnv.action`` and ``.reward`` as the episode before left them, which the recorder
    reproduces, while a kept episode's row 0 carries ``BoatEnv.__init__``'s zeros by contract;
    there these two columns are held to 0 and everything else to the recorder."""
    from sacenv.recorder import COLUMNS, VecRecorder
    r = real_run
    b = r["traces"].best(0)
    t, L, e = b["end_step"], b["length"], b["env"]
    number = int(r["done"][: t - L + 1, e].sum())             # the env's episodes that ended before this one began
    out = tmp_path / "traces"
    assert r["traces"].save_csv(str(out)) == [0, 1]
    env = _real_env(gpu)
    acts = _real_actions(gpu)
    rec = VecRecorder(env, [e], str(tmp_path / "rec"), flush_steps=T_REAL + 1)
    for k in range(t + 1):
        rec.record()
        env.step(acts[k])
        rec.after_step(acts[k])
    rec.close()

    def read(path):
        with open(path) as f:
            rows = list(csv.reader(f, delimiter=";"))
        return rows[0], rows[1:]

    head, mine = read(out / "member_0" / "episodes" / "episode_0_data.csv")
    head2, theirs = read(tmp_path / "rec" / "episodes" / f"env_{e}" / f"episode_{number}_data.csv")
    assert tuple(head) == tuple(head2) == COLUMNS
    assert len(mine) == len(theirs) == L
    cfg = env.cfg
    bounds = dict(BOUNDS, boat_position_x=(0, float(cfg.goal_line)),
                  boat_position_y=(-float(cfg.track_width), float(cfg.track_width)))
    for i, (a, c) in enumerate(zip(mine, theirs)):
        for col, x, y in zip(COLUMNS, a, c):
            if i == 0 and number > 0 and col in ("action_rudder", "reward"):
                assert float(x) == 0.0, (col, x)
            elif col in ("action_rudder", "n"):
                assert x == y, (i, col, x, y)
            else:
                lo, hi = bounds[col]
                v = float(y)
                print(f"row {i} {col}: {float(x)!r} vs {v!r}")
                assert abs(float(x) - v) <= 4 * 2.0 ** -24 * (abs(v) + abs(lo) + (hi - lo)), (i, col, x, y)
    info_head, info = read(out / "member_0" / "episodes" / "info.csv")
    assert info_head[0] == "termination" and info[0][0] == b["term"] and float(info[0][-1]) == b["score"]


def _example():
    spec = importlib.util.spec_from_file_location("train_population",
                                                  os.path.join(ROOT, "examples", "train_population.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_example_keeps_traces(gpu, built_lib, tmp_path, capsys, monkeypatch):
    """``--keep-traces DIR``: the table is printed, each member's CSV has as many rows as its
    printed length, and the JSON line's ``traces`` is ``table()``; without the flag the JSON line
    has the keys it had before."""
    from sacenv import traces as tr
    kept = []
    save = tr.BestEpisodes.save_csv
    monkeypatch.setattr(tr.BestEpisodes, "save_csv", lambda self, d: (kept.append(self), save(self, d))[1])
    args = ["--members", "2", "--envs-per-member", "64", "--iters", "60", "--batch", "256", "--max-episode-steps", "20"]
    out_dir = tmp_path / "best"
    torch.manual_seed(5)
    out = _example().main(args + ["--keep-traces", str(out_dir)])
    printed = capsys.readouterr().out
    assert "best episodes:" in printed
    keeper, = kept
    line = json.loads(printed.strip().split("\n")[-1])
    assert line["traces"] == out["traces"] == keeper.table() and len(out["traces"]) == 2
    for row in out["traces"]:
        assert row["rows"] == row["length"] + 1 and row["first_row"] == 0
        with open(out_dir / f"member_{row['member']}" / "episodes" / "episode_0_data.csv") as f:
            assert len(f.readlines()) == 1 + row["length"]
        assert f"{row['member']:>6} {row['score']:12.2f}" in printed
    torch.manual_seed(5)
    plain = _example().main(args)
    assert list(plain) == ["pipeline", "replay", "noise", "members", "envs_per_member", "iters", "batch",
                           "env_steps_per_s", "ms_per_iter", "losses", "table"]
    assert "best episodes" not in capsys.readouterr().out
