"""The population scoreboard on the device (include/sacenv_scoreboard.h, sacenv/scoreboard.py).

The kernel cases write a log straight into a device buffer (header plus entries) and hold the
whole board, byte for byte, against the packed state of the Python restatement
(tests/scoreboard_oracle.py), which tests/test_scoreboard_cpu.py holds against the reference's
own lines. Sizes are the smallest at which the kernels take another path: a wave is 64 entries,
a workgroup loads 1 024 entries twice per round.
"""
import csv
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import scoreboard_oracle as so
from conftest import ROOT

pytestmark = pytest.mark.gpu

CALLS = (0, 1, 63, 64, 65, 1000)          # new entries per call: the wave's edges
LOOKBACKS = (1, 7, 8, 9, 50, 128)         # the n < 8 branch, the first full block, the cap


class Dev:
    """A log buffer and a board on the device, driven through the C entry points."""

    def __init__(self, gpu, lib, P, epm, L, cap, env_base=0, member_floats=0, slack=0):
        from sacenv import _lib
        from sacenv.episodes import ENTRY_DTYPE
        self._lib, self.lib, self.gpu, self.dtype = _lib, lib, gpu, ENTRY_DTYPE
        self.params = _lib.Board(members=P, envs_per_member=epm, env_base=env_base, lookback=L, cap=cap,
                                 member_floats=member_floats)
        need = ctypes.c_int64()
        _lib.check(lib.sacenv_board_bytes(ctypes.byref(self.params), ctypes.byref(need)))
        assert need.value == 32 + P * 128 + P * L * 8
        self.board = torch.full((need.value,), 0xAB, dtype=torch.uint8, device=gpu)     # init must write all of it
        self.log = torch.zeros(32 + 32 * (cap + slack), dtype=torch.uint8, device=gpu)
        _lib.check(lib.sacenv_board_init(ctypes.byref(self.params), self.board.data_ptr(), self._stream()))

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.gpu).cuda_stream)

    def write(self, total, entries, at=0):
        """Set the log's header to ``total`` and store ``entries`` from position ``at``."""
        raw = np.zeros(len(entries), self.dtype)
        if len(raw):
            for f in self.dtype.names:
                raw[f] = entries[f]
            self.log[32 + 32 * at: 32 + 32 * (at + len(raw))].copy_(torch.from_numpy(raw.view(np.uint8).copy()))
        self.log[:8].copy_(torch.from_numpy(np.array([total], "<i8").view(np.uint8)))

    def update(self, weights=None, snapshot=None):
        self._lib.check(self.lib.sacenv_board_update(
            ctypes.byref(self.params), self.log.data_ptr(), self.board.data_ptr(),
            None if weights is None else weights.data_ptr(), None if snapshot is None else snapshot.data_ptr(),
            self._stream()))

    def rewind(self):
        self._lib.check(self.lib.sacenv_board_rewind(ctypes.byref(self.params), self.board.data_ptr(),
                                                     self._stream()))

    def bytes(self):
        torch.cuda.synchronize(self.gpu)
        return self.board.cpu().numpy().tobytes()


def _entries(n, P, epm, L, family, seed, env_base=0, outside=True):
    """n log entries: the family's scores, ascending end steps, term codes 1..9 and envs over the
    members' range -- with ``outside`` also up to 3 envs below it and 3 at or above its end."""
    from sacenv.episodes import ENTRY_DTYPE
    rng = np.random.default_rng(seed)
    e = np.zeros(n, ENTRY_DTYPE)
    span = P * epm
    lo, hi = (max(env_base - 3, 0), env_base + span + 3) if outside else (env_base, env_base + span)
    e["env"] = rng.integers(lo, hi, n)
    e["end_step"] = np.cumsum(rng.integers(0, 3, n))
    e["term"] = rng.integers(1, 10, n)
    e["length"] = rng.integers(1, 500, n)
    # each member sees the family from its start, in its own order of arrival
    e["score"] = rng.uniform(-1, 1, n)
    owner = (e["env"].astype(np.int64) - env_base) // epm
    for m in range(P):
        mine = np.flatnonzero(owner == m)
        e["score"][mine] = so.scores(family, len(mine), L, seed + m)
    return e


def _diff(got: bytes, want: bytes, P, L) -> str:
    if got == want:
        return ""
    from sacenv.scoreboard import MEMBER_DTYPE
    out = [f"header {np.frombuffer(got[:32], '<i8')} != {np.frombuffer(want[:32], '<i8')}"]
    g, w = (np.frombuffer(b[32: 32 + 128 * P], MEMBER_DTYPE) for b in (got, want))
    for m in range(P):
        if g[m].tobytes() != w[m].tobytes():
            out.append(f"member {m}: {g[m]} != {w[m]}")
    gr, wr = (np.frombuffer(b[32 + 128 * P:], "<u8").reshape(P, L) for b in (got, want))
    out.append(f"ring slots that differ (member, slot): {np.argwhere(gr != wr)[:8].tolist()}")
    return "\n".join(out)


def _run_calls(gpu, lib, P, epm, L, family, calls, seed=0, env_base=0, outside=True):
    """The calls' entries appended one call at a time; the board against the oracle after each."""
    n = sum(calls)
    entries = _entries(n, P, epm, L, family, seed, env_base, outside)
    dev = Dev(gpu, lib, P, epm, L, cap=n + 8, env_base=env_base)
    ora = so.BoardOracle(P, epm, L, n + 8, env_base)
    assert dev.bytes() == ora.pack(), "the empty board"
    at = 0
    with np.errstate(all="ignore"):
        for c in calls:
            dev.write(at + c, entries[at: at + c], at)
            dev.update()
            ora.update(at + c, entries)
            at += c
            d = _diff(dev.bytes(), ora.pack(), P, L)
            assert not d, f"after the call that added {c} entries at {at - c}:\n{d}"
    return dev, ora, entries


@pytest.mark.parametrize("P,epm,L,family", [
    (P, epm, LOOKBACKS[(i + 2 * j) % 6], so.FAMILIES[(2 * i + j) % 6])
    for i, P in enumerate((1, 3, 16, 64)) for j, epm in enumerate((1, 64, 100))])
def test_members_and_envs_per_member(gpu, built_lib, P, epm, L, family):
    _, ora, _ = _run_calls(gpu, built_lib, P, epm, L, family, CALLS, seed=P + epm, env_base=5)
    assert all(m.episodes > 0 for m in ora.members)
    assert sum(m.episodes for m in ora.members) < sum(CALLS)    # (some entries are of envs outside the members)


@pytest.mark.parametrize("family", so.FAMILIES)
@pytest.mark.parametrize("L", LOOKBACKS)
def test_lookbacks_and_score_families(gpu, built_lib, L, family):
    _, ora, _ = _run_calls(gpu, built_lib, 3, 64, L, family, CALLS, seed=L)
    if family == "equal":
        assert all(m.saves == 0 for m in ora.members)
    if family in ("random", "ties") and L > 1:                 # (with L = 1 the mean is the score: never a save)
        assert all(m.saves > 0 for m in ora.members)


@pytest.mark.parametrize("P", (1, 16))
def test_round_edges(gpu, built_lib, P):
    """1 024 lanes load two entries each per round: calls that end one entry before, on and after a
    lane row and a round, and one of several rounds; with P = 1 the member owns every entry, so
    lanes judge two entries of a round and the 50-slot ring wraps many times inside a call."""
    _run_calls(gpu, built_lib, P, 64, 50, "random", (1023, 1, 1, 1023, 1, 2047, 2049, 5000), seed=3, outside=False)


def test_a_wave_of_one_member_and_a_wave_of_none(gpu, built_lib):
    """Waves (64 consecutive entries) that belong to one member entirely, to another, and to none."""
    P, epm, L = 3, 64, 9
    entries = _entries(64 * 6, P, epm, L, "random", 11, outside=False)
    rng = np.random.default_rng(5)
    for w, (lo, hi) in enumerate(((64, 128), (0, 64), (192, 300), (64, 128), (128, 192), (0, 192))):
        entries["env"][64 * w: 64 * (w + 1)] = rng.integers(lo, hi, 64)      # (192, 300): nobody's
    dev = Dev(gpu, built_lib, P, epm, L, cap=len(entries))
    ora = so.BoardOracle(P, epm, L, len(entries))
    for total in (128, len(entries)):
        dev.write(total, entries)
        dev.update()
        ora.update(total, entries)
        d = _diff(dev.bytes(), ora.pack(), P, L)
        assert not d, d
    assert [m.episodes for m in ora.members][:2] == [64 + sum(entries["env"][320:] < 64),
                                                     128 + sum((entries["env"][320:] >= 64) & (entries["env"][320:] < 128))]


def test_the_cursor_splits_nothing(gpu, built_lib):
    """The same 1 000 entries in one call and in calls of 1, 63, 64, 65 and the rest: the same
    bytes (but for the header's call count and the per-call saved_now). L = 7: each member's ring
    wraps inside a call and across calls."""
    from sacenv.scoreboard import MEMBER_DTYPE
    P, L = 3, 7
    one, ora1, _ = _run_calls(gpu, built_lib, P, 64, L, "random", (1000,), seed=9)
    many, ora2, _ = _run_calls(gpu, built_lib, P, 64, L, "random", (1, 63, 64, 65, 807), seed=9)
    assert min(m.episodes for m in ora1.members) > 40 * L

    def rest(b):
        b = bytearray(b)
        b[16:24] = bytes(8)                                            # calls
        for m in range(P):
            at = 32 + 128 * m + MEMBER_DTYPE.fields["saved_now"][1]
            b[at: at + 4] = bytes(4)
        return bytes(b)

    a, b = one.bytes(), many.bytes()
    assert np.frombuffer(a[:32], "<i8").tolist() == [1000, 0, 1, 0]
    assert np.frombuffer(b[:32], "<i8").tolist() == [1000, 0, 5, 0]
    assert rest(a) == rest(b)


def test_overflow_reads_nothing_past_cap(gpu, built_lib):
    """total = cap + 37: the 64 entries behind cap hold in-range envs with NaN scores and would
    show in every field; ``missed`` is 37, and a second call adds nothing."""
    P, epm, L, cap = 3, 64, 8, 200
    entries = _entries(cap, P, epm, L, "random", 4)
    poison = _entries(64, P, epm, L, "random", 5, outside=False)
    poison["score"] = np.nan
    poison["term"] = 7
    dev = Dev(gpu, built_lib, P, epm, L, cap, slack=64)
    ora = so.BoardOracle(P, epm, L, cap)
    dev.write(cap + 37, np.concatenate([entries, poison]))
    for calls in (1, 2):
        dev.update()
        ora.update(cap + 37, entries)
        got = dev.bytes()
        d = _diff(got, ora.pack(), P, L)
        assert not d, d
        assert np.frombuffer(got[:32], "<i8").tolist() == [cap + 37, 37, calls, 0]
    assert all(m.last == m.last for m in ora.members)
    # a header of garbage reads nothing past cap either, and nothing at all when it is negative
    for junk in (1 << 62, -5):
        dev.rewind()
        ora.rewind()
        dev.write(junk, [])
        dev.update()
        ora.update(junk, entries)
        d = _diff(dev.bytes(), ora.pack(), P, L)
        assert not d, (junk, d)
    assert ora.cursor == 0 and ora.missed == 37 + (1 << 62) - cap


def test_rewind_continues_the_histories(gpu, built_lib):
    P, epm, L = 3, 64, 9
    first = _entries(150, P, epm, L, "random", 6)
    second = _entries(90, P, epm, L, "ties", 7)
    dev = Dev(gpu, built_lib, P, epm, L, cap=256)
    ora = so.BoardOracle(P, epm, L, 256)
    dev.write(150, first)
    dev.update()
    ora.update(150, first)
    before = [m.episodes for m in ora.members]
    dev.write(0, [])                                   # the host empties the log ...
    dev.rewind()
    ora.rewind()
    dev.write(90, second)                              # ... and the scan refills it from the start
    dev.update()
    ora.update(90, second)
    d = _diff(dev.bytes(), ora.pack(), P, L)
    assert not d, d
    assert all(m.episodes > b > L for m, b in zip(ora.members, before))
    assert np.frombuffer(dev.bytes()[:32], "<i8").tolist() == [90, 0, 2, 0]


def _real_member_floats():
    from sacenv import _lib
    p = _lib.SacParams(obs_dim=11, n_actions=1, hidden=_lib.SAC_HIDDEN, batch=256, max_action=1.0, gamma=0.99,
                       tau=0.005, reward_scale=2.0, lr_actor=3e-4, lr_critic=3e-4, adam_beta1=0.9,
                       adam_beta2=0.999, adam_eps=1e-8)
    return int(_lib.sac_pop_layout(p, 3).member_floats)


def _three_calls(P=3, epm=64):
    """Call 1: members 0 and 2 save (a second episode above the first), member 1 does not; call 2:
    nobody saves; call 3: member 1 alone."""
    from sacenv.episodes import ENTRY_DTYPE
    rows = [[(0, 1.0), (64, 2.0), (128, 1.0), (0, 2.0), (64, 1.0), (128, 3.0)],
            [(0, 0.5), (64, 0.25), (128, -1.0)],
            [(64, 9.0), (0, -2.0)]]
    out, step = [], 0
    for call in rows:
        e = np.zeros(len(call), ENTRY_DTYPE)
        for i, (env, score) in enumerate(call):
            step += 1
            e[i] = (step, score, env + i % epm // 2, 7, 5)
        out.append(e)
    return out


# one vector; a workgroup's share and one more; one group of four vectors past the clamp of 64
# workgroups of 256 lanes with four loads each (the unrolled loop once, then the tail in four
# lanes); the real slab
@pytest.mark.parametrize("member_floats", (4, 1028, 4 * (256 * 4 * 64 + 4), None))
def test_snapshot_copies_the_members_that_saved(gpu, built_lib, member_floats):
    P, L = 3, 50
    mf = _real_member_floats() if member_floats is None else member_floats
    runs = []
    for _ in range(2):                                                   # twice: the same bytes run to run
        g = torch.Generator(device=gpu).manual_seed(3)
        weights = torch.randn((P, mf), device=gpu, generator=g)
        snap = torch.full((P, mf), 7.25, device=gpu)
        dev = Dev(gpu, built_lib, P, 64, L, cap=64, member_floats=mf)
        ora = so.BoardOracle(P, 64, L, 64)
        all_entries = np.concatenate(_three_calls())
        at, saved = 0, []
        for call in _three_calls():
            dev.write(at + len(call), call, at)
            at += len(call)
            before = snap.clone()
            dev.update(weights, snap)
            saved.append(ora.update(at, all_entries))
            d = _diff(dev.bytes(), ora.pack(), P, L)
            assert not d, d
            for m in range(P):
                want = weights[m] if m in saved[-1] else before[m]
                assert torch.equal(snap[m], want), (len(saved), m)
            weights += 1.0                                               # the live weights move on
        assert saved == [[0, 2], [], [1]]
        # without the two pointers the rule still runs and nothing is copied
        final = snap.clone()
        dev.update(None, None)
        torch.cuda.synchronize(gpu)
        assert torch.equal(snap, final)
        runs.append((dev.bytes(), snap.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]


def test_board_bytes_are_the_same_run_to_run(gpu, built_lib):
    a = _run_calls(gpu, built_lib, 16, 64, 50, "random", (5000, 1000), seed=8)[0].bytes()
    b = _run_calls(gpu, built_lib, 16, 64, 50, "random", (5000, 1000), seed=8)[0].bytes()
    assert a == b


# ---- with the real pieces

P_REAL, N_REAL, ITERS, LOOKBACK = 2, 64, 40, 5


def _post_hoc(entries, P, N, L):
    """The example's table, from drained entries."""
    owner = entries["env"] // N
    rows = []
    for m in range(P):
        scores = entries["score"][owner == m]
        rows.append({"episodes": int(scores.size), "score": float(scores[-1]), "best_score": float(scores.max()),
                     "avg_score": float(np.mean(scores[-L:]))})
    return rows


def test_with_env_population_and_log(gpu, built_lib):
    """The loop of examples/train_population.py: 2 members x 64 envs with 7-step episodes, 40
    iterations, a drain in the middle."""
    from sacenv import MemberScoreboard, NativeSACPopulation, PopulationReplay, VecBoatEnv, sample_hpsets
    from sacenv.agent import AgentConfig
    from sacenv.episodes import ENTRY_DTYPE, EpisodeLog
    P, N = P_REAL, N_REAL
    torch.manual_seed(77)
    configs = sample_hpsets(P, 0, base=AgentConfig(batch_size=256, max_size=1 << 14))
    replay = PopulationReplay(P, configs[0].max_size, (11,), 1, device=gpu, seeds=list(range(P)))
    pop = NativeSACPopulation(gpu, configs, init_seeds=list(range(P)), replay=replay)
    env = VecBoatEnv({"base_settings": {"experiment": 6, "test_mode": 0}}, P * N, seed=0, device=gpu,
                     max_episode_steps=7)
    obs = env.reset().clone()
    log = EpisodeLog(env, capacity=4096)
    board = MemberScoreboard(log, P, N, lookback=LOOKBACK, population=pop)
    assert board.best_member() is None and log.watchers == [board]
    with pytest.raises(RuntimeError, match="never saved"):
        board.snapshot_member(0)
    ora = so.BoardOracle(P, N, LOOKBACK, log.capacity)
    kept, kept_at, drained = {}, {}, []
    for it in range(ITERS):
        a = pop.choose_action(obs.view(P, N, -1))
        env.step(a.view(-1))
        log.update()
        replay.store_env_step(obs, a, env)
        obs = env.obs.clone()
        pop.learn(losses=False)
        board.update()
        torch.cuda.synchronize(gpu)
        total = int(log._total.item())
        entries = log.log[32: 32 + 32 * total].cpu().numpy().view(ENTRY_DTYPE)
        for m in ora.update(total, entries):                  # the members the rule selects in this iteration
            kept[m], kept_at[m] = pop.weights[m].clone(), it
        if it == ITERS // 2:
            drained.append(log.drain().copy())
            ora.update(total, entries)                        # (drain updates its watchers first: nothing new)
            ora.rewind()
    assert pop.adam_step > 30 and set(kept) == {0, 1}
    got = board.raw()
    d = _diff(got, ora.pack(), P, LOOKBACK)
    assert not d, d
    table = board.table()
    drained.append(log.drain().copy())
    entries = np.concatenate(drained)
    assert len(entries) >= 5 * P * N and len(drained[0]) and len(drained[1])
    want = _post_hoc(entries, P, N, LOOKBACK)
    for m in range(P):
        row = table[m]
        assert {k: row[k] for k in want[m]} == want[m], m
        assert row["saves"] == ora.members[m].saves > 0 and row["last_save_step"] == ora.members[m].last_save_step
        assert sum(row["terminations"].values()) == row["episodes"]
        assert {k: row[k] for k in pop.members[m].hpset()} == pop.members[m].hpset()
        assert torch.equal(board.snapshot[m], kept[m]), m
        if kept_at[m] < ITERS - 1:                                       # learning went on after the last save
            assert not torch.equal(board.snapshot[m], pop.weights[m])
        agent = board.snapshot_member(m)
        assert torch.equal(agent.weights, kept[m][: agent.weights.numel()])
        act = agent.choose_action(obs[m * N: (m + 1) * N])
        assert act.shape == (N, 1) and bool(torch.isfinite(act).all())
    assert board.table() == table                                        # the last drain changed nothing
    best = [r["best_score"] for r in table]
    assert board.best_member() == best.index(max(best))
    assert board.header()["missed"] == 0


def test_the_example_keeps_the_best(gpu, built_lib, tmp_path, monkeypatch, capsys):
    from sacenv import scoreboard
    from sacenv.sac_native import NativeSAC
    spec = importlib.util.spec_from_file_location("train_population",
                                                  os.path.join(ROOT, "examples", "train_population.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    boards = []
    save = scoreboard.MemberScoreboard.save_models
    monkeypatch.setattr(scoreboard.MemberScoreboard, "save_models",
                        lambda self, d: (boards.append(self), save(self, d))[1])
    out_dir = str(tmp_path / "search")
    torch.manual_seed(5)
    out = mod.main(["--members", "2", "--envs-per-member", "64", "--iters", "40", "--batch", "256",
                    "--max-episode-steps", "7", "--lookback", "5", "--keep-best", out_dir])
    printed = capsys.readouterr().out
    assert "on the device:" in printed
    board, = boards
    assert len(out["table"]) == len(out["device_table"]) == 2 and out["kept"] == [0, 1]
    for post, dev in zip(out["table"], out["device_table"]):
        assert post["episodes"] >= 5 * 64                        # 40 steps of episodes of at most 7
        for k in ("member", "episodes", "score", "best_score", "avg_score", "saves", "last_save_step",
                  "learning_rate_alpha", "learning_rate_beta", "gamma", "tvn_parameter_modulation_tau"):
            assert post[k] == dev[k], k
    with open(os.path.join(out_dir, "overview.csv"), newline="") as f:
        rows = list(csv.reader(f, delimiter=";"))
    assert [r[0] for r in rows] == ["member_0", "member_1"]
    assert [float(r[1]) for r in rows] == [r["best_score"] for r in out["device_table"]]
    for m in out["kept"]:
        snap = board.snapshot_member(m)
        loaded = NativeSAC(gpu, board.population.configs[m], with_memory=False)
        loaded.load_models(os.path.join(out_dir, f"member_{m}"))
        torch.cuda.synchronize(gpu)
        for net, sd in snap.state_dicts().items():
            for k, v in sd.items():
                assert torch.equal(loaded.state_dicts()[net][k], v), (m, net, k)
    # without the flag the output is as before
    plain = mod.main(["--members", "2", "--envs-per-member", "64", "--iters", "6", "--batch", "256"])
    assert "on the device:" not in capsys.readouterr().out
    assert not {"device_table", "kept", "best_member"} & set(plain) and set(plain) | {"device_table", "kept",
                                                                                      "best_member"} == set(out)
    assert set(plain["table"][0]) == set(out["table"][0]) - {"saves", "last_save_step"}


def _board_where_all_saved(gpu, built_lib):
    """A ``MemberScoreboard`` over a fresh population of three members, fed the entries of
    ``_three_calls`` through a log buffer written by hand (no env): every member saved its initial
    weights. Then one ``learn``: the live weights have moved on."""
    import types
    from sacenv import MemberScoreboard
    from test_sac_population_gpu import _population, _stacked
    P = 3
    pop = _population(gpu, P, 256, 11, noise_seeds=[5, 6, 7])
    dev = Dev(gpu, built_lib, P, 64, 5, cap=64)
    log = types.SimpleNamespace(device=gpu, env_base=0, capacity=64, watchers=[], log=dev.log, term_names=())
    board = MemberScoreboard(log, P, 64, lookback=5, population=pop)
    at = 0
    for call in _three_calls():
        dev.write(at + len(call), call, at)
        at += len(call)
        board.update()
    assert board.records()["saves"].tolist() == [1, 1, 1] and torch.equal(board.snapshot, pop.weights)
    _, batch, noise = _stacked(gpu, P, 256, 11, 1)
    pop.learn(batch, noise, losses=False)
    return pop, board


def test_saved_members_leave_the_generators_as_before(gpu, built_lib, tmp_path):
    """``snapshot_member`` builds one set of nets from torch's global CPU generator (and overwrites
    them), the first ``save_models`` one per member that saved, the second none: the views are
    kept (tests/test_sac_native_gpu.py: ``check_generators``)."""
    from test_sac_native_gpu import check_generators
    pop, board = _board_where_all_saved(gpu, built_lib)
    assert check_generators(gpu, 41, lambda: board.snapshot_member(1), pop.configs[1:2]) is not None
    for builds in (pop.configs, []):
        assert check_generators(gpu, 41, lambda: board.save_models(str(tmp_path)), builds) == [0, 1, 2]


def test_member_views_sit_on_the_snapshot(gpu, built_lib, tmp_path, monkeypatch):
    """The modules ``save_models`` writes from are ``SlabNets`` on ``board.snapshot[m]`` (no
    population stands behind them); the files load into a fresh ``NativeSAC`` whose weights are
    ``snapshot_member(m)``'s bit for bit; ``snapshot_member`` and ``export_member`` are both
    ``NativeSAC.from_slab``."""
    from sacenv.sac_native import NativeSAC, SlabNets
    pop, board = _board_where_all_saved(gpu, built_lib)
    calls = []
    real = NativeSAC.from_slab.__func__
    monkeypatch.setattr(NativeSAC, "from_slab",
                        classmethod(lambda cls, *a, **kw: (calls.append(cls), real(cls, *a, **kw))[1]))
    assert board.save_models(str(tmp_path)) == [0, 1, 2] and not calls
    esz = board.snapshot.element_size()
    off = pop.layout.net[2] + pop.layout.tensor[1][5]                   # critic_2's q.bias in a slab
    for m in range(3):
        snap, live = board.snapshot_member(m), pop.export_member(m)
        assert calls == [NativeSAC] * (3 * m + 2)                       # (a third at the end of each round)
        assert (snap.cfg, snap.noise_seed, snap.params.adam_eps) == (live.cfg, live.noise_seed, live.params.adam_eps)
        assert (snap.adam_step, snap.act_calls, live.adam_step, live.act_calls) == (0, 0, 1, 0)
        assert torch.equal(snap.weights, board.snapshot[m]) and torch.equal(live.weights, pop.weights[m])
        assert not torch.equal(snap.weights, live.weights)
        # the files: the snapshot's nets; a fresh agent has the snapshot's zero moments and, after
        # load_models' sync, its kernel copies
        loaded = NativeSAC(gpu, pop.configs[m], with_memory=False)
        loaded.load_models(str(tmp_path / f"member_{m}"))
        torch.cuda.synchronize(gpu)
        assert torch.equal(loaded.weights, snap.weights), m
        # the view: five modules whose parameters lie inside snapshot[m], and write through to it
        view = board._view(m)
        assert type(view) is SlabNets and board._view(m) is view and view.cfg == pop.configs[m]
        lo = board.snapshot[m].data_ptr()
        hi = lo + board.snapshot[m].numel() * esz
        for net in view.NETS:
            for p in getattr(view, net).parameters():
                assert lo <= p.data_ptr() and p.data_ptr() + p.numel() * esz <= hi, (m, net)
        assert view.critic_2.q.bias.data_ptr() == lo + off * esz
        with torch.no_grad():
            view.critic_2.q.bias.fill_(-3.5)
        assert float(board.snapshot[m, off]) == -3.5 and float(pop.weights[m, off]) != -3.5
        assert float(board.snapshot_member(m).weights[off]) == -3.5


