"""Population selection on the device (include/sacenv_selection.h, sacenv/selection.py).

The kernel cases write a board straight into a device buffer (each member's ``episodes`` and
``avg``), drive the C entry points and hold the whole selection state, byte for byte, against the
packed state of the numpy restatement (tests/selection_oracle.py), which
tests/test_selection_cpu.py holds to first principles. The slab carries a member-coded bit
pattern with a guard region behind it: after every call each loser's slab is its source's bytes
and every other byte -- the other slabs, the guard, the board -- is as before. Sizes are the
smallest at which the kernels take another path: a wave is 64 members, a copy workgroup moves
``COPY_THREADS x COPY_UNROLL`` 16-B vectors per pass.
"""
import ctypes
import dataclasses
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

import selection_oracle as sel
from conftest import ROOT

pytestmark = pytest.mark.gpu

E_NULL, E_SIZE, E_RANGE = -1, -4, -5
GUARD = 256                                   # floats behind the slabs, bytes behind the state
MIN_EPISODES, LOOKBACK = 4, 7
PQ = sorted({(P, q) for P in (2, 3, 5, 63, 64) for q in (1, P // 2)})


def _share():
    """Floats one copy workgroup moves per pass, from the copy kernel's own constants."""
    from sacenv import _lib
    return 4 * _lib.SELECT_COPY_THREADS * _lib.SELECT_COPY_UNROLL


def _real_member_floats(P=4):
    from sacenv import _lib
    p = _lib.SacParams(obs_dim=11, n_actions=1, hidden=_lib.SAC_HIDDEN, batch=256, max_action=1.0, gamma=0.99,
                       tau=0.005, reward_scale=2.0, lr_actor=3e-4, lr_critic=3e-4, adam_beta1=0.9,
                       adam_beta2=0.999, adam_eps=1e-8)
    return int(_lib.sac_pop_layout(p, P).member_floats)


def _hp(P, seed=0):
    rng = np.random.default_rng(seed)
    return [[float(rng.uniform(lo, hi)) for lo, hi in zip(sel.DEFAULT_LO, sel.DEFAULT_HI)] for _ in range(P)]


class Dev:
    """A hand-written board, a selection state and a slab on the device, driven through the C
    entry points."""

    def __init__(self, gpu, lib, P, q, mf, hp, seed=0, min_episodes=MIN_EPISODES, L=LOOKBACK, **kw):
        from sacenv import _lib
        from sacenv.scoreboard import MEMBER_DTYPE
        self._lib, self.lib, self.gpu, self.P, self.mf, self.L = _lib, lib, gpu, P, mf, L
        self.member_dtype = MEMBER_DTYPE
        fields = dict(members=P, quantile=q, lookback=L, reserved=0, min_episodes=min_episodes, member_floats=mf,
                      seed=seed, factor=(0.8, 1.2), lo=sel.DEFAULT_LO, hi=sel.DEFAULT_HI)
        fields.update(kw)
        for name, n in (("factor", 2), ("lo", 4), ("hi", 4)):
            fields[name] = (ctypes.c_double * n)(*fields[name])
        self.params = _lib.Select(**fields)
        need = ctypes.c_int64()
        _lib.check(lib.sacenv_select_bytes(ctypes.byref(self.params), ctypes.byref(need)))
        assert need.value == 32 + 64 * P
        self.state_bytes = need.value
        self.state = torch.full((need.value + GUARD,), 0xAB, dtype=torch.uint8, device=gpu)   # init writes all of it
        self.board = torch.zeros(32 + P * 128 + P * L * 8, dtype=torch.uint8, device=gpu)
        # member m's float i holds the bits (m + 1) << 24 | i; the guard holds 0x7Fxxxxxx
        bits = ((np.arange(P, dtype=np.int64)[:, None] + 1) << 24 | (np.arange(mf, dtype=np.int64)[None, :] & 0xFFFFFF))
        flat = np.concatenate([bits.reshape(-1), 0x7F000000 | np.arange(GUARD, dtype=np.int64)]).astype(np.int32)
        self.slab = torch.from_numpy(flat).to(gpu)
        self.hp0 = (_lib.SacMember * P)(*[_lib.SacMember(*row, 2.0) for row in hp])
        _lib.check(lib.sacenv_select_init(ctypes.byref(self.params), self.hp0, self.state.data_ptr(), self._stream()))

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.gpu).cuda_stream)

    def write_board(self, episodes, avg, seed=0):
        """A board whose members have these ``episodes`` and ``avg``; every other field, the header
        and the rings hold noise (the selection reads none of it)."""
        P, L = self.P, self.L
        rng = np.random.default_rng(seed)
        raw = rng.integers(0, 256, 32 + P * 128 + P * L * 8, dtype=np.uint8)
        rec = raw[32: 32 + P * 128].view(self.member_dtype)
        rec["episodes"] = episodes
        rec["avg"] = avg
        self.board.copy_(torch.from_numpy(raw))
        return raw.tobytes()

    def step(self):
        return self.lib.sacenv_select_step(ctypes.byref(self.params), self.board.data_ptr(), self.state.data_ptr(),
                                           self.slab.data_ptr(), self._stream())

    def read(self):
        """(state bytes, state guard bytes, slab + guard as int32, board bytes)."""
        torch.cuda.synchronize(self.gpu)
        st = self.state.cpu().numpy().tobytes()
        return st[: self.state_bytes], st[self.state_bytes:], self.slab.cpu().numpy(), self.board.cpu().numpy().tobytes()


def _diff(got: bytes, want: bytes, P) -> str:
    if got == want:
        return ""
    from sacenv.selection import STATE_DTYPE
    out = [f"header {np.frombuffer(got[:32], '<i8')} != {np.frombuffer(want[:32], '<i8')}"]
    g, w = (np.frombuffer(b[32:], STATE_DTYPE) for b in (got, want))
    for m in range(P):
        if g[m].tobytes() != w[m].tobytes():
            out.append(f"member {m}: {g[m]} != {w[m]}")
    return "\n".join(out)


def _three_calls(gpu, lib, P, q, mf, family, seed):
    """Init and three consecutive calls, the members' episodes advanced in between so that
    ``since`` and ``round`` matter; everything is checked after each. Returns the final bytes."""
    hp = _hp(P, seed)
    dev = Dev(gpu, lib, P, q, mf, hp, seed=seed)
    ora = sel.SelectionOracle(hp, q, MIN_EPISODES, seed=seed)
    state, guard, slab, _ = dev.read()
    assert state == ora.pack(), "the empty state"
    assert guard == bytes([0xAB]) * GUARD
    episodes, avg = sel.board_family(family, P, q, MIN_EPISODES, seed=seed + P)
    replaced = 0
    for call in range(3):
        board = dev.write_board(episodes, avg, seed=call)
        assert dev.step() == 0
        pairs = ora.step(episodes, avg)
        state, guard, after, board_after = dev.read()
        d = _diff(state, ora.pack(), P)
        assert not d, f"{family}, call {call}:\n{d}"
        want = slab.copy()
        for l, s in pairs:                                   # rule 7: the loser's slab is its source's, as it was
            want[l * mf: (l + 1) * mf] = slab[s * mf: (s + 1) * mf]
        bad = np.flatnonzero(after != want)
        assert bad.size == 0, f"{family}, call {call}: slab differs first at float {bad[0]} (member {bad[0] // mf})"
        assert guard == bytes([0xAB]) * GUARD and board_after == board
        if call == 0:
            R = sum(r >= 0 for r in ora.rank_now)
            if family == "short":                            # a no-op that still ranks
                assert not pairs and R == 2 * q - 1
            if family in ("distinct", "equal", "zeros", "inf", "exact"):
                assert len(pairs) == q
        replaced += len(pairs)
        slab = after
        episodes = episodes + np.arange(P) % 3 + (MIN_EPISODES - 1)
    assert ora.round == 3 and ora.replaced_total == replaced
    return state, slab.tobytes()


@pytest.mark.parametrize("family", sel.FAMILIES)
@pytest.mark.parametrize("P,q", PQ)
def test_members_quantiles_and_board_families(gpu, built_lib, P, q, family):
    """36 floats per member: nine 16-B vectors, fewer than a wave. Twice: the same bytes."""
    a = _three_calls(gpu, built_lib, P, q, 36, family, seed=P + q)
    b = _three_calls(gpu, built_lib, P, q, 36, family, seed=P + q)
    assert a == b


@pytest.mark.parametrize("member_floats", ("one", "below", "at", "above", "real"))
def test_slab_sizes(gpu, built_lib, member_floats):
    """One vector; one vector below, at and above what a copy workgroup moves per pass; the real
    slab of a 256-wide agent (more than COPY_CHUNKS workgroups' passes: the grid is clamped and
    every lane loops)."""
    from sacenv import _lib
    share = _share()
    mf = {"one": 4, "below": share - 4, "at": share, "above": share + 4, "real": _real_member_floats()}[member_floats]
    if member_floats == "real":
        assert mf > share * _lib.SELECT_COPY_CHUNKS and mf % 4 == 0
    a = _three_calls(gpu, built_lib, 4, 2, mf, "distinct", seed=3)
    b = _three_calls(gpu, built_lib, 4, 2, mf, "distinct", seed=3)
    assert a == b


def test_argument_errors_change_nothing(gpu, built_lib):
    """Every error of the header returns its code; the state, the slab and the guards stay as they
    were."""
    from sacenv import _lib
    lib, P, mf = built_lib, 4, 36
    hp = _hp(P)
    dev = Dev(gpu, lib, P, 1, mf, hp)
    episodes, avg = sel.board_family("distinct", P, 1, MIN_EPISODES)
    dev.write_board(episodes, avg)
    assert dev.step() == 0
    before = dev.read()
    assert np.frombuffer(before[0][:16], "<i8").tolist() == [1, 1]
    nan, inf = float("nan"), float("inf")
    good = dev.params
    b, s, w, st = dev.board.data_ptr(), dev.state.data_ptr(), dev.slab.data_ptr(), dev._stream()

    def params(**kw):
        fields = {n: getattr(good, n) for n, _ in _lib.Select._fields_}
        fields.update(kw)
        for name, n in (("factor", 2), ("lo", 4), ("hi", 4)):
            fields[name] = (ctypes.c_double * n)(*fields[name])
        return _lib.Select(**fields)

    cases = [(E_SIZE, kw) for kw in (dict(members=1), dict(members=65), dict(quantile=0), dict(quantile=3),
                                     dict(lookback=0), dict(lookback=129), dict(min_episodes=0),
                                     dict(member_floats=0), dict(member_floats=mf + 2))]
    cases += [(E_RANGE, kw) for kw in (dict(factor=(nan, 1.2)), dict(factor=(0.8, inf)), dict(factor=(0.0, 1.2)),
                                       dict(lo=(nan, 0, 0, 0)), dict(hi=(1, inf, 1, 1)),
                                       dict(lo=(0, 0, 0.5, 0), hi=(1, 1, 0.25, 1)))]
    n = ctypes.c_int64(-7)
    for code, kw in cases:
        p = params(**kw)
        assert lib.sacenv_select_step(ctypes.byref(p), b, s, w, st) == code, kw
        assert lib.sacenv_select_init(ctypes.byref(p), dev.hp0, s, st) == code, kw
        assert lib.sacenv_select_bytes(ctypes.byref(p), ctypes.byref(n)) == code and n.value == -7, kw
    g = ctypes.byref(good)
    assert lib.sacenv_select_step(None, b, s, w, st) == E_NULL
    assert lib.sacenv_select_step(g, None, s, w, st) == E_NULL
    assert lib.sacenv_select_step(g, b, None, w, st) == E_NULL
    assert lib.sacenv_select_step(g, b, s, None, st) == E_NULL
    assert lib.sacenv_select_step(g, b + 8, s, w, st) == E_RANGE
    assert lib.sacenv_select_step(g, b, s + 8, w, st) == E_RANGE
    assert lib.sacenv_select_step(g, b, s, w + 4, st) == E_RANGE
    assert lib.sacenv_select_init(g, None, s, st) == E_NULL
    assert lib.sacenv_select_init(g, dev.hp0, None, st) == E_NULL
    assert lib.sacenv_select_init(g, dev.hp0, s + 8, st) == E_RANGE
    for field, bad in (("lr_actor", nan), ("lr_critic", inf), ("gamma", -inf), ("tau", nan)):
        hp2 = (_lib.SacMember * P)(*[_lib.SacMember(*row, 2.0) for row in hp])
        setattr(hp2[P - 1], field, bad)
        assert lib.sacenv_select_init(g, hp2, s, st) == E_RANGE, field
    after = dev.read()
    assert after[0] == before[0] and after[1] == before[1] and after[3] == before[3]
    assert np.array_equal(after[2], before[2])


# ---- with the real pieces

def _log_for(dev, scores):
    """Member m's episodes (env 64 m) with the scores ``scores[m]``, in a log buffer written by
    hand."""
    from sacenv.episodes import ENTRY_DTYPE
    rows = [(64 * m, s) for m, ss in enumerate(scores) for s in ss]
    e = np.zeros(len(rows), ENTRY_DTYPE)
    for i, (env, score) in enumerate(rows):
        e[i] = (i + 1, score, env, 7, 5)
    dev.write(len(e), e)


def _population_and_board(gpu, built_lib, scores):
    """A population of four members that learnt once (so its Adam moments are not zero) and a
    ``MemberScoreboard`` that has read ``scores``."""
    from sacenv import MemberScoreboard
    from test_sac_population_gpu import _population, _stacked
    from test_scoreboard_gpu import Dev as BoardDev
    P = 4
    pop = _population(gpu, P, 256, 11)
    _, batch, noise = _stacked(gpu, P, 256, 11, 1)
    pop.learn(batch, noise, losses=False)
    dev = BoardDev(gpu, built_lib, P, 64, 5, cap=64)
    log = types.SimpleNamespace(device=gpu, env_base=0, capacity=64, watchers=[], log=dev.log, term_names=())
    board = MemberScoreboard(log, P, 64, lookback=5)
    _log_for(dev, scores)
    board.update()
    return pop, board


SCORES = ([5.0, 7.0, 6.0], [3.0, 2.5, 3.5], [1.0, 2.0, 1.5], [-4.0, -3.0, -5.0])     # member 0 best, 3 worst


def test_end_to_end_with_population_and_board(gpu, built_lib):
    from sacenv import PopulationSelection
    from sacenv.sac_native import NativeSAC
    from test_sac_population_gpu import _stacked
    pop, board = _population_and_board(gpu, built_lib, SCORES)
    twin, _ = _population_and_board(gpu, built_lib, SCORES)
    assert torch.equal(pop.weights, twin.weights) and pop.adam_step == 1
    configs = list(pop.configs)
    selection = PopulationSelection(board, pop, quantile=1, min_episodes=3, seed=5)
    rec = board.records()
    ora = sel.SelectionOracle([[c.lr_alpha, c.lr_beta, c.gamma, c.tau] for c in configs], 1, 3, seed=5)
    assert ora.step(rec["episodes"], rec["avg"]) == [(3, 0)]
    winner = pop.weights[0].clone()
    out = selection.step()
    assert selection.raw() == ora.pack()
    # the slab: weights, Adam moments, target net and kernel copies
    assert torch.equal(pop.weights[3].view(torch.int32), winner.view(torch.int32))
    assert torch.equal(pop.weights[:3].view(torch.int32), twin.weights[:3].view(torch.int32))
    m_off, v_off = pop.layout.adam_m[0], pop.layout.adam_v[0]
    for off in (m_off, v_off):
        assert bool((pop.weights[3, off: off + 4096] != 0).any())
    # the values: the oracle's doubles exactly, everywhere the host keeps them
    want = ora.hp[3]
    assert out == [{"member": 3, "source": 0, **dict(zip(
        ("learning_rate_alpha", "learning_rate_beta", "gamma", "tvn_parameter_modulation_tau"), want))}]
    c = pop.configs[3]
    assert [c.lr_alpha, c.lr_beta, c.gamma, c.tau] == want and pop.members[3].cfg is c
    assert list(pop.members[3].hpset().values()) == want
    h = pop._hp[3]
    assert [h.lr_actor, h.lr_critic, h.gamma, h.tau, h.reward_scale] == [*want, configs[3].reward_scale]
    assert c == dataclasses.replace(configs[3], lr_alpha=want[0], lr_beta=want[1], gamma=want[2], tau=want[3])
    assert pop.configs[:3] == configs[:3] and selection.commit() == []
    table = selection.table()
    assert [(r["rank"], r["replaced"], r["parent"]) for r in table] == [(0, 0, None), (1, 0, None), (2, 0, None),
                                                                        (3, 1, 0)]
    assert [list(r.values())[4:] for r in table] == ora.hp
    # one learn, no sync in between: member 3 is a stand-alone agent on member 0's old slab with its
    # own new config; members 0-2 are the twin's
    per, batch, noise = _stacked(gpu, 4, 256, 11, 2)
    p = pop.params
    alone = NativeSAC.from_slab(gpu, pop.configs[3], winner, obs_dim=p.obs_dim, max_action=p.max_action,
                                adam_eps=p.adam_eps, noise_seed=None, adam_step=pop.adam_step)
    pop.learn(batch, noise, losses=False)
    twin.learn(batch, noise, losses=False)
    alone.learn(*per[3], losses=False)
    torch.cuda.synchronize(gpu)
    n = alone.weights.numel()
    assert torch.equal(pop.weights[3, :n].view(torch.int32), alone.weights.view(torch.int32))
    assert torch.equal(pop.weights[:3].view(torch.int32), twin.weights[:3].view(torch.int32))
    assert not torch.equal(pop.weights[3], twin.weights[3]) and not torch.equal(pop.weights[3], pop.weights[0])


def test_commit_refuses_another_population(gpu, built_lib):
    from sacenv import PopulationSelection, _lib
    from test_sac_population_gpu import _population
    pop, board = _population_and_board(gpu, built_lib, SCORES)
    selection = PopulationSelection(board, pop, quantile=1, min_episodes=3)
    selection.select()
    selection.population = _population(gpu, 3, 256, 11)
    with pytest.raises(ValueError, match="3 members"):
        selection.commit()
    selection.population = types.SimpleNamespace(P=4, device=gpu, pop_layout=types.SimpleNamespace(
        member_floats=pop.pop_layout.member_floats + 4))
    with pytest.raises(ValueError, match="floats per member"):
        selection.commit()
    selection.population = types.SimpleNamespace(P=4, device=torch.device("cuda", 1), pop_layout=pop.pop_layout)
    with pytest.raises(ValueError, match="different devices"):
        selection.commit()
    selection.population = pop
    assert [r["member"] for r in selection.commit()] == [3]
    with pytest.raises(ValueError, match="3 members"):
        PopulationSelection(board, _population(gpu, 3, 256, 11))
    with pytest.raises(_lib.SacenvError):                    # 2 q > P: found by the library, on the host
        PopulationSelection(board, pop, quantile=3)


def test_the_example_selects(gpu, built_lib, monkeypatch, capsys):
    """``--select-every 8`` at the example's smallest sizes: the replacements it reports and the
    table it returns are the oracle's, replayed on the boards the run's selections saw."""
    from sacenv import sample_hpsets, selection
    from sacenv.agent import AgentConfig
    spec = importlib.util.spec_from_file_location("train_population",
                                                  os.path.join(ROOT, "examples", "train_population.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = []
    select = selection.PopulationSelection.select

    def recording(self):
        rec = self.board.records()                           # (synchronises: the board as the launch will read it)
        seen.append((rec["episodes"].copy(), rec["avg"].copy()))
        select(self)

    monkeypatch.setattr(selection.PopulationSelection, "select", recording)
    torch.manual_seed(5)
    out = mod.main(["--members", "2", "--envs-per-member", "64", "--iters", "40", "--batch", "256",
                    "--max-episode-steps", "7", "--lookback", "5", "--select-every", "8", "--quantile", "1",
                    "--min-episodes", "2", "--select-seed", "9"])
    printed = capsys.readouterr().out
    assert len(seen) == 5 and "on the device:" not in printed
    configs = sample_hpsets(2, 0, base=AgentConfig(batch_size=256))
    ora = sel.SelectionOracle([[c.lr_alpha, c.lr_beta, c.gamma, c.tau] for c in configs], 1, 2, seed=9)
    want = []
    for k, (episodes, avg) in enumerate(seen):
        for l, s in ora.step(episodes, avg):
            want.append({"iter": 8 * k + 7, "member": l, "source": s, **dict(zip(selection.HP_KEYS, ora.hp[l]))})
    assert len(want) >= 2 and out["replacements"] == want
    assert printed.count(" <- member ") == len(want)
    assert out["selection"] == [
        {"member": m, "rank": ora.rank_now[m] if ora.rank_now[m] >= 0 else None, "replaced": ora.replaced[m],
         "parent": ora.parent[m] if ora.parent[m] >= 0 else None, **dict(zip(selection.HP_KEYS, ora.hp[m]))}
        for m in range(2)]
    for m, row in enumerate(out["table"]):                   # the members' last values
        assert [row[k] for k in selection.HP_KEYS] == ora.hp[m]
