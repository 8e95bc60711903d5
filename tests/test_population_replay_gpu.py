"""PopulationReplay (sacenv_replay_pop.hip, include/sacenv_population_replay.h) against P
stand-alone DeviceReplayBuffer objects, bit for bit, and its draws against numpy itself.

A population launch runs the device code of the one-buffer kernels (sacenv_replay.hip's bodies)
on member m's slab and rows; nothing in them is atomic or order-dependent, so member m's slab
must end with exactly the bytes a ``DeviceReplayBuffer`` with member m's seed ends with after
the same calls: ``torch.equal`` on ``pop.arena[m]`` against that buffer's ``arena`` (the ring,
the count, the MT19937 key and position) and on every output. The first test checks the premise.

The reference for the draws is independent of this project: member m's ``idx``, call by call,
equal ``np.random.RandomState(seed_m).choice(min(cntr, M), B)`` on one stream per member.

Shapes are the smallest that reach each branch of ``store_body`` (a wrap inside a store; n > M,
rows skipped; one row) and of the draw (ranges 1 -- no words drawn --, 63, 300 and M; batches
from one row to more than one 624-word block per call); P = 9 is more members than XCDs.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

GUARD = 4096          # canary bytes either side of the arena
PAD = 64              # canary elements either side of every input
SHAPES = {100: (11, 1), 1 << 14: (1, 1), 50: (14, 2)}       # M -> (D, A), as the CPU layout test


def _seeds(P):
    return [7 + 13 * m for m in range(P)]


def _pop(gpu, P, M, **kw):
    from sacenv.population_replay import PopulationReplay
    D, A = SHAPES[M]
    return PopulationReplay(P, M, (D,), A, device=gpu, seeds=_seeds(P), **kw)


def _refs(gpu, P, M, **kw):
    from sacenv.replay import DeviceReplayBuffer
    D, A = SHAPES[M]
    return [DeviceReplayBuffer(M, (D,), A, device=gpu, seed=s, **kw) for s in _seeds(P)]


def _guard(pop):
    """Move the arena between two canary regions; returns the whole guarded buffer. (The field
    views of ``pop`` keep pointing at the old storage: these tests read ``pop.arena``.)"""
    P, mb = pop.arena.shape
    big = torch.full((2 * GUARD + P * mb,), 0xA5, dtype=torch.uint8, device=pop.device)
    mid = big[GUARD: GUARD + P * mb].view(P, mb)
    mid.copy_(pop.arena)
    assert mid.data_ptr() % 256 == 0
    pop.arena = mid
    return big


def _guard_ok(big):
    return bool((big[:GUARD] == 0xA5).all()) and bool((big[-GUARD:] == 0xA5).all())


class Padded:
    """A contiguous tensor between two canary runs."""

    def __init__(self, t, gpu):
        t = t.contiguous()
        canary = 77 if t.dtype == torch.uint8 else 12345
        self.full = torch.full((t.numel() + 2 * PAD,), canary, dtype=t.dtype, device=gpu)
        self.t = self.full[PAD: PAD + t.numel()].view(t.shape)
        self.t.copy_(t)
        self.before = self.full.clone()

    def untouched(self):
        return torch.equal(self.full, self.before)

    def pads_untouched(self):
        return torch.equal(self.full[:PAD], self.before[:PAD]) and torch.equal(self.full[-PAD:], self.before[-PAD:])


def _rows(gpu, P, n, M, seed, reward_f32=True):
    """One lockstep store's inputs [P, n, ...]; about a third of the codes non-zero, from 0..6."""
    D, A = SHAPES[M]
    g = torch.Generator().manual_seed(seed)
    s = torch.rand((P, n, D), generator=g)
    a = torch.rand((P, n, A), generator=g) * 2 - 1
    r = torch.rand((P, n), generator=g, dtype=torch.float64) * 3 - 2
    r = r.to(torch.float32) if reward_f32 else r
    s2 = torch.rand((P, n, D), generator=g)
    fs = torch.rand((P, n, D), generator=g) + 10
    code = torch.randint(1, 7, (P, n), generator=g, dtype=torch.uint8)
    code[torch.rand((P, n), generator=g) > 1 / 3] = 0
    return [Padded(x, gpu) for x in (s, a, r, s2, code, fs)]


def _same_arenas(pop, refs, what=""):
    torch.cuda.synchronize()
    assert pop.mem_cntr == refs[0].mem_cntr
    for m, ref in enumerate(refs):
        assert torch.equal(pop.arena[m], ref.arena), f"member {m}: arena differs {what}"


def _store_both(pop, refs, rows, lt=None, lt_ref=None, extras=True, **kw):
    s, a, r, s2, c, fs = (x.t for x in rows)
    pop.store_batch(s, a, r, s2, c, final_state=fs if extras else None, last_term=lt, **kw)
    for m, ref in enumerate(refs):
        ref.store_batch(s[m], a[m], r[m], s2[m], c[m], final_state=fs[m] if extras else None,
                        last_term=None if lt_ref is None else lt_ref[m])


def test_two_equal_buffers_end_equal(gpu, built_lib):
    """The premise: one buffer's stores and samples are the same from run to run, bit for bit."""
    from sacenv.replay import DeviceReplayBuffer
    M = 100
    D, A = SHAPES[M]
    a, b = (DeviceReplayBuffer(M, (D,), A, device=gpu, seed=3) for _ in range(2))
    lts = [torch.zeros(64, dtype=torch.uint8, device=gpu) for _ in range(2)]
    outs = []
    for rb, lt in zip((a, b), lts):
        for k in range(3):
            s, ac, r, s2, c, fs = (x.t[0] for x in _rows(gpu, 1, 64, M, 50 + k))
            rb.store_batch(s, ac, r, s2, c, final_state=fs, last_term=lt)
        outs.append(rb.sample(256, as_bool=False))
    torch.cuda.synchronize()
    assert torch.equal(a.arena, b.arena) and torch.equal(lts[0], lts[1])
    for x, y in zip(*outs):
        assert torch.equal(x, y)


# (M, rows per store, stores): a wrap inside the second store | n - M > 0: rows skipped, their
# last_term still updated | one row (the rng == 0 case for the sample that follows)
STORE_CASES = [(100, 64, 3), (50, 64, 2), (1 << 14, 1, 1)]


@pytest.mark.parametrize("reward_f32", [True, False])
@pytest.mark.parametrize("M,n,stores", STORE_CASES)
@pytest.mark.parametrize("P", [1, 2, 3, 9])
def test_store_matches_stand_alone_buffers(gpu, built_lib, P, M, n, stores, reward_f32):
    pop, refs = _pop(gpu, P, M, reward_f32=reward_f32), _refs(gpu, P, M, reward_f32=reward_f32)
    big = _guard(pop)
    _same_arenas(pop, refs, "after init")
    lt = Padded(torch.zeros((P, n), dtype=torch.uint8), gpu)
    lt_ref = [torch.zeros(n, dtype=torch.uint8, device=gpu) for _ in range(P)]
    for k in range(stores):
        rows = _rows(gpu, P, n, M, 1000 * P + 10 * k + M % 7, reward_f32)
        _store_both(pop, refs, rows, lt.t, lt_ref)
        _same_arenas(pop, refs, f"after store {k}")
        assert torch.equal(lt.t, torch.stack(lt_ref)), f"last_term after store {k}"
        assert all(x.untouched() for x in rows), "a store wrote to its inputs"
        assert lt.pads_untouched() and _guard_ok(big)
    assert pop.mem_cntr == stores * n
    # the rows come back out: one sample at this count (a buffer of one row draws no words)
    got = pop.sample(64, as_bool=False)
    for m, ref in enumerate(refs):
        want = ref.sample(64, as_bool=False)
        for x, y in zip(got, want):
            assert torch.equal(x[m], y), f"member {m}"
    _same_arenas(pop, refs, "after the sample")
    assert _guard_ok(big)
    one = pop.export_member(P - 1)
    assert one.mem_cntr == pop.mem_cntr and torch.equal(one.arena, refs[P - 1].arena)


def test_store_without_final_state_and_last_term(gpu, built_lib):
    P, M = 2, 100
    pop, refs = _pop(gpu, P, M), _refs(gpu, P, M)
    for k in range(3):
        _store_both(pop, refs, _rows(gpu, P, 64, M, 400 + k), extras=False)
        _same_arenas(pop, refs, f"after store {k}")


@pytest.mark.parametrize("P,M,n", [(3, 100, 64), (2, 50, 64)])
def test_host_count_equals_device_count(gpu, built_lib, P, M, n):
    """``graph_safe=True`` (the device counts: a store and an advance launch) against the
    default (the host's count in one launch)."""
    a, b = _pop(gpu, P, M), _pop(gpu, P, M)
    lts = [torch.zeros((P, n), dtype=torch.uint8, device=gpu) for _ in range(2)]
    for k in range(3):
        s, ac, r, s2, c, fs = (x.t for x in _rows(gpu, P, n, M, 70 + k))
        a.store_batch(s, ac, r, s2, c, final_state=fs, last_term=lts[0])
        b.store_batch(s, ac, r, s2, c, final_state=fs, last_term=lts[1], graph_safe=True)
        torch.cuda.synchronize()
        assert torch.equal(a.arena, b.arena), f"after store {k}"
        assert torch.equal(lts[0], lts[1])
    assert int(b._cntr[P - 1, 0]) == 3 * n == a.mem_cntr == b.mem_cntr


# rows held (M): 1, 63 and 300 of 1 << 14; 128 of 100 (the ring is full: the range is M)
@pytest.mark.parametrize("batch", [1, 64, 256, 1000])
@pytest.mark.parametrize("M,held", [(1 << 14, 1), (1 << 14, 63), (1 << 14, 300), (100, 128)])
def test_sample_matches_stand_alone_buffers_and_numpy(gpu, built_lib, M, held, batch):
    P = 3
    pop, refs = _pop(gpu, P, M), _refs(gpu, P, M)
    big = _guard(pop)
    left, k = held, 0
    while left:
        n = min(left, 64)
        _store_both(pop, refs, _rows(gpu, P, n, M, 9000 + held + k), extras=False)
        left, k = left - n, k + 1
    rng = [np.random.RandomState(s) for s in _seeds(P)]
    top = min(held, M)
    for call in range(8):
        got = pop.sample(batch, as_bool=False)
        assert [tuple(x.shape[:2]) for x in got] == [(P, batch)] * 6
        for m, ref in enumerate(refs):
            want = ref.sample(batch, as_bool=False)
            for x, y in zip(got, want):
                assert torch.equal(x[m], y), f"member {m}, call {call}"
            idx = got[5][m].cpu().numpy()
            assert idx.min() >= 0 and idx.max() < top
            assert np.array_equal(idx, rng[m].choice(top, batch)), f"member {m}, call {call}: not numpy's draws"
        _same_arenas(pop, refs, f"after sample {call}")
    assert _guard_ok(big)
    # as_bool: the dones as booleans
    got = pop.sample(batch)
    assert got[4].dtype == torch.bool and torch.equal(got[4][0], refs[0].sample(batch)[4])


def test_sample_that_ends_on_the_last_word_of_a_block(gpu, built_lib):
    """``RandomState(105).choice(100, 1000)`` accepts word 623 of a block as its last: the
    position written back is 624, and the next sample has to twist before its first word."""
    from sacenv.population_replay import PopulationReplay
    from sacenv.replay import DeviceReplayBuffer
    P, M, held, batch = 3, 100, 128, 1000
    D, A = SHAPES[M]
    seeds = [7, 105, 20]
    pop = PopulationReplay(P, M, (D,), A, device=gpu, seeds=seeds)
    refs = [DeviceReplayBuffer(M, (D,), A, device=gpu, seed=s) for s in seeds]
    big = _guard(pop)
    for k in range(2):
        _store_both(pop, refs, _rows(gpu, P, 64, M, 9500 + k), extras=False)
    probe = np.random.RandomState(105)
    probe.choice(M, batch)
    assert probe.get_state()[2] == 624
    rng = [np.random.RandomState(s) for s in seeds]
    for call in range(3):
        got = pop.sample(batch, as_bool=False)
        for m, ref in enumerate(refs):
            want = ref.sample(batch, as_bool=False)
            for x, y in zip(got, want):
                assert torch.equal(x[m], y), f"member {m}, call {call}"
            assert np.array_equal(got[5][m].cpu().numpy(), rng[m].choice(M, batch)), \
                f"member {m}, call {call}: not numpy's draws"
        _same_arenas(pop, refs, f"after sample {call}")
        if call == 0:
            assert pop.arena[1, pop.layout.mt_pos: pop.layout.mt_pos + 4].view(torch.int32).item() == 624
    assert _guard_ok(big)


def test_one_member_is_one_buffer(gpu, built_lib):
    """P = 1 runs the one-buffer kernels (the branch in sacenv_replay_pop.hip): both count
    forms of the store, the sample and the gather."""
    M, B = 100, 256
    pop, refs = _pop(gpu, 1, M), _refs(gpu, 1, M)
    big = _guard(pop)
    lt, lt_ref = torch.zeros((1, 64), dtype=torch.uint8, device=gpu), [torch.zeros(64, dtype=torch.uint8, device=gpu)]
    rng = np.random.RandomState(_seeds(1)[0])
    for k in range(3):
        _store_both(pop, refs, _rows(gpu, 1, 64, M, 600 + k), lt, lt_ref, graph_safe=bool(k & 1))
        _same_arenas(pop, refs, f"after store {k}")
        assert torch.equal(lt[0], lt_ref[0])
        got, want = pop.sample(B, as_bool=False), refs[0].sample(B, as_bool=False)
        for x, y in zip(got, want):
            assert torch.equal(x[0], y)
        assert np.array_equal(got[5][0].cpu().numpy(), rng.choice(min(64 * (k + 1), M), B))
        for x, y in zip(pop.gather(got[5], as_bool=False), refs[0].gather(want[5], as_bool=False)):
            assert torch.equal(x[0], y)
        _same_arenas(pop, refs, f"after sample {k}")
    assert _guard_ok(big)


def test_sample_of_an_empty_buffer_raises(gpu, built_lib):
    pop, ref = _pop(gpu, 2, 100), _refs(gpu, 1, 100)[0]
    for rb in (pop, ref):
        with pytest.raises(ValueError, match="a must be greater than 0"):
            rb.sample(4)


def test_gather_matches_stand_alone_buffers(gpu, built_lib):
    P, M = 3, 100
    pop, refs = _pop(gpu, P, M), _refs(gpu, P, M)
    for k in range(2):
        _store_both(pop, refs, _rows(gpu, P, 64, M, 30 + k))
    g = torch.Generator().manual_seed(5)
    idx = torch.randint(-5, M + 5, (P, 300), generator=g).to(gpu)
    idx[:, :4] = torch.tensor([-1, M, M - 1, 0])
    got = pop.gather(idx, as_bool=False)
    for m, ref in enumerate(refs):
        want = ref.gather(idx[m], as_bool=False)
        for x, y in zip(got, want):
            assert torch.equal(x[m], y), f"member {m}"
        outside = (idx[m] < 0) | (idx[m] >= M)
        assert outside.any() and not got[0][m][outside].any() and not got[2][m][outside].any()
    _same_arenas(pop, refs)


def test_a_poisoned_member_draws_nothing(gpu, built_lib):
    """The documented rule of a stream whose position is < 0 (a staged draw that ran short
    marks its arena so): its draws come out -1 and the poison stays; the others go on."""
    P, M, B = 3, 100, 64
    pop, refs = _pop(gpu, P, M), _refs(gpu, P, M)
    _store_both(pop, refs, _rows(gpu, P, 64, M, 11))
    pop.mt_pos[1] = -1
    for call in range(2):
        got = pop.sample(B, as_bool=False)
        torch.cuda.synchronize()
        assert bool((got[5][1] == -1).all()) and int(pop.mt_pos[1]) == -1
        assert not got[0][1].any() and not got[4][1].any()       # rows outside the ring: zeros
        for m in (0, 2):
            want = refs[m].sample(B, as_bool=False)
            for x, y in zip(got, want):
                assert torch.equal(x[m], y), f"member {m}, call {call}"
            torch.cuda.synchronize()
            assert torch.equal(pop.arena[m], refs[m].arena)


def _cfg(m, B, max_size):
    from sacenv.agent import AgentConfig
    return AgentConfig(lr_alpha=0.0015 + 0.001 * m, lr_beta=0.0003 * (m + 2), gamma=0.95 + 0.004 * m,
                       tau=0.002 * (m + 1), reward_scale=2.0 + m, batch_size=B, max_size=max_size)


def test_learn_through_the_population_replay(gpu, built_lib):
    from sacenv.population import NativeSACPopulation
    from sacenv.population_replay import PopulationReplay
    P, B, D, M = 2, 256, 11, 1 << 14
    cfgs = [_cfg(m, B, M) for m in range(P)]
    replay = PopulationReplay(P, M, (D,), 1, device=gpu, seeds=[5, 6])
    pa = NativeSACPopulation(gpu, cfgs, obs_dim=D, init_seeds=[1, 2], replay=replay)
    pb = NativeSACPopulation(gpu, cfgs, obs_dim=D, init_seeds=[1, 2], buffer_seeds=[5, 6])
    assert pa.memory is replay and len(pb.memory) == P
    g = torch.Generator().manual_seed(2)
    noise = (torch.randn((P, B), generator=g).to(gpu), torch.randn((P, B), generator=g).to(gpu))
    for k in range(2):
        assert pa.learn(noise=noise) is None and pb.learn(noise=noise) is None     # fewer than B rows held
        s = torch.rand((P, 150, D), generator=g).to(gpu)
        a = (torch.rand((P, 150, 1), generator=g) * 2 - 1).to(gpu)
        r = torch.rand((P, 150), generator=g).to(gpu)
        s2 = torch.rand((P, 150, D), generator=g).to(gpu)
        c = (torch.rand((P, 150), generator=g) < 0.1).to(torch.uint8).to(gpu)
        replay.store_batch(s, a, r, s2, c)
        for m in range(P):
            pb.remember(m, s[m], a[m], r[m], s2[m], c[m])
    assert pa.adam_step == pb.adam_step == 0
    la, lb = pa.learn(noise=noise), pb.learn(noise=noise)
    torch.cuda.synchronize()
    assert la is not None and lb is not None and pa.adam_step == pb.adam_step == 1
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
    assert torch.equal(pa.weights, pb.weights)
    for m in range(P):
        assert torch.equal(replay.arena[m], pb.memory[m].arena)


def test_store_env_step_on_a_real_env(gpu, built_lib):
    from sacenv import VecBoatEnv
    from sacenv.population_replay import PopulationReplay
    from sacenv.replay import DeviceReplayBuffer
    P, n, M, D = 3, 64, 500, 11
    env = VecBoatEnv({"base_settings": {"experiment": 6, "test_mode": 0}}, P * n, seed=0, device=gpu,
                     max_episode_steps=5)
    pop = PopulationReplay(P, M, (D,), 1, device=gpu, seeds=_seeds(P))
    refs = [DeviceReplayBuffer(M, (D,), 1, device=gpu, seed=s) for s in _seeds(P)]
    lt = [torch.zeros(n, dtype=torch.uint8, device=gpu) for _ in range(P)]
    act = (torch.rand(P * n, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(gpu)
    obs = env.reset().clone()
    ended = 0
    for step in range(12):
        env.step(act)
        pop.store_env_step(obs, act, env)
        for m, ref in enumerate(refs):
            rows = slice(m * n, (m + 1) * n)
            ref.store_batch(obs[rows], act[rows], env.reward[rows], env.obs[rows], env.term[rows],
                            final_state=env.final_obs[rows], last_term=lt[m])
        ended += int((env.term != 0).sum())
        obs = env.obs.clone()
        _same_arenas(pop, refs, f"after step {step}")
    assert ended >= P * n      # endings (and auto-resets) did occur
    assert torch.equal(pop._last_term[env], torch.cat(lt))


def test_the_example_prints_the_same_with_either_replay(gpu, built_lib, capsys):
    spec = importlib.util.spec_from_file_location("train_population",
                                                  os.path.join(ROOT, "examples", "train_population.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for replay in ("population", "members"):
        torch.manual_seed(1234)
        out[replay] = mod.main(["--members", "2", "--envs-per-member", "64", "--iters", "12", "--batch", "256",
                                "--replay", replay])
    capsys.readouterr()
    a, b = out["population"], out["members"]
    assert a["replay"] == "population" and b["replay"] == "members"
    assert a["losses"] is not None and a["losses"] == b["losses"]
    assert a["table"] == b["table"]


def test_host_validation(gpu, built_lib):
    """Refused on the host, before any launch: the arena stays as it was."""
    from sacenv.population import NativeSACPopulation
    from sacenv.population_replay import PopulationReplay
    P, M, n = 3, 100, 8
    D, A = SHAPES[M]
    pop = _pop(gpu, P, M)
    s, a, r, s2, c, fs = (x.t for x in _rows(gpu, P, n, M, 1))
    pop.store_batch(s, a, r, s2, c)
    torch.cuda.synchronize()
    before = pop.arena.clone()
    with pytest.raises(ValueError):                                  # a wrong leading P
        pop.store_batch(s[:2], a[:2], r[:2], s2[:2], c[:2])
    with pytest.raises(ValueError):
        pop.store_batch(s, a, r[:2], s2, c)
    with pytest.raises(ValueError):
        pop.store_batch(s, a, r, s2[:, :4], c)
    with pytest.raises(ValueError):
        pop.gather(torch.zeros((P + 1, 4), dtype=torch.int64))
    good = torch.zeros((P, n), dtype=torch.uint8, device=gpu)
    for bad in (torch.zeros((P, 2 * n), dtype=torch.uint8, device=gpu)[:, ::2],          # not contiguous
                torch.zeros((P, n), dtype=torch.int32, device=gpu),                      # wrongly typed
                torch.zeros((P, n), dtype=torch.uint8),                                  # on the host
                torch.zeros((P - 1, n), dtype=torch.uint8, device=gpu)):                 # too few bytes
        with pytest.raises(ValueError, match="last_term"):
            pop.store_batch(s, a, r, s2, c, last_term=bad)
    assert pop.mem_cntr == n and not good.any()
    torch.cuda.synchronize()
    assert torch.equal(pop.arena, before)
    with pytest.raises(ValueError):
        PopulationReplay(0, M, (D,), A, device=gpu)
    with pytest.raises(ValueError):
        PopulationReplay(65, M, (D,), A, device=gpu)
    with pytest.raises(ValueError, match="seed"):
        PopulationReplay(2, M, (D,), A, device=gpu, seeds=[1])

    # a replay that disagrees with its population
    B, MS = 256, 1 << 10
    cfgs = [_cfg(m, B, MS) for m in range(2)]
    ok = PopulationReplay(2, MS, (11,), 1, device=gpu)
    for what, bad in (("members", PopulationReplay(3, MS, (11,), 1, device=gpu)),
                      ("max_size", PopulationReplay(2, MS // 2, (11,), 1, device=gpu)),
                      ("obs_dim", PopulationReplay(2, MS, (5,), 1, device=gpu))):
        with pytest.raises(ValueError, match=what):
            NativeSACPopulation(gpu, cfgs, replay=bad)
    with pytest.raises(TypeError):
        NativeSACPopulation(gpu, cfgs, replay=[ok])
    holder = NativeSACPopulation(gpu, cfgs, replay=ok)
    z = torch.zeros((4, 11), device=gpu)
    with pytest.raises(TypeError, match="store_batch"):
        holder.remember(0, z, torch.zeros((4, 1), device=gpu), torch.zeros(4, device=gpu), z,
                        torch.zeros(4, dtype=torch.uint8, device=gpu))
    assert ok.mem_cntr == 0
