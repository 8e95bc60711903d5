"""The pooled sample (sacenv_replay_pop.hip: k_rb_draw_pool / k_rb_gather_pool, include/
sacenv_population_share.h) against numpy, bit for bit.

The reference for the draws is numpy's own legacy generator (tests/share_oracle.py): per member
``RandomState(seed_m).choice(s, B - K)`` then ``.choice(P s, K)``, as global rows owner x M + row;
the reference for the rows is the members' rings read back. Nothing in the two kernels is atomic
or order-dependent, so every comparison is for equality of bytes.

Shapes are the smallest at which the draw can still go wrong: (P, M, rows stored) = (9, 57, 80) is
a wrapped ring whose pool range 513 is one past a power of two (about half of the words rejected,
64 pool rows take ~122 words) with more members than XCDs; (2, 40 000, 32 769) is a partly filled
ring whose pool range 65 538 makes 700 pool rows take ~1 378 words, across two twists; (2, 64, 1)
is s = 1: the own draw consumes nothing and the pool range is P. One filled replay per shape is
built once and put back to its snapshot before every use.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import share_oracle
from conftest import ROOT

pytestmark = pytest.mark.gpu

D, A = 5, 2
FILLS = [(9, 57, 80), (2, 40000, 32769), (2, 64, 1)]           # (P, M, rows stored per member)
DRAWS = [(1, 0), (1, 1), (64, 0), (64, 1), (64, 63), (64, 64), (700, 700)]   # (B, K)
FIELDS = ("state_memory", "action_memory", "reward_memory", "new_state_memory", "terminal_memory")


def _seeds(P):
    return [7 + 13 * m for m in range(P)]


def _new(gpu, P, M, seeds=None):
    from sacenv.population_replay import PopulationReplay
    return PopulationReplay(P, M, (D,), A, device=gpu, seeds=seeds or _seeds(P))


@functools.lru_cache(maxsize=None)
def _filled(gpu, P, M, count, seeds=None):
    """(replay, its arena after the stores, the members' rings as numpy [P, M, ...] in the
    outputs' order): built once per shape; a test copies the snapshot back before it samples."""
    pop = _new(gpu, P, M, seeds)
    g = torch.Generator().manual_seed(1000 * P + M + count)
    left = count
    while left:
        n = min(left, 16384)
        pop.store_batch(torch.rand((P, n, D), generator=g), torch.rand((P, n, A), generator=g) * 2 - 1,
                        torch.rand((P, n), generator=g) * 3 - 2, torch.rand((P, n, D), generator=g),
                        (torch.rand((P, n), generator=g) < 0.3).to(torch.uint8))
        left -= n
    torch.cuda.synchronize()
    members = [pop.export_member(m) for m in range(P)]
    rings = tuple(np.stack([getattr(b, f).cpu().numpy() for b in members]) for f in FIELDS)
    return pop, pop.arena.clone(), rings


def _fresh(gpu, P, M, count):
    pop, snap, rings = _filled(gpu, P, M, count)
    pop.arena.copy_(snap)
    return pop, snap, rings


def _same_bytes(got, want, what=""):
    for name, x, y in zip(FIELDS, got, want):
        x = x.cpu().numpy()
        assert x.shape == y.shape and x.dtype == y.dtype, f"{name} {what}: {x.shape} {x.dtype} / {y.shape} {y.dtype}"
        assert x.tobytes() == y.tobytes(), f"{name} {what}"


@pytest.mark.parametrize("B,K", DRAWS)
@pytest.mark.parametrize("P,M,count", FILLS)
def test_indices_rows_and_stream_match_numpy(gpu, built_lib, P, M, count, B, K):
    pop, _, rings = _fresh(gpu, P, M, count)
    s = min(count, M)
    rngs = [np.random.RandomState(x) for x in _seeds(P)]
    for call in range(2):                                      # (the second starts where the first stopped)
        got = pop.sample_pool(B, K, as_bool=False)
        want = share_oracle.draw(rngs, P, M, count, B, K)
        idx = got[5].cpu().numpy()
        assert idx.shape == (P, B) and idx.dtype == np.int64
        assert np.array_equal(idx, want), f"call {call}: not numpy's draws"
        assert np.array_equal(idx[:, : B - K] // M, np.repeat(np.arange(P)[:, None], B - K, 1))   # own rows first
        assert (idx % M).max() < s and idx.min() >= 0 and idx.max() < P * M
        _same_bytes(got[:5], share_oracle.gather(rings, want, M), f"call {call}")
    # the key and position written back: a plain sample goes on where numpy goes on
    nxt = pop.sample(64, as_bool=False)[5].cpu().numpy()
    for m in range(P):
        assert np.array_equal(nxt[m], rngs[m].choice(s, 64)), f"member {m}: the stream after the pooled draws"
    if K:                                                      # sample(pool_rows=K) is the same call
        pop, _, _ = _fresh(gpu, P, M, count)
        rngs = [np.random.RandomState(x) for x in _seeds(P)]
        got = pop.sample(B, as_bool=False, pool_rows=K)
        assert np.array_equal(got[5].cpu().numpy(), share_oracle.draw(rngs, P, M, count, B, K))
        assert pop.sample(B, pool_rows=K)[4].dtype == torch.bool


def test_own_fill_that_ends_on_the_last_word_of_a_block(gpu, built_lib):
    """Member 1 (seed 582, found by a search on the CPU): the own fill of its second call,
    ``choice(100, 192)``, accepts word 623 of a block as its last, so the pool fill that follows on
    the same block pair starts at position 624 and has to twist first."""
    P, M, count, B, K = 3, 100, 128, 256, 64
    seeds = (7, 582, 20)
    pop, snap, rings = _filled(gpu, P, M, count, seeds)
    pop.arena.copy_(snap)
    s = min(count, M)
    probe = np.random.RandomState(seeds[1])
    probe.choice(s, B - K), probe.choice(P * s, K), probe.choice(s, B - K)
    assert probe.get_state()[2] == 624
    rngs = [np.random.RandomState(x) for x in seeds]
    for call in range(3):
        got = pop.sample_pool(B, K, as_bool=False)
        want = share_oracle.draw(rngs, P, M, count, B, K)
        assert np.array_equal(got[5].cpu().numpy(), want), f"call {call}: not numpy's draws"
        _same_bytes(got[:5], share_oracle.gather(rings, want, M), f"call {call}")
    nxt = pop.sample(64, as_bool=False)[5].cpu().numpy()
    for m in range(P):
        assert np.array_equal(nxt[m], rngs[m].choice(s, 64)), f"member {m}: the stream after the pooled draws"


def test_every_output_may_be_null(gpu, built_lib):
    """Each output pointer NULL in turn: that output is not written, the others are as before."""
    from sacenv import _lib
    P, M, count = FILLS[0]
    B, K = 64, 32
    pop, _, rings = _fresh(gpu, P, M, count)
    fn, = _lib.require(_lib.REPLAY_SHARE_EXPORTS[:1], "sacenv_population_share.h")
    rngs = [np.random.RandomState(x) for x in _seeds(P)]
    for skip in range(5):
        st, ac, rw, ns, tm, idx = pop._outputs(B, idx=True)
        outs = [st, ac, rw, ns, tm]
        for t in outs:
            t.view(torch.uint8).fill_(0xA5)
        ptrs = [None if k == skip else t.data_ptr() for k, t in enumerate(outs)]
        _lib.check(fn(pop._pp, P, pop.arena.data_ptr(), B, K, pop.mem_cntr, idx.data_ptr(), *ptrs, pop.stream))
        want_idx = share_oracle.draw(rngs, P, M, count, B, K)
        assert np.array_equal(idx.cpu().numpy(), want_idx)
        want = share_oracle.gather(rings, want_idx, M)
        for k, (t, w) in enumerate(zip(outs, want)):
            if k == skip:
                assert bool((t.view(torch.uint8) == 0xA5).all()), f"{FIELDS[k]} was written though NULL"
            else:
                assert t.cpu().numpy().tobytes() == w.tobytes(), f"{FIELDS[k]} with {FIELDS[skip]} NULL"


@pytest.mark.parametrize("B", [1, 64, 700])
@pytest.mark.parametrize("P,M,count", FILLS)
def test_no_pool_rows_is_todays_sample(gpu, built_lib, P, M, count, B):
    """Two replays with the same seeds and rows: ``sample(B)`` on one, the pooled entry point with
    no pool rows on the other."""
    a, snap, _ = _fresh(gpu, P, M, count)
    b = _new(gpu, P, M)
    b.arena.copy_(snap)
    b.mem_cntr = a.mem_cntr
    offset = (torch.arange(P, device=gpu) * M)[:, None]
    for call in range(3):
        x, y = a.sample(B, as_bool=False), b.sample_pool(B, 0, as_bool=False)
        for u, v in zip(x[:5], y[:5]):
            assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), f"call {call}"
        assert torch.equal(y[5] - x[5], offset.expand(P, B)), f"call {call}: idx is not sample's + m M"
        torch.cuda.synchronize()
        assert torch.equal(a.arena, b.arena), f"call {call}: the arenas differ"
    # and sample(B, pool_rows=0) is sample(B) itself: local rows
    a.arena.copy_(snap)
    b.arena.copy_(snap)
    x, y = a.sample(B, as_bool=False), b.sample(B, as_bool=False, pool_rows=0)
    for u, v in zip(x, y):
        assert torch.equal(u, v)


def test_gather_pool(gpu, built_lib):
    P, M, count = FILLS[0]
    pop, snap, rings = _fresh(gpu, P, M, count)
    got = pop.sample_pool(64, 40, as_bool=False)
    again = pop.gather_pool(got[5], as_bool=False)
    for u, v in zip(got[:5], again):
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
    assert pop.gather_pool(got[5])[4].dtype == torch.bool
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(-4, P * M + 4, (P, 300), generator=g)
    idx[:, :6] = torch.tensor([-1, P * M, 1 << 40, P * M - 1, 0, M])
    out = pop.gather_pool(idx, as_bool=False)
    _same_bytes(out, share_oracle.gather(rings, idx.numpy(), M))
    outside = ((idx < 0) | (idx >= P * M)).to(gpu)
    assert int(outside[:, :3].sum()) == 3 * P
    for t in out:
        assert not t[outside].view(torch.uint8).any()            # zero bits
    torch.cuda.synchronize()
    assert torch.equal(pop.arena[:, : pop.layout.mt_key], snap[:, : pop.layout.mt_key])   # a gather writes nothing
    with pytest.raises(ValueError):
        pop.gather_pool(torch.zeros((P + 1, 4), dtype=torch.int64))


def test_a_poisoned_member_draws_nothing(gpu, built_lib):
    P, M, count = FILLS[0]
    B, K = 64, 32
    pop, _, rings = _fresh(gpu, P, M, count)
    pop.mt_pos[1] = -1
    key = pop.mt_key[1].clone()
    rngs = [np.random.RandomState(x) for x in _seeds(P)]
    for call in range(2):
        got = pop.sample_pool(B, K, as_bool=False)
        want = share_oracle.draw(rngs, P, M, count, B, K, poisoned=(1,))
        torch.cuda.synchronize()
        assert bool((got[5][1] == -1).all()) and int(pop.mt_pos[1]) == -1 and torch.equal(pop.mt_key[1], key)
        for t in got[:5]:
            assert not t[1].view(torch.uint8).any()              # rows outside the pool: zero bits
        assert np.array_equal(got[5].cpu().numpy(), want), f"call {call}"
        _same_bytes(got[:5], share_oracle.gather(rings, want, M), f"call {call}")


def _cfg(m, B, max_size):
    from sacenv.agent import AgentConfig
    return AgentConfig(lr_alpha=0.0015 + 0.001 * m, lr_beta=0.0003 * (m + 2), gamma=0.95 + 0.004 * m,
                       tau=0.002 * (m + 1), reward_scale=2.0 + m, batch_size=B, max_size=max_size)


def test_learn_through_the_pooled_replay(gpu, built_lib):
    """A population that samples its replay with pool rows against one that is handed the
    oracle's batches: the same weights, bit for bit. (B = 256 is the least batch the learn kernels
    take -- a multiple of 256 -- so it stands for the issue's 64.)"""
    from sacenv.population import NativeSACPopulation
    from sacenv.population_replay import PopulationReplay
    P, B, Dn, M = 2, 256, 11, 512
    cfgs = [_cfg(m, B, M) for m in range(P)]
    replay = PopulationReplay(P, M, (Dn,), 1, device=gpu, seeds=[5, 6])
    kw = dict(obs_dim=Dn, init_seeds=[1, 2], noise_seeds=[100, 101])
    pa = NativeSACPopulation(gpu, cfgs, replay=replay, pool_rows=B // 2, **kw)
    pb = NativeSACPopulation(gpu, cfgs, with_memory=False, **kw)
    assert pa.pool_rows == B // 2 and pb.pool_rows == 0
    rngs = [np.random.RandomState(x) for x in (5, 6)]
    g = torch.Generator().manual_seed(2)
    assert pa.learn() is None                                    # fewer than B rows held
    for k in range(3):
        n = 300                                                  # (the second store wraps the ring)
        replay.store_batch(torch.rand((P, n, Dn), generator=g), torch.rand((P, n, 1), generator=g) * 2 - 1,
                           torch.rand((P, n), generator=g), torch.rand((P, n, Dn), generator=g),
                           (torch.rand((P, n), generator=g) < 0.1).to(torch.uint8))
        rings = [getattr(replay, f).cpu().numpy() for f in FIELDS]
        idx = share_oracle.draw(rngs, P, M, replay.mem_cntr, B, B // 2)
        batch = [torch.from_numpy(x).to(gpu) for x in share_oracle.gather(rings, idx, M)]
        la, lb = pa.learn(), pb.learn(batch)
        torch.cuda.synchronize()
        assert la is not None and pa.adam_step == pb.adam_step == k + 1
        assert torch.equal(la.view(torch.int32), lb.view(torch.int32)), f"learn {k}: losses"
        assert torch.equal(pa.weights, pb.weights), f"learn {k}: weights"


def test_the_example_shares_replay(gpu, built_lib, capsys):
    spec = importlib.util.spec_from_file_location("train_population",
                                                  os.path.join(ROOT, "examples", "train_population.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    # (--batch 256, the least the learn kernels take, for the issue's 64: three learns in 6 iterations)
    base = ["--members", "2", "--envs-per-member", "64", "--batch", "256", "--iters", "6"]
    out = {}
    for name, extra in (("plain", []), ("zero", ["--share-replay", "0"]), ("half", ["--share-replay", "128"])):
        torch.manual_seed(1234)
        out[name] = mod.main(base + extra)
    capsys.readouterr()
    a, b, c = out["plain"], out["zero"], out["half"]
    assert "pool_rows" not in a and b["pool_rows"] == 0 and c["pool_rows"] == 128
    assert a["losses"] is not None and a["losses"] == b["losses"] and a["table"] == b["table"]
    assert c["losses"] is not None and len(c["table"]) == 2
    with pytest.raises(SystemExit):
        mod.main(base + ["--share-replay", "257"])
    with pytest.raises(SystemExit):
        mod.main(base + ["--share-replay", "8", "--replay", "members"])
    capsys.readouterr()


def test_host_validation(gpu, built_lib):
    """Refused on the host, before any launch: the arena stays as it was."""
    from sacenv.population import NativeSACPopulation
    from sacenv.population_replay import PopulationReplay
    P, M, count = FILLS[2]
    pop, snap, _ = _fresh(gpu, P, M, count)
    for bad in (-1, 65):
        with pytest.raises(ValueError, match="pool_rows"):
            pop.sample(64, pool_rows=bad)
        with pytest.raises(ValueError, match="pool_rows"):
            pop.sample_pool(64, bad)
    empty = _new(gpu, 2, 64)
    with pytest.raises(ValueError, match="a must be greater than 0"):
        empty.sample(4, pool_rows=2)
    torch.cuda.synchronize()
    assert torch.equal(pop.arena, snap)
    B, MS = 256, 512
    cfgs = [_cfg(m, B, MS) for m in range(2)]
    ok = PopulationReplay(2, MS, (11,), 1, device=gpu)
    for bad in (-1, B + 1):
        with pytest.raises(ValueError, match="pool_rows"):
            NativeSACPopulation(gpu, cfgs, replay=ok, pool_rows=bad)
    for kw in (dict(), dict(with_memory=False), dict(buffer_seeds=[1, 2])):
        with pytest.raises(ValueError, match="PopulationReplay"):
            NativeSACPopulation(gpu, cfgs, pool_rows=B // 2, **kw)
    assert NativeSACPopulation(gpu, cfgs, replay=ok, pool_rows=B).pool_rows == B
