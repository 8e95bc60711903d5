"""The prioritized population replay on the device against its restatement on Python ints
(include/sacenv_prioritized_replay.h, sacenv/prioritized.py, tests/prio_oracle.py): the state's
bytes after init, mark, set and update; every drawn index and leaf; the TD path behind a real learn;
and that nothing changes for a replay that is not prioritized.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import prio_oracle
from conftest import ROOT

pytestmark = pytest.mark.gpu

D = 11
SHAPES = [(1, 64), (3, 65), (2, 100), (2, 4097), (64, 130)]      # (P, M): leaves only; 65 = one past a node;
BATCHES = (1, 33, 64, 256)                                        # three levels; the most members


def _seeds(P):
    return [1000 + 7 * m for m in range(P)]


def _new(gpu, P, M, cls=None, **kw):
    from sacenv.prioritized import PrioritizedPopulationReplay
    return (cls or PrioritizedPopulationReplay)(P, M, (D,), 1, device=gpu, seeds=list(range(P)), **kw)


def _rows(P, n, g):
    return (torch.rand((P, n, D), generator=g), torch.rand((P, n, 1), generator=g) * 2 - 1,
            torch.rand((P, n), generator=g), torch.rand((P, n, D), generator=g),
            (torch.rand((P, n), generator=g) < 0.1).to(torch.uint8))


def _same_state(rep, trees, what):
    torch.cuda.synchronize()
    got = rep.prio.cpu().numpy()
    for m, t in enumerate(trees):
        want = np.frombuffer(t.to_bytes(), np.uint8)
        assert got[m].size == want.size, what
        bad = np.flatnonzero(got[m] != want)
        assert bad.size == 0, f"{what}: member {m}, first byte {bad[:4]} of {want.size}"


def _fill(gpu, P, M, seed=0):
    """A replay and its trees after two stores (a partly filled ring, then one on the device
    counts) and an explicit set: distinct priorities on many rows."""
    rep = _new(gpu, P, M, prio_seeds=_seeds(P))
    trees = [prio_oracle.Tree(M) for _ in range(P)]
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    for n, safe in ((M // 3 + 1, False), (M // 2, True)):
        for t in trees:
            t.mark_stored(rep.mem_cntr, n)
        rep.store_batch(*_rows(P, n, g), graph_safe=safe)
    B = 96
    idx = rng.integers(0, min(rep.mem_cntr, M), (P, B))
    leaf = rng.integers(1, 1 << 22, (P, B))
    for m, t in enumerate(trees):
        t.set(idx[m], leaf[m])
    rep.set_priorities(idx, leaf)
    return rep, trees


@pytest.mark.parametrize("P,M", SHAPES)
def test_tree_bytes(gpu, built_lib, P, M):
    from sacenv import PopulationReplay
    rep = _new(gpu, P, M)
    plain = _new(gpu, P, M, cls=PopulationReplay)
    trees = [prio_oracle.Tree(M) for _ in range(P)]
    L = rep.prio_layout
    assert L.levels == prio_oracle.layout(M)["levels"] and rep.prio.shape == (P, prio_oracle.layout(M)["member_bytes"])
    _same_state(rep, trees, "init")
    g = torch.Generator().manual_seed(M)
    rng = np.random.default_rng(M)
    # a partly filled ring, a store that wraps it, one with n > M, one on the device counts
    for k, (n, safe) in enumerate(((M // 3 + 1, False), (M - M // 5, True), (2 * M + 5, False), (7, True))):
        for t in trees:
            t.mark_stored(rep.mem_cntr, n)
        rows = _rows(P, n, g)
        rep.store_batch(*rows, graph_safe=safe)
        plain.store_batch(*rows, graph_safe=safe)
        _same_state(rep, trees, f"store {k}")
        if k == 0:
            stored = rep.levels(0)[0] != 0
            assert stored[: n].all() and not stored[n:].any()     # leaf 0 exactly for the rows never stored
    torch.cuda.synchronize()
    assert torch.equal(rep.arena, plain.arena)                    # the arena is a plain PopulationReplay's
    # explicit leaves: duplicates (the last wins), rows outside the ring, leaves outside [1, 2^31 - 1]
    for B in (5, 300, 1500 if M > 1000 else 70):                  # (1 500: two chunks of the writing workgroup)
        idx = rng.integers(-3, M + 3, (P, B))
        idx[:, : min(B, 4)] = [[-1, M, 1 << 40, M - 1][: min(B, 4)]] * P
        idx[:, B // 2:] = idx[:, : B - B // 2]                    # every row of the first half named again
        leaf = rng.integers(0, 1 << 24, (P, B))
        leaf[:, -1], leaf[:, 0] = (1 << 32) - 1, 0
        if B > 8:
            idx[:, -1], idx[:, -2], idx[:, -3] = 3, 3, 5
            leaf[:, -2], leaf[:, -3] = 12345, 0
        for m, t in enumerate(trees):
            t.set(idx[m], leaf[m])
        rep.set_priorities(idx, leaf)
        _same_state(rep, trees, f"set {B}")
    assert rep.header(0)["max_leaf"] == prio_oracle.CAP == trees[0].max_leaf
    # new rows enter at the largest priority so far
    for t in trees:
        t.mark_stored(rep.mem_cntr, 3)
    rep.store_batch(*_rows(P, 3, g))
    _same_state(rep, trees, "store after set")
    # TD errors, alpha = 1 (pow(a, 1) is a on the host and within an ulp of it on the device, which shows
    # only where a x 65536 is an integer: tests/test_prioritized_edges_gpu.py), with the edge values
    rep.alpha, rep.eps = 1.0, 1e-3
    B = 130
    idx = rng.integers(-1, M + 1, (P, B))
    sq1 = (rng.random((P, B)) * 4).astype(np.float32)
    sq2 = (rng.random((P, B)) * 9).astype(np.float32)
    sq1[:, :5] = [np.nan, np.inf, 0.0, -1.0, 1e30]
    idx[:, :5] = np.arange(5) % M
    for two in (True, False):
        for m, t in enumerate(trees):
            t.update_td(idx[m], sq1[m], sq2[m] if two else None, 1.0, 1e-3)
        rep.update_priorities(idx, sq1, sq2 if two else None)
        _same_state(rep, trees, f"update_td two={two}")
    lv = rep.levels(P - 1)
    assert [a.size for a in lv] == prio_oracle.level_counts(M) and rep.total(P - 1) == trees[P - 1].total()


@pytest.mark.parametrize("P,M", SHAPES)
def test_draw(gpu, built_lib, P, M):
    rep, trees = _fill(gpu, P, M, seed=P + M)
    _same_state(rep, trees, "fill")
    for B in BATCHES:
        for safe in (False, False, True, True):                   # two consecutive calls each, host call and device calls
            call = trees[0].calls if safe else rep.sample_calls   # (the device numbers its own samples)
            got = rep.sample(B, as_bool=False, graph_safe=safe)
            torch.cuda.synchronize()
            idx, leaf, w = got[5].cpu().numpy(), rep.last_leaf.cpu().numpy().view(np.uint32), rep.last_weights.cpu().numpy()
            for m, t in enumerate(trees):
                want = t.draw(B, call, m, _seeds(P)[m], descend=(P <= 3))
                assert np.array_equal(idx[m], want[0]), f"B {B} call {call} member {m}: idx"
                assert np.array_equal(leaf[m], want[1]), f"B {B} call {call} member {m}: leaf"
                assert (want[1] > 0).all()
                assert prio_oracle.ulp_distance_f32(w[m], prio_oracle.weights(want[1], rep.beta)).max() <= 1
                if safe:
                    t.calls += 1
            again = rep.gather(got[5], as_bool=False)
            for u, v in zip(got[:5], again):
                assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
    assert rep.sample_calls == 2 * len(BATCHES)
    _same_state(rep, trees, "after the draws")                    # (only `calls` moved: twice per B)
    assert rep.header(0)["calls"] == 2 * len(BATCHES)


def test_max_leaf_follows_the_winners(gpu, built_lib):
    """``max_leaf`` on a fresh state (65 536, far from the cap), exactly: a batch of two chunks of
    the writing workgroup whose largest leaf sits in the first chunk on a row that the second chunk
    names again, the same in one chunk, and TD updates (alpha = 1, finite values) in one and in two
    chunks."""
    P, M = 2, 4097
    rep = _new(gpu, P, M)
    trees = [prio_oracle.Tree(M) for _ in range(P)]
    rng = np.random.default_rng(11)
    for B, a, b in ((1500, 0, 1024), (1500, 1023, 1499), (700, 3, 650), (2100, 1030, 2050)):
        idx = rng.integers(0, M, (P, B))
        leaf = rng.integers(1, 60000, (P, B))              # below max_leaf's 65 536 at init
        big = trees[0].max_leaf + 5000
        idx[:, a] = idx[:, b] = 77                         # position a loses to position b, chunks apart or not
        leaf[:, a], leaf[:, b] = big, 10
        want = max(trees[0].max_leaf, int(leaf[0][np.arange(B) != a].max()))
        for m, t in enumerate(trees):
            t.set(idx[m], leaf[m])
        rep.set_priorities(idx, leaf)
        _same_state(rep, trees, f"set {B} {a} {b}")
        assert rep.header(0)["max_leaf"] == trees[0].max_leaf < big and trees[0].max_leaf >= want
        assert rep.levels(0)[0][77] == 10
    # a winner above the old value moves it
    idx, leaf = rng.integers(0, M, (P, 1500)), rng.integers(1, 60000, (P, 1500))
    idx[:, 5] = idx[:, 1400] = 99
    leaf[:, 5], leaf[:, 1400] = 10, 200000
    for m, t in enumerate(trees):
        t.set(idx[m], leaf[m])
    rep.set_priorities(idx, leaf)
    _same_state(rep, trees, "set, a late winner")
    assert rep.header(1)["max_leaf"] == 200000
    # TD updates drive it, exactly: alpha = 1, sqrt(sq) * 65536 up to 8 x 65536
    rep.alpha, rep.eps = 1.0, 0.0
    for B in (300, 1500):
        idx = rng.integers(0, M, (P, B))
        sq1 = (rng.random((P, B)) * 16).astype(np.float32)
        sq2 = (rng.random((P, B)) * 16).astype(np.float32)
        idx[:, 2] = idx[:, B - 3] = 55                     # the largest TD error loses its row
        sq1[:, 2] = sq2[:, 2] = np.float32(64.0 + B)
        for m, t in enumerate(trees):
            t.update_td(idx[m], sq1[m], sq2[m], 1.0, 0.0)
        rep.update_priorities(idx, sq1, sq2)
        _same_state(rep, trees, f"update_td {B}")
        assert 200000 < rep.header(0)["max_leaf"] == trees[0].max_leaf < int(np.sqrt(64.0 + B) * 65536)
        rep.alpha, rep.eps = 1.0, 0.0


def test_four_levels(gpu, built_lib):
    """M = 262 145: the least ring with four levels, so that ``k_prio_upper`` builds level 3 from the
    level 2 it has just written and the draw walks four levels. Bytes and draws against the oracle
    (the rows found in the leaves' running sum)."""
    P, M, B = 1, 64 ** 3 + 1, 256
    assert prio_oracle.level_counts(M) == [M, 4097, 65, 2]
    rep = _new(gpu, P, M, prio_seeds=_seeds(P))
    trees = [prio_oracle.Tree(M)]
    g = torch.Generator().manual_seed(3)
    rng = np.random.default_rng(3)
    for n in (200000, 70000):                              # the second store wraps the ring
        trees[0].mark_stored(rep.mem_cntr, n)
        rep.store_batch(*_rows(P, n, g))
    idx, leaf = rng.integers(0, M, (P, 5000)), rng.integers(1, 1 << 24, (P, 5000))
    trees[0].set(idx[0], leaf[0])
    rep.set_priorities(idx, leaf)
    _same_state(rep, trees, "four levels")
    for call in range(2):
        got = rep.sample(B, as_bool=False)
        torch.cuda.synchronize()
        want = trees[0].draw(B, call, 0, _seeds(P)[0], descend=False)
        assert np.array_equal(got[5][0].cpu().numpy(), want[0]), f"call {call}"
        assert np.array_equal(rep.last_leaf[0].cpu().numpy().view(np.uint32), want[1])
    want = trees[0].draw(64, 2, 0, _seeds(P)[0], descend=True)       # and the walk down the four levels
    got = rep.sample(64, as_bool=False)
    assert np.array_equal(got[5][0].cpu().numpy(), want[0])


def test_an_empty_tree_draws_nothing(gpu, built_lib):
    rep = _new(gpu, 2, 100)
    rep.mem_cntr = 5                                              # (rows the priorities never heard of)
    got = rep.sample(33, as_bool=False)
    torch.cuda.synchronize()
    assert bool((got[5] == -1).all()) and not rep.last_leaf.any() and not rep.last_weights.any()
    for t in got[:5]:
        assert not t.view(torch.uint8).any()


def _cfg(m, B, max_size):
    from sacenv.agent import AgentConfig
    return AgentConfig(lr_alpha=0.0015 + 0.001 * m, lr_beta=0.0003 * (m + 2), gamma=0.95 + 0.004 * m,
                       tau=0.002 * (m + 1), reward_scale=2.0 + m, batch_size=B, max_size=max_size)


def test_td_path_behind_a_real_learn(gpu, built_lib):
    """``NativeSACPopulation.learn`` on a prioritized replay, P = 2, M = 1024. (B = 256 is the least
    batch the learn kernels take -- a multiple of 256 -- so it stands for the issue's 64.) The
    leaves are held against the exact ones (``prio_oracle.td_leaves_mp``): equal on every decided
    row, within one unit on a row whose value lies within 2^-44 of an integer, of which there may
    be 1 % at the most."""
    from sacenv.population import NativeSACPopulation
    P, B, M = 2, 256, 1024
    rep = _new(gpu, P, M, prio_seeds=_seeds(P))
    pop = NativeSACPopulation(gpu, [_cfg(m, B, M) for m in range(P)], replay=rep, obs_dim=D, init_seeds=[1, 2],
                              noise_seeds=[100, 101])
    g = torch.Generator().manual_seed(9)
    assert pop.learn() is None and rep.last_idx is None
    for k in range(3):
        rep.store_batch(*_rows(P, 300, g))
        before = [rep.levels(m)[0] for m in range(P)]
        hdr = [rep.header(m) for m in range(P)]
        assert pop.learn() is not None
        torch.cuda.synchronize()
        sq1, sq2, stride = rep.learn_rows(pop)
        idx = rep.last_idx.cpu().numpy()
        scratch = pop.scratch.cpu().numpy()
        o1, o2 = sq1.storage_offset(), sq2.storage_offset()
        assert stride * 4 == pop.pop_layout.scratch_bytes and o2 == o1 + B
        moved = 0
        for m in range(P):
            t = prio_oracle.Tree(M)
            t.leaf, t.max_leaf = [int(v) for v in before[m]], hdr[m]["max_leaf"]
            a, b = scratch[m * stride + o1:][:B], scratch[m * stride + o2:][:B]
            assert np.isfinite(a).all() and (a >= 0).all() and (a > 0).any() and not np.array_equal(a, b)
            # the exact leaves (mpmath); of equal rows the highest position wins, with its `decided`
            exact, decided = prio_oracle.td_leaves_mp(a, b, rep.alpha, rep.eps)
            assert (~decided).sum() <= 0.01 * B
            t.set(idx[m], exact)
            sure = np.ones(M, bool)
            for i, d in zip(idx[m], decided):
                sure[i] = d
            lv = rep.levels(m)
            diff = np.abs(lv[0].astype(np.int64) - np.array(t.leaf, np.int64))
            assert not diff[sure].any(), f"learn {k} member {m}: a decided leaf {diff[sure].max()} units from the exact one"
            assert diff.max() <= 1, f"learn {k} member {m}: a leaf {diff.max()} units from the exact one"
            # max_leaf: exact where every written row that can hold the maximum is decided
            top = [i for i in set(idx[m].tolist()) if t.leaf[i] >= max(t.leaf[j] for j in idx[m]) - 1]
            if sure[top].all():
                assert rep.header(m)["max_leaf"] == t.max_leaf
            assert abs(rep.header(m)["max_leaf"] - t.max_leaf) <= 1
            moved += int((lv[0] != before[m]).sum())
            # every internal node is the exact sum of the device's own leaves
            t.leaf = [int(v) for v in lv[0]]
            for k_, (have, want) in enumerate(zip(lv, t.levels())):
                assert [int(v) for v in have] == want, f"level {k_}"
            assert rep.total(m) == t.total()
        assert moved > P * B // 2                                 # the sampled rows took new priorities
    # a draw on the device's leaves, and its weights
    trees = []
    for m in range(P):
        t = prio_oracle.Tree(M)
        t.leaf = [int(v) for v in rep.levels(m)[0]]
        trees.append(t)
    call = rep.sample_calls
    got = rep.sample(B, as_bool=False)
    torch.cuda.synchronize()
    leaf = rep.last_leaf.cpu().numpy().view(np.uint32)
    for m, t in enumerate(trees):
        want = t.draw(B, call, m, _seeds(P)[m])
        assert np.array_equal(got[5][m].cpu().numpy(), want[0]) and np.array_equal(leaf[m], want[1])
        ulps = prio_oracle.ulp_distance_f32(rep.last_weights[m].cpu().numpy(), prio_oracle.weights(want[1], rep.beta))
        assert ulps.max() <= 1, ulps.max()
        assert len(set(want[1].tolist())) > 8                     # (weights of many different leaves)


def test_no_change_without_it(gpu, built_lib):
    """A plain ``PopulationReplay`` under ``NativeSACPopulation.learn`` (which now looks at its
    replay's type) against the unchanged path -- the same replay sampled by hand and the batch handed
    to the core's learn -- over 20 iterations: the same weights, losses and arena, bit for bit."""
    from sacenv import PopulationReplay
    from sacenv.population import NativeSACPopulation
    from sacenv.sac_native import _SacCore
    P, B, M, n = 2, 256, 1024, 96
    cfgs = [_cfg(m, B, M) for m in range(P)]
    kw = dict(obs_dim=D, init_seeds=[1, 2], noise_seeds=[100, 101])
    ra, rb = (PopulationReplay(P, M, (D,), 1, device=gpu, seeds=[5, 6]) for _ in range(2))
    pa = NativeSACPopulation(gpu, cfgs, replay=ra, **kw)
    pb = NativeSACPopulation(gpu, cfgs, with_memory=False, **kw)
    assert pa._prioritized is False
    g = torch.Generator().manual_seed(4)
    learns = 0
    for it in range(20):
        rows = _rows(P, n, g)
        ra.store_batch(*rows)
        rb.store_batch(*rows)
        la = pa.learn()
        lb = None if rb.mem_cntr < B else _SacCore.learn(pb, rb.sample(B, as_bool=False)[:5])
        assert (la is None) == (lb is None)
        if la is not None:
            learns += 1
            assert torch.equal(la.view(torch.int32), lb.view(torch.int32)), f"iteration {it}: losses"
    torch.cuda.synchronize()
    assert learns == 18 and pa.adam_step == pb.adam_step == learns
    assert torch.equal(pa.weights, pb.weights) and torch.equal(ra.arena, rb.arena)
    # and a prioritized replay's arena after the same stores is the plain one's
    rc = _new(gpu, P, M)
    rd = PopulationReplay(P, M, (D,), 1, device=gpu, seeds=list(range(P)))
    g = torch.Generator().manual_seed(4)
    for it in range(20):
        rows = _rows(P, n, g)
        rc.store_batch(*rows, graph_safe=bool(it & 1))
        rd.store_batch(*rows, graph_safe=bool(it & 1))
    rc.sample(B)
    torch.cuda.synchronize()
    assert torch.equal(rc.arena, rd.arena)                        # (a prioritized sample leaves the MT stream alone)


def test_the_example_runs_prioritized(gpu, built_lib, capsys):
    spec = importlib.util.spec_from_file_location("train_population",
                                                  os.path.join(ROOT, "examples", "train_population.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    # (--batch 256, the least the learn kernels take: 27 learns in 30 iterations)
    base = ["--members", "2", "--envs-per-member", "64", "--batch", "256", "--iters", "30"]
    torch.manual_seed(1234)
    plain = mod.main(base)
    torch.manual_seed(1234)
    out = mod.main(base + ["--prioritized"])
    torch.manual_seed(1234)
    other = mod.main(base + ["--prioritized", "0.3"])
    capsys.readouterr()
    assert "prioritized" not in plain
    assert out["prioritized"]["alpha"] == 0.6 and other["prioritized"]["alpha"] == 0.3
    assert out["prioritized"]["beta"] == 0.4 and len(out["prioritized"]["totals"]) == 2
    assert all(t > 0 for t in out["prioritized"]["totals"])
    assert out["losses"] is not None and np.isfinite(np.array(out["losses"])).all() and len(out["table"]) == 2
    assert out["losses"] != plain["losses"]                       # other rows were learnt from
    for bad in (["--prioritized", "--replay", "members"], ["--prioritized", "--share-replay", "8"],
                ["--prioritized", "-1"]):
        with pytest.raises(SystemExit):
            mod.main(base + bad)
    capsys.readouterr()


def test_host_validation(gpu, built_lib):
    from sacenv.population import NativeSACPopulation
    rep, _ = _fill(gpu, 2, 100)
    snap = rep.prio.clone()
    with pytest.raises(ValueError, match="pool_rows"):
        rep.sample(8, pool_rows=2)
    with pytest.raises(ValueError, match="idx must be"):
        rep.set_priorities(torch.zeros((3, 4), dtype=torch.int64), torch.ones((3, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match="shape"):
        rep.set_priorities(torch.zeros((2, 4), dtype=torch.int64), torch.ones((2, 5), dtype=torch.int64))
    with pytest.raises(ValueError, match="shape"):
        rep.update_priorities(torch.zeros((2, 4), dtype=torch.int64), torch.ones((2, 5)))
    with pytest.raises(ValueError, match="prio_seeds"):
        _new(gpu, 2, 100, prio_seeds=[1])
    torch.cuda.synchronize()
    assert torch.equal(rep.prio, snap)
    B, M = 256, 512
    ok = _new(gpu, 2, M)
    with pytest.raises(ValueError, match="pool_rows"):
        NativeSACPopulation(gpu, [_cfg(m, B, M) for m in range(2)], replay=ok, pool_rows=8)
    with pytest.raises(RuntimeError, match="follows a sample"):
        ok.update_from_learn(NativeSACPopulation(gpu, [_cfg(m, B, M) for m in range(2)], replay=ok))
