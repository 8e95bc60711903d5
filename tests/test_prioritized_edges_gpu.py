"""The prioritized population replay at its value and size edges (tests/prio_edge_cases.py has the
inputs, tests/test_prioritized_edges_cpu.py what holds for them on the oracle alone):

* ``update_priorities`` against the exact leaf (``prio_oracle.td_leaves_mp``, mpmath) for every
  exponent, one and two critics, the edge values and leaves up to 2^30: exact on decided rows, within
  one unit on the others; every node the exact sum of the device's leaves; ``max_leaf``; a
  ``member_stride`` that is not the batch.
* draws and weights, bit for bit and to 1 f32 ulp, for batches past the 1 024 threads of the weights'
  workgroup (plain and annealed), a total below the batch, one stored row, leaves at the cap (node
  sums past 32 bits on three and four levels), rings of full nodes, and a header total that the
  leaves do not add up to.
"""
import numpy as np
import pytest
import torch

import prio_edge_cases as K
import prio_oracle
import test_prioritized_replay_gpu as base
from test_prioritized_replay_gpu import _new, _rows, _same_state

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. TD leaves against the exact oracle

def _stored(gpu, P, M, n=None, seed=1, **kw):
    """A replay with its first n rows (default: all) stored, and its trees."""
    rep = _new(gpu, P, M, **kw)
    trees = [prio_oracle.Tree(M) for _ in range(P)]
    n = M if n is None else n
    for t in trees:
        t.mark_stored(0, n)
    rep.store_batch(*_rows(P, n, torch.Generator().manual_seed(seed)))
    return rep, trees


def _check_leaves(rep, m, idx, leaf, decided, before, what):
    """Member m's leaves after an update of the distinct rows idx: exact on decided rows, within one
    unit on the others, the other rows as before; every node and the total the exact sums of the
    device's own leaves. Returns the largest distance on an undecided row."""
    lv = rep.levels(m)
    got = lv[0][idx].astype(np.int64)
    diff = np.abs(got - leaf.astype(np.int64))
    und = int((~decided).sum())
    worst = int(diff[~decided].max()) if und else 0
    print(f"{what} member {m}: {und} of {idx.size} undecided, largest |device - exact| on them {worst}, "
          f"on decided rows {int(diff[decided].max())}")
    for i in np.flatnonzero(diff != 0)[:8]:
        print(f"    position {i}: device {got[i]}, exactly {leaf[i]}, decided {decided[i]}")
    assert und <= K.UNDECIDED_CAP * idx.size
    bad = np.flatnonzero(decided & (diff != 0))
    assert bad.size == 0, f"{what} member {m}: decided positions {bad[:8]} give {got[bad[:8]]}, exactly {leaf[bad[:8]]}"
    assert diff.max() <= 1, f"{what} member {m}: an undecided row {diff.max()} units from the exact leaf"
    rest = np.ones(lv[0].size, bool)
    rest[idx] = False
    assert np.array_equal(lv[0][rest], before[rest]), f"{what} member {m}: a row outside the batch moved"
    t = prio_oracle.Tree(lv[0].size)
    t.leaf = [int(v) for v in lv[0]]
    for k, (have, want) in enumerate(zip(lv, t.levels())):
        assert [int(v) for v in have] == want, f"{what} member {m}: level {k}"
    assert rep.total(m) == t.total()
    return worst, got


def _check_max_leaf(rep, m, old, got, leaf, decided, what):
    """``max_leaf``: the maximum of its old value and the leaves written; the exact oracle's where
    every row that can hold the maximum is decided."""
    have = rep.header(m)["max_leaf"]
    assert have == max(old, int(got.max())), what
    if decided[leaf.astype(np.int64) >= int(leaf.max()) - 1].all():
        assert have == max(old, int(leaf.max())), what


@pytest.mark.parametrize("two", [True, False], ids=["two", "one"])
@pytest.mark.parametrize("alpha,eps", K.ALPHA_EPS)
def test_update_priorities_against_the_exact_leaf(gpu, built_lib, alpha, eps, two):
    P, M, B = K.TD_P, K.TD_M, K.TD_ROWS
    rep, _ = _stored(gpu, P, M)
    rep.alpha, rep.eps = alpha, eps
    cases = [K.td_case(alpha, eps, two, m) for m in range(P)]
    idx = np.stack([K.td_rows(m) for m in range(P)])
    before = [rep.levels(m)[0] for m in range(P)]
    assert all((b == prio_oracle.ONE).all() for b in before)
    rep.update_priorities(idx, np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]) if two else None)
    torch.cuda.synchronize()
    for m, (_, _, leaf, decided) in enumerate(cases):
        what = f"alpha {alpha} eps {eps} two {two}"
        _, got = _check_leaves(rep, m, idx[m], leaf, decided, before[m], what)
        _check_max_leaf(rep, m, prio_oracle.ONE, got, leaf, decided, what)
        if alpha > 0:                                             # (the +inf row: the cap, a decided row)
            assert rep.header(m)["max_leaf"] == prio_oracle.CAP and (leaf[: K.EDGES.size] == 1).sum() >= 3


@pytest.mark.parametrize("two", [True, False], ids=["two", "one"])
def test_member_stride_and_max_leaf(gpu, built_lib, two):
    """alpha = 0.6: the members' rows read out of a larger buffer, B + 37 floats apart, with NaN in
    between (the leaves are those of the contiguous tensors); then, on a fresh state, the rows
    without the edge list, so that ``max_leaf`` is a leaf below the cap that came out of the pow."""
    P, M, B, alpha, eps = K.TD_P, K.TD_M, K.TD_ROWS, 0.6, 1e-3
    cases = [K.td_case(alpha, eps, two, m) for m in range(P)]
    idx = np.stack([K.td_rows(m) for m in range(P)])
    rep, _ = _stored(gpu, P, M, alpha=alpha, eps=eps)
    flat, _ = _stored(gpu, P, M, alpha=alpha, eps=eps)
    before = rep.levels(0)[0]
    stride = B + 37
    bufs = []
    for c in (0, 1):
        buf = np.full(P * stride, np.nan, np.float32)
        for m in range(P):
            buf[m * stride: m * stride + B] = K.td_inputs(alpha, eps, m)[c]
        bufs.append(torch.from_numpy(buf).to(gpu))
    rep.update_priorities(idx, bufs[0][:B], bufs[1][:B] if two else None, member_stride=stride)
    flat.update_priorities(idx, np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]) if two else None)
    torch.cuda.synchronize()
    assert torch.equal(rep.prio, flat.prio)
    for m, (_, _, leaf, decided) in enumerate(cases):
        _check_leaves(rep, m, idx[m], leaf, decided, before, f"stride {stride} two {two}")
    # the log-uniform rows alone: two chunks still, the largest leaf below the cap
    E = K.EDGES.size
    rep, _ = _stored(gpu, P, M, alpha=alpha, eps=eps)
    rep.update_priorities(idx[:, E:], np.stack([c[0][E:] for c in cases]),
                          np.stack([c[1][E:] for c in cases]) if two else None)
    torch.cuda.synchronize()
    for m, (_, _, leaf, decided) in enumerate(cases):
        what = f"no edges, two {two}"
        _, got = _check_leaves(rep, m, idx[m, E:], leaf[E:], decided[E:], before, what)
        _check_max_leaf(rep, m, prio_oracle.ONE, got, leaf[E:], decided[E:], what)
        assert 1 << 26 < rep.header(m)["max_leaf"] < prio_oracle.CAP


# ---------------------------------------------------------------- 2. draws and weights at the size edges

def _check_sample(rep, trees, B, safe, seeds, descend=True, what=""):
    """One sample against the oracle: idx and leaf bit for bit, weights within 1 f32 ulp of
    (min leaf / leaf)^beta_at(the sample's number); the gathered rows are ``gather``'s."""
    call = trees[0].calls if safe else rep.sample_calls
    got = rep.sample(B, as_bool=False, graph_safe=safe)
    torch.cuda.synchronize()
    idx, leaf, w = got[5].cpu().numpy(), rep.last_leaf.cpu().numpy().view(np.uint32), rep.last_weights.cpu().numpy()
    wants, worst = [], 0
    for m, t in enumerate(trees):
        want = t.draw(B, call, m, seeds[m], descend=descend)
        assert np.array_equal(idx[m], want[0]), f"{what} B {B} call {call} member {m}: idx"
        assert np.array_equal(leaf[m], want[1]), f"{what} B {B} call {call} member {m}: leaf"
        ulps = prio_oracle.ulp_distance_f32(w[m], prio_oracle.weights(want[1], rep.beta_at(call)))
        worst = max(worst, int(ulps.max()))
        assert ulps.max() <= 1, f"{what} B {B} call {call} member {m}: a weight {ulps.max()} ulp off"
        if safe:
            t.calls += 1
        wants.append(want)
    print(f"{what} B {B} call {call} safe {safe}: worst weight {worst} ulp")
    again = rep.gather(got[5], as_bool=False)
    for u, v in zip(got[:5], again):
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
    return wants, w


def _big(gpu, **kw):
    P, M = K.BIG_P, K.BIG_M
    rep, trees = _stored(gpu, P, M, prio_seeds=list(K.BIG_SEEDS), **kw)
    leaf = np.stack([K.big_fill(m) for m in range(P)])
    for m, t in enumerate(trees):
        t.set(np.arange(M), leaf[m])
    rep.set_priorities(np.tile(np.arange(M), (P, 1)), leaf)
    _same_state(rep, trees, "big fill")
    return rep, trees


def test_batches_past_one_stride_of_the_weights_workgroup(gpu, built_lib):
    """B = 1 025, 2 048 and 2 500 on a fill whose small leaves are drawn by the last slots only: the
    batch's minimum lies past position 1 023, and has to survive the strides of 1 024 threads and
    the reduction through LDS to reach every weight."""
    rep, trees = _big(gpu)
    for B in K.BIG_BATCHES:
        for safe in (False, False, True, True):
            assert (B, trees[0].calls if safe else rep.sample_calls) in K.BIG_DRAWS
            wants, w = _check_sample(rep, trees, B, safe, K.BIG_SEEDS, what="big")
            for m, want in enumerate(wants):
                assert int(np.argmin(want[1])) >= 1024
                assert not np.array_equal(w[m], K.weights_first_stride(want[1], rep.beta))
    assert rep.sample_calls == 2 * len(K.BIG_BATCHES) == rep.header(1)["calls"]
    _same_state(rep, trees, "after the big draws")


def test_annealed_weights_past_one_stride(gpu, built_lib):
    """The same fill under ``beta_final = 1, beta_anneal = 3``: four device-counted samples of 2 048,
    the weights' exponent beta_at(0..3), the last one clamped."""
    rep, trees = _big(gpu, beta_final=1.0, beta_anneal=3)
    assert [rep.beta_at(k) for k in (0, 3, 4)] == [0.4, 1.0, 1.0] and 0.4 < rep.beta_at(1) < rep.beta_at(2) < 1.0
    seen = []
    for k in range(4):
        assert rep.header(0)["calls"] == k and (2048, k) in K.ANNEALED_DRAWS
        wants, w = _check_sample(rep, trees, 2048, True, K.BIG_SEEDS, what="annealed")
        for m, want in enumerate(wants):
            assert int(np.argmin(want[1])) >= 1024
            assert not np.array_equal(w[m], K.weights_first_stride(want[1], rep.beta_at(k)))
        seen.append(w)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[2], seen[3])   # (other draws, too)


@pytest.mark.parametrize("B", [33, 64, 256])
def test_a_total_below_the_batch(gpu, built_lib, B):
    """T = 6 < B: B - 6 strata are empty and draw t = lo_j."""
    P, M = 2, 100
    rep, trees = _stored(gpu, P, M, n=5, prio_seeds=[3, 4])
    for t in trees:
        t.set(np.arange(5), (1, 1, 2, 1, 1))
    rep.set_priorities(np.tile(np.arange(5), (P, 1)), np.tile((1, 1, 2, 1, 1), (P, 1)))
    _same_state(rep, trees, "five rows")
    assert rep.total(0) == 6 == trees[0].total()
    assert sum(lo == hi for lo, hi in (prio_oracle.stratum(6, B, j) for j in range(B))) == B - 6
    for safe in (False, True):
        wants, _ = _check_sample(rep, trees, B, safe, [3, 4], what="T < B")
        for want in wants:
            assert ((want[0] >= 0) & (want[0] < 5)).all() and set(want[0].tolist()) == set(range(5))


def test_one_stored_row(gpu, built_lib):
    P, M, B = 2, 4097, 256
    rep, trees = _stored(gpu, P, M, n=1, prio_seeds=[3, 4])
    for t in trees:
        t.set([0], [1])
    rep.set_priorities(np.zeros((P, 1), np.int64), np.ones((P, 1), np.int64))
    _same_state(rep, trees, "one row")
    assert rep.total(1) == 1
    for safe in (False, True):
        _check_sample(rep, trees, B, safe, [3, 4], what="one row")
        assert not rep.last_idx.any() and bool((rep.last_leaf == 1).all()) and bool((rep.last_weights == 1.0).all())


def test_leaves_at_the_cap_three_levels(gpu, built_lib):
    """Level-1 sums of 37 bits and a total of 43: the draw's scan, ballot and hand-off past 32 bits."""
    P, M, B = 2, 4097, 256
    rep, trees = _stored(gpu, P, M, prio_seeds=[3, 4])
    leaf = np.stack([K.cap_fill(m) for m in range(P)])
    for m, t in enumerate(trees):
        t.set(np.arange(M), leaf[m])
    rep.set_priorities(np.tile(np.arange(M), (P, 1)), leaf)
    _same_state(rep, trees, "cap fill")
    assert max(trees[0].levels()[1]).bit_length() == 37 and rep.total(0).bit_length() == 43
    for safe in (False, False, True, True):
        wants, _ = _check_sample(rep, trees, B, safe, [3, 4], what="cap")
        assert all(prio_oracle.CAP in want[1] for want in wants)


def test_leaves_at_the_cap_four_levels(gpu, built_lib):
    """M = 64^3 + 1 with the cap on every row (one row set to it, then the stores mark all rows with
    ``max_leaf``): level sums of 37, 43 and 49 bits, a total near 2^49; then 5 000 smaller leaves, so
    that the rows are not all alike. Bytes, and two draws of 256 found in the running sum."""
    P, M, B = 1, 64 ** 3 + 1, 256
    rep = _new(gpu, P, M, prio_seeds=[9])
    trees = [prio_oracle.Tree(M)]
    trees[0].set([7], [prio_oracle.CAP])
    rep.set_priorities([[7]], [[prio_oracle.CAP]])
    g = torch.Generator().manual_seed(3)
    for n in (200000, M - 200000):
        trees[0].mark_stored(rep.mem_cntr, n)
        rep.store_batch(*_rows(P, n, g))
    assert trees[0].total() == M * prio_oracle.CAP == rep.total(0) and rep.total(0).bit_length() == 50
    rng = np.random.default_rng(3)
    idx, leaf = rng.integers(0, M, (P, 5000)), rng.integers(1, 1 << 31, (P, 5000))
    trees[0].set(idx[0], leaf[0])
    rep.set_priorities(idx, leaf)
    _same_state(rep, trees, "four levels at the cap")
    assert [max(lv).bit_length() for lv in trees[0].levels()[1:]] == [37, 43, 49]
    for _ in range(2):
        _check_sample(rep, trees, B, False, [9], descend=False, what="cap, four levels")


FULL = [(2, 128), (1, 4096)]          # every node full; 4 096: a top level of exactly 64 entries


@pytest.mark.parametrize("P,M", FULL)
def test_tree_bytes_of_full_nodes(gpu, built_lib, P, M):
    assert prio_oracle.level_counts(M)[-1] * 64 == M
    base.test_tree_bytes(gpu, built_lib, P, M)


@pytest.mark.parametrize("P,M", FULL)
def test_draw_of_full_nodes(gpu, built_lib, P, M):
    base.test_draw(gpu, built_lib, P, M)


@pytest.mark.parametrize("M", [64, 4097])
def test_a_tree_that_does_not_add_up(gpu, built_lib, M):
    """Member 0's header total doubled by a caller's own write: a slot whose t reaches past the
    leaves' sum finds no child at the top level (``hit == 0``) and gives idx -1, leaf 0 and zero
    gathered bits; the other slots and member 1 are the oracle's."""
    P, B, seeds = 2, 256, [3, 4]
    rep, trees = _stored(gpu, P, M, prio_seeds=seeds)
    leaf = np.random.default_rng(M).integers(1, 1 << 22, (P, M))
    for m, t in enumerate(trees):
        t.set(np.arange(M), leaf[m])
    rep.set_priorities(np.tile(np.arange(M), (P, 1)), leaf)
    _same_state(rep, trees, "fill")
    T = trees[0].total()
    rep.prio[0, :8] = torch.from_numpy(np.frombuffer(np.uint64(2 * T).tobytes(), np.uint8).copy()).to(gpu)
    assert rep.total(0) == 2 * T and rep.total(1) == trees[1].total()
    snap = rep.prio.clone()
    got = rep.sample(B, as_bool=False)
    torch.cuda.synchronize()
    idx, lf, w = got[5].cpu().numpy(), rep.last_leaf.cpu().numpy().view(np.uint32), rep.last_weights.cpu().numpy()
    want = trees[0].draw(B, 0, 0, seeds[0], total=2 * T)
    past = np.array([t >= T for t in want[2]])
    assert 0 < past.sum() < B and (want[0][past] == -1).all() and (want[1][past] == 0).all()
    assert np.array_equal(idx[0], want[0]) and np.array_equal(lf[0], want[1])
    for t_ in got[:5]:
        assert not t_[0][torch.from_numpy(past).to(gpu)].view(torch.uint8).any()
    hit = torch.from_numpy(~past).to(gpu)
    for u, v in zip(got[:5], rep.gather(got[5], as_bool=False)):
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)) and u[0][hit].view(torch.uint8).any()
    other = trees[1].draw(B, 0, 1, seeds[1])
    assert np.array_equal(idx[1], other[0]) and np.array_equal(lf[1], other[1])
    for m in range(P):                                            # (member 0: the least leaf is 0, every weight 0)
        assert prio_oracle.ulp_distance_f32(w[m], prio_oracle.weights(lf[m], rep.beta)).max() <= 1
    assert not w[0].any() and w[1].all()
    assert torch.equal(rep.prio, snap)                            # (a host-numbered sample writes no state)
