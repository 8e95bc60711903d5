"""What tests/test_prioritized_edges_gpu.py relies on, established on the oracle alone
(tests/prio_oracle.py, tests/prio_edge_cases.py):

* the exact TD leaf (mpmath) at the special values, and numpy's f64 restatement equal to it on every
  decided row of every input set, with at most 1 % of an input set's rows undecided;
* the bar has teeth: a pow carried out in float32, and a round-to-nearest in place of the floor, move
  hundreds of 2 000 leaves that reach up to 2^30;
* on the big batches the smallest drawn leaf lies past position 1 023, and weights from the minimum
  of the first 1 024 positions differ from the oracle's;
* a total below the batch draws the five stored rows only; a header total that the leaves do not
  add up to gives idx -1 exactly for the slots whose t reaches past the leaves' sum.
"""
import numpy as np
import pytest

import prio_edge_cases as K
import prio_oracle
from prio_oracle import CAP, ONE


def test_exact_leaf_at_the_special_values():
    f = np.float32
    sq = np.array([np.nan, -1.0, -np.inf, -1e-45, -0.0, 0.0, np.inf, 1.0, 4.0, 2.0 ** -32], f)
    for alpha in (0.3, 0.6, 1.0, 2.0):
        leaf, decided = prio_oracle.td_leaves_mp(sq, None, alpha, 0.0)
        assert list(leaf[:7]) == [1, 1, 1, 1, 1, 1, CAP] and decided[:7].all()
        assert leaf[7] == ONE and not decided[7]                     # (1^alpha x 65536: on an integer)
        leaf, decided = prio_oracle.td_leaves_mp(sq, sq[::-1].copy(), alpha, 1e-3)
        assert list(leaf[:4]) == [1, 1, 1, 1] and leaf[6] == 1 and decided[:4].all()   # (inf beside -1: NaN first)
    leaf, decided = prio_oracle.td_leaves_mp(sq, None, 0.0, 0.0)
    assert list(leaf) == [1, 1, 1, 1] + [ONE] * 6 and decided.all()   # pow(0, 0) = pow(inf, 0) = 1
    # exact values: (0.5 (2 + 4) + 1)^0.5 = 2; sqrt(2^-32) x 65536 = 1, the lower threshold, from both sides
    leaf, decided = prio_oracle.td_leaves_mp(f([4.0]), f([16.0]), 0.5, 1.0)
    assert leaf[0] == 2 * ONE and not decided[0]
    lo, hi = np.nextafter(f(2.0 ** -32), f(0)), np.nextafter(f(2.0 ** -32), f(1))
    leaf, decided = prio_oracle.td_leaves_mp(f([lo, 2.0 ** -32, hi]), None, 1.0, 0.0)
    assert list(leaf) == [1, 1, 1] and list(decided) == [True, False, True]
    # the cap: sqrt(2^30) x 65536 = 2^31 is capped either way and undecided by the rule; far past it, decided
    leaf, decided = prio_oracle.td_leaves_mp(f([2.0 ** 30, 1e19, K.FLT_MAX]), None, 1.0, 0.0)
    assert list(leaf) == [CAP, CAP, CAP] and list(decided) == [False, True, True]
    # a value 2^-40 s below an integer is decided at 160 bits, and floors to the integer below
    leaf, decided = prio_oracle.td_leaves_mp(f([1.0]), None, 1.0, float(np.nextafter(1.0, 2.0)) - 1.0)
    assert leaf[0] == ONE and not decided[0]                         # (1 + 2^-52) x 65536: inside the margin
    leaf, decided = prio_oracle.td_leaves_mp(f([1.0 - 2.0 ** -24]), None, 1.0, 0.0)
    assert leaf[0] == ONE - 1 and decided[0]                         # sqrt(1 - 2^-24) x 65536 = 65536 - 2^-9


SETS = [(a, e, two) for a, e in K.ALPHA_EPS for two in (True, False)]


@pytest.mark.parametrize("alpha,eps,two", SETS)
def test_numpy_leaves_are_exact_on_decided_rows(alpha, eps, two):
    """Every input set of the GPU tests, both members: numpy's f64 chain gives the exact leaf on the
    decided rows and is within one unit on the others, and at most 1 % of the rows are undecided."""
    for m in range(K.TD_P):
        sq1, sq2, leaf, decided = K.td_case(alpha, eps, two, m)
        have = prio_oracle.td_leaves(sq1, sq2, alpha, eps)
        diff = np.abs(have.astype(np.int64) - leaf.astype(np.int64))
        und = int((~decided).sum())
        print(f"alpha {alpha} eps {eps} two {two} member {m}: {und} of {leaf.size} undecided, numpy off on "
              f"{int((diff != 0).sum())} of them")
        assert und <= K.UNDECIDED_CAP * leaf.size
        assert not (diff[decided] != 0).any() and diff.max() <= 1
        if alpha == 0:
            assert decided.all() and set(leaf.tolist()) == {1, ONE}
            continue
        rest = leaf[K.EDGES.size:]
        assert (rest < CAP).all() and rest.min() < ONE                 # none of the log-uniform rows is capped
        share = (rest > 1 << 26).mean()
        assert share > 0.15, share                                     # (a third at small alpha and two critics)
        assert (leaf[: K.EDGES.size] == CAP).any() and (leaf[: K.EDGES.size] == 1).sum() >= 3


def test_the_excluded_combination_breaks_the_cap():
    """alpha = 2, eps = 0, one critic: sqrt(x)^2 x 65536 is an integer for many f32 x."""
    sq1, _ = K.td_inputs(2.0, 0.0)
    _, decided = prio_oracle.td_leaves_mp(sq1, None, 2.0, 0.0)
    assert (~decided).sum() > 5 * K.UNDECIDED_CAP * sq1.size
    assert (2.0, 0.0) not in K.ALPHA_EPS


@pytest.mark.parametrize("alpha,eps", [(0.6, 0.0), (0.6, 1e-3), (0.3, 1e-3), (1.7, 0.0), (2.0, 1e-3)])
def test_bar_notices_a_float32_pow_and_a_rounding(alpha, eps):
    """2 000 log-uniform rows of one critic, a fifth of the leaves above 2^26 and none
    capped: exact-on-decided-rows fails by hundreds of rows for a pow in float32 (more than 300) and
    for rint in place of floor (more than 900), both of which pass a bar of one unit on leaves below
    2^20."""
    sq = K.log_uniform(alpha, 2000, np.random.default_rng(2000))
    leaf, decided = prio_oracle.td_leaves_mp(sq, None, alpha, eps)
    assert (~decided).sum() <= K.UNDECIDED_CAP * sq.size and (leaf < CAP).all() and (leaf > 1 << 26).mean() > 0.15
    assert np.array_equal(K.td_leaves_variant(sq, None, alpha, eps)[decided], leaf[decided])
    p32 = K.td_leaves_variant(sq, None, alpha, eps, pow32=True)
    rnd = K.td_leaves_variant(sq, None, alpha, eps, rint=True)
    n32, nr = int((p32 != leaf)[decided].sum()), int((rnd != leaf)[decided].sum())
    small = leaf < 1 << 20
    print(f"alpha {alpha} eps {eps}: float32 pow moves {n32} of 2000 decided leaves, rint {nr}; below 2^20 the "
          f"largest moves are {np.abs(p32.astype(np.int64) - leaf)[small].max()} and "
          f"{np.abs(rnd.astype(np.int64) - leaf)[small].max()}")
    assert n32 > 300 and nr > 900
    assert np.abs(rnd.astype(np.int64) - leaf).max() == 1            # (what the bar of one unit let through)


def _big_trees():
    return [K.tree_of(K.big_fill(m)) for m in range(K.BIG_P)]


def test_big_batches_hold_their_minimum_past_the_first_stride():
    """The calls the GPU test makes (numbers 0..5, host- and device-counted alike): the smallest drawn
    leaf lies at position 1 024 or later, and weights from the first 1 024 positions' minimum differ."""
    trees = _big_trees()
    assert max(trees[0].leaf[: K.BIG_M // 2]) < 1 << 21 and max(trees[0].leaf[K.BIG_M // 2:]) < 2000
    assert K.BIG_DRAWS == ((1025, 0), (1025, 1), (2048, 2), (2048, 3), (2500, 4), (2500, 5))
    for B, call in sorted(set(K.BIG_DRAWS + K.ANNEALED_DRAWS)):
        for m, t in enumerate(trees):
            idx, leaf, _ = t.draw(B, call, m, K.BIG_SEEDS[m], descend=False)
            at = int(np.argmin(leaf))
            print(f"B {B} call {call} member {m}: the smallest leaf at position {at}")
            assert at >= 1024 and leaf[:1024].min() >= 1 << 20 and leaf[at] < 2000, (B, call, m, at)
            for beta in (0.4, 0.6, 0.8, 1.0):
                w, bad = prio_oracle.weights(leaf, beta), K.weights_first_stride(leaf, beta)
                assert prio_oracle.ulp_distance_f32(w, bad).min() > 1000 and bad.max() > 1.0 == w.max()
    idx, leaf, _ = trees[0].draw(2048, 0, 0, K.BIG_SEEDS[0], descend=True)
    assert np.array_equal(idx, trees[0].draw(2048, 0, 0, K.BIG_SEEDS[0], descend=False)[0])


@pytest.mark.parametrize("B,empty", [(33, 27), (64, 58), (256, 250)])
def test_a_total_below_the_batch(B, empty):
    t = K.tree_of([1, 1, 2, 1, 1] + [0] * 95)
    t.leaf[5:] = [0] * 95                                              # (rows never stored: leaf 0, not the clamp's 1)
    assert t.total() == 6
    assert sum(lo == hi for lo, hi in (prio_oracle.stratum(6, B, j) for j in range(B))) == empty
    idx, leaf, ts = t.draw(B, 0, 0, 3)
    assert ts == [6 * j // B for j in range(B)]                        # t = lo_j, the width being 0 or 1
    assert set(idx.tolist()) == set(range(5)) and (leaf > 0).all()
    assert np.array_equal(idx, t.draw(B, 0, 0, 3, descend=False)[0])


@pytest.mark.parametrize("M", [64, 4097])
def test_a_total_that_the_leaves_do_not_add_up_to(M):
    t = K.tree_of(np.random.default_rng(M).integers(1, 1 << 22, M))
    T, B = t.total(), 256
    idx, leaf, ts = t.draw(B, 0, 0, 3, total=2 * T)
    past = np.array([x >= T for x in ts])
    assert all(0 <= x < 2 * T for x in ts) and past[B // 2 + 1:].all() and not past[: B // 2 - 1].any()
    assert (idx[past] == -1).all() and (leaf[past] == 0).all() and (idx[~past] >= 0).all()
    flat = t.draw(B, 0, 0, 3, descend=False, total=2 * T)
    assert np.array_equal(flat[0], idx) and np.array_equal(flat[1], leaf) and flat[2] == ts
    assert np.array_equal(leaf[~past], np.array(t.leaf, np.uint32)[idx[~past]])
    same = t.draw(B, 0, 0, 3, total=T)                                 # the total given is the default's
    for a, b in zip(same, t.draw(B, 0, 0, 3)):
        assert np.array_equal(a, b)
    assert not prio_oracle.weights(leaf, 0.4).any()                    # the least leaf is 0: every weight 0
