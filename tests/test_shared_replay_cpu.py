"""The pooled sample's C interface and its numpy restatement without a GPU
(include/sacenv_population_share.h, tests/share_oracle.py).

* the library exports the two entry points beside every older header's, ``_lib.load`` still
  takes a library without them, and only ``require`` asks for them;
* every argument error is found on the host, before anything is launched, in the order the header
  states;
* the stream rule both draws follow -- masked rejection on 32-bit words, the stream stopping
  after the last accepted word, a draw of size 0 consuming nothing -- is numpy's, word for word;
* the oracle's two ends are plain ``choice`` calls: K = 0 is ``choice(s, B)`` + m M, K = B is
  ``choice(P s, B)`` mapped to (owner, row), and after either the generator stands where two
  plain ``choice`` calls leave it.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import share_oracle
from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "sacenv_population_share.h")
E_NULL, E_SIZE = -1, -4
NAMES = ("sacenv_replay_pop_sample_pool", "sacenv_replay_pop_gather_pool")


def _params(M=100, D=11, A=1, reward_f32=1, mask=2):
    from sacenv import _lib
    p = _lib.ReplayParams()
    p.mem_size, p.obs_dim, p.act_dim, p.reward_f32, p.terminal_mask = M, D, A, reward_f32, mask
    return p


def _older():
    from sacenv import _lib
    return (_lib.EXPORTS + _lib.EPISODE_EXPORTS + _lib.POPULATION_EXPORTS + _lib.REPLAY_POP_EXPORTS +
            _lib.NOISE_EXPORTS + _lib.SCOREBOARD_EXPORTS + _lib.SELECTION_EXPORTS + _lib.TRACES_EXPORTS +
            _lib.FRAMES_EXPORTS)


def test_library_exports_the_pooled_entry_points(built_lib):
    from sacenv import _build, _lib
    assert _lib.REPLAY_SHARE_EXPORTS == NAMES
    for n in NAMES:
        assert hasattr(built_lib, n), n
        assert n not in _older()
    src = open(HEADER).read()
    assert set(re.findall(r"\b(sacenv_\w+)\s*\(", src)) == set(NAMES)
    assert int(re.search(r"#define SACENV_REPLAY_SHARE_VERSION (\d+)", src).group(1)) == _lib.REPLAY_SHARE_VERSION == 1
    assert _lib.ABI_VERSION == 20 == built_lib.sacenv_abi_version()           # sacenv.h does not move
    assert _lib.REPLAY_POP_VERSION == 1                                       # nor the population replay's header
    rel = [r for r, _ in _build.deps()]
    assert os.path.join("include", "sacenv_population_share.h") in rel
    assert "sacenv_population_share.h" in _build.PUBLIC_HEADERS


def test_lib_loads_a_library_without_the_pooled_entry_points(built_lib, tmp_path):
    """``SACENV_LIB`` may point at a build from before sacenv_population_share.h (a stand-in that
    exports every older name and neither of the two): it loads, everything older is bound, and
    only asking for the pooled entry points raises."""
    from sacenv import _lib
    src = tmp_path / "old.c"
    body = ["int sacenv_abi_version(void) { return %d; }" % _lib.ABI_VERSION]
    body += [f"int {n}(void) {{ return 0; }}" for n in _older() if n != "sacenv_abi_version"]
    src.write_text("\n".join(body))
    so = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = _lib.load(str(so))
    assert lib.sacenv_abi_version() == _lib.ABI_VERSION
    assert not any(hasattr(lib, n) for n in NAMES)
    assert len(_lib.require(_lib.REPLAY_POP_EXPORTS, "sacenv_population_replay.h", lib)) == 5
    with pytest.raises(_lib.SacenvError, match="sacenv_population_share.h"):
        _lib.require(_lib.REPLAY_SHARE_EXPORTS, "sacenv_population_share.h", lib)
    assert len(_lib.require(_lib.REPLAY_SHARE_EXPORTS, "sacenv_population_share.h", built_lib)) == 2


BAD_PARAMS = (dict(M=0), dict(M=-5), dict(M=1 << 31), dict(D=0), dict(A=0))


def test_argument_errors_without_gpu(built_lib):
    """Every rule of the two entry points, none of which launches (there is no device here).
    Pointers are plain numbers with the alignment under test."""
    lib, cap = built_lib, 64
    pp = ctypes.byref(_params())
    AR, X = 1 << 20, 3 << 20          # (256-B aligned)

    def sample(p=pp, m=2, ar=AR, batch=256, pool=128, stored=10, idx=X, s=X, a=X, r=X, s2=X, t=X):
        return lib.sacenv_replay_pop_sample_pool(p, m, ar, batch, pool, stored, idx, s, a, r, s2, t, None)

    def gather(p=pp, m=2, ar=AR, batch=256, idx=X, s=X, a=X, r=X, s2=X, t=X):
        return lib.sacenv_replay_pop_gather_pool(p, m, ar, batch, idx, s, a, r, s2, t, None)

    B = 256
    for call, none in ((sample, dict(batch=0, pool=0)), (gather, dict(batch=0))):   # none: a call of no rows
        assert call(p=None) == E_NULL
        for k in ("ar", "idx"):                              # NULL arena or NULL idx
            assert call(**{k: None}) == E_NULL, k
        for m in (0, -1, cap + 1):                           # members = 0 and members = 65
            assert call(m=m) == E_SIZE, m
        for bad in BAD_PARAMS:
            assert call(p=ctypes.byref(_params(**bad))) == E_SIZE, bad
        assert call(batch=-1) == E_SIZE
        assert call(ar=AR + 64) == E_SIZE
        assert call(batch=(1 << 31) - 1) == E_SIZE           # (2^31 - 1) x 13 >= 2^32 elements
        # members x mem_size > 2^32 (no P <= 64 and M < 2^31 multiply to 2^32 + 1 exactly: the
        # least product above 2^32 with 3 members is 2^32 + 2); 2^32 itself and 2^32 - 2 are legal
        assert call(p=ctypes.byref(_params(M=1431655766)), m=3) == E_SIZE
        assert call(p=ctypes.byref(_params(M=(1 << 26) + 1)), m=64) == E_SIZE
        assert call(p=ctypes.byref(_params(M=1 << 26)), m=64, **none) == 0
        assert call(p=ctypes.byref(_params(M=(1 << 31) - 1)), m=2, **none) == 0
        assert call(**none) == 0                            # nothing to draw: OK, nothing launched
        assert call(**none, s=None, a=None, r=None, s2=None, t=None) == 0
        assert call(**none, idx=None) == E_NULL             # idx is required
        assert call(**none, m=cap + 1) == E_SIZE            # the members are checked before the rows
        assert call(**none, m=1) == 0                       # one member is legal
    for pool in (-1, B + 1):                                 # pool_rows = -1 and pool_rows = B + 1
        assert sample(batch=B, pool=pool) == E_SIZE, pool
    assert sample(batch=0, pool=1) == E_SIZE
    assert sample(batch=0, pool=0) == 0
    for stored in (0, -1):                                   # stored = 0: np.random.choice(0, n) raises
        assert sample(stored=stored) == E_SIZE, stored
        assert sample(stored=stored, batch=0, pool=0) == E_SIZE, stored
    # the order: the family's rules first (a NULL idx beside bad pool rows is the NULL), the pool
    # rows before the pool's size
    assert sample(idx=None, pool=B + 1) == E_NULL
    assert sample(p=ctypes.byref(_params(M=1431655766)), m=3, pool=B + 1) == E_SIZE


# (range, size) as include/sacenv_population_share.h's draws meet them: P s = 2; one past a power
# of two (about half of the words rejected); a range past 2^16 whose 700 and 1 024 rows cross two
# 624-word blocks
STREAM_CASES = [(2, 5), (513, 64), (65538, 700), (65538, 1024), (1, 7), (57, 0)]


def _masked_rejection(words, rng, size):
    """The rule of sacenv_replay_core.h on a word sequence: (values, words consumed)."""
    if rng == 0 or size == 0:
        return np.zeros(size, np.int64), 0
    mask = (1 << int(rng).bit_length()) - 1
    out, used = [], 0
    for w in words:
        used += 1
        v = int(w) & mask
        if v <= rng:
            out.append(v)
            if len(out) == size:
                break
    assert len(out) == size, "the word sequence ran short"
    return np.array(out, np.int64), used


@pytest.mark.parametrize("n,size", STREAM_CASES)
def test_the_stream_rule_is_numpys(n, size):
    """``RandomState.choice(n, size)`` is masked rejection on the generator's 32-bit words with rng
    = n - 1, and leaves the generator right after the last accepted word. (``randint`` over the
    full 32-bit range returns the raw words.)"""
    seed = 1234 + n
    a, b, raw = (np.random.RandomState(seed) for _ in range(3))
    a.choice(50, 3), b.choice(50, 3), raw.choice(50, 3)       # (not at the start of a block)
    words = raw.randint(0, 1 << 32, 4 * size + 64, dtype=np.uint32)
    want, used = _masked_rejection(words, n - 1, size)
    assert np.array_equal(a.choice(n, size), want)
    b.randint(0, 1 << 32, used, dtype=np.uint32)              # skip the words the draw consumed
    assert np.array_equal(a.randint(0, 1 << 32, 8, dtype=np.uint32), b.randint(0, 1 << 32, 8, dtype=np.uint32))
    if (n, size) == (513, 64):
        assert used > 100                                     # about half of the words are rejected
    if (n, size) == (65538, 700):
        assert used > 2 * 624                                 # the draw crosses two twists


ORACLE_CASES = [(2, 64, 1, 64), (9, 57, 57, 64), (2, 40000, 32769, 700), (3, 100, 250, 33), (1, 100, 60, 16)]


@pytest.mark.parametrize("P,M,count,B", ORACLE_CASES)
def test_oracle_ends_are_plain_choice_calls(P, M, count, B):
    s = min(count, M)
    seeds = [7 + 13 * m for m in range(P)]
    # K = 0: choice(s, B) + m M
    rngs, ref = [np.random.RandomState(x) for x in seeds], [np.random.RandomState(x) for x in seeds]
    idx = share_oracle.draw(rngs, P, M, count, B, 0)
    assert idx.shape == (P, B) and idx.dtype == np.int64
    for m in range(P):
        assert np.array_equal(idx[m], ref[m].choice(s, B) + m * M)
        ref[m].choice(P * s, 0)                                # (a draw of size 0 moves nothing)
        assert np.array_equal(rngs[m].randint(0, 1 << 32, 4, dtype=np.uint32),
                              ref[m].randint(0, 1 << 32, 4, dtype=np.uint32))
    # K = B: choice(P s, B) as (owner, row)
    rngs, ref = [np.random.RandomState(x) for x in seeds], [np.random.RandomState(x) for x in seeds]
    idx = share_oracle.draw(rngs, P, M, count, B, B)
    for m in range(P):
        ref[m].choice(s, 0)
        g = ref[m].choice(P * s, B)
        assert np.array_equal(idx[m] // M, g // s) and np.array_equal(idx[m] % M, g % s)
        assert (idx[m] // M).max() < P and (idx[m] % M).max() < s
        assert np.array_equal(rngs[m].randint(0, 1 << 32, 4, dtype=np.uint32),
                              ref[m].randint(0, 1 << 32, 4, dtype=np.uint32))
    # in between: two plain choice calls, own rows first
    K = B // 2
    rngs, ref = [np.random.RandomState(x) for x in seeds], [np.random.RandomState(x) for x in seeds]
    idx = share_oracle.draw(rngs, P, M, count, B, K, poisoned=(P - 1,) if P > 1 else ())
    for m in range(P):
        if P > 1 and m == P - 1:
            assert (idx[m] == -1).all()
        else:
            own, g = ref[m].choice(s, B - K), ref[m].choice(P * s, K)
            assert np.array_equal(idx[m], np.concatenate([m * M + own, (g // s) * M + g % s]))
        assert np.array_equal(rngs[m].randint(0, 1 << 32, 4, dtype=np.uint32),
                              ref[m].randint(0, 1 << 32, 4, dtype=np.uint32))
    with pytest.raises(ValueError):
        share_oracle.draw(rngs, P, M, count, B, B + 1)
    with pytest.raises(ValueError):
        share_oracle.draw(rngs, P, M, 0, B, 0)


def test_oracle_gather_reads_the_owners_rows():
    P, M, D = 3, 5, 2
    state = np.arange(P * M * D, dtype=np.float32).reshape(P, M, D) + 1
    reward = np.arange(P * M, dtype=np.float64).reshape(P, M) + 100
    idx = np.array([[0, 14, -1, 7], [5, 15, 1 << 40, 4], [10, 9, 3, 3]], np.int64)
    st, rw = share_oracle.gather((state, reward), idx, M)
    assert st.shape == (P, 4, D) and rw.shape == (P, 4)
    assert np.array_equal(rw, [[100, 114, 0, 107], [105, 0, 0, 104], [110, 109, 103, 103]])
    assert np.array_equal(st[1, 0], state[1, 0]) and np.array_equal(st[0, 1], state[2, 4])
    assert not st[0, 2].any() and not st[1, 1].any() and not st[1, 2].any()


def test_python_side_without_a_device(built_lib):
    """``pool_rows`` is refused before the device is looked at."""
    from sacenv.agent import AgentConfig
    from sacenv.population import NativeSACPopulation
    cfgs = [AgentConfig(batch_size=64, max_size=1024) for _ in range(2)]
    for bad in (-1, 65):
        with pytest.raises(ValueError, match="pool_rows"):
            NativeSACPopulation("cuda", cfgs, pool_rows=bad)
    with pytest.raises(ValueError, match="PopulationReplay"):
        NativeSACPopulation("cuda", cfgs, pool_rows=32)
