"""The prioritized replay's C interface and its restatement without a GPU
(include/sacenv_prioritized_replay.h, tests/prio_oracle.py).

* the library exports the entry points beside every older header's, ``_lib.load`` still takes a
  library without them, and ``_build`` lists the two new headers and no new source;
* every argument error is found on the host, before anything is launched, in the order the header
  states;
* the stratum bounds are floor(T j / B) without a 128-bit product, every drawn t lies below T, a
  row with leaf 0 is never drawn, and the oracle's draws follow the priorities;
* the Python side refuses pooling and a replay of the wrong type before it looks for a device.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import prio_oracle
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sacenv_prioritized_replay.h")
E_NULL, E_SIZE, E_RANGE = -1, -4, -5
NAMES = ("sacenv_replay_prio_layout", "sacenv_replay_prio_init", "sacenv_replay_prio_mark_stored",
         "sacenv_replay_prio_set", "sacenv_replay_prio_update_td", "sacenv_replay_prio_learn_rows",
         "sacenv_replay_prio_sample")


def _params(M=100, D=11, A=1, reward_f32=1, mask=2):
    from sacenv import _lib
    p = _lib.ReplayParams()
    p.mem_size, p.obs_dim, p.act_dim, p.reward_f32, p.terminal_mask = M, D, A, reward_f32, mask
    return p


def _older():
    from sacenv import _lib
    return (_lib.EXPORTS + _lib.EPISODE_EXPORTS + _lib.POPULATION_EXPORTS + _lib.REPLAY_POP_EXPORTS +
            _lib.NOISE_EXPORTS + _lib.SCOREBOARD_EXPORTS + _lib.SELECTION_EXPORTS + _lib.TRACES_EXPORTS +
            _lib.FRAMES_EXPORTS + _lib.REPLAY_SHARE_EXPORTS)


def test_library_exports_the_prioritized_entry_points(built_lib):
    import sacenv
    from sacenv import _build, _lib
    assert _lib.REPLAY_PRIO_EXPORTS == NAMES
    for n in NAMES:
        assert hasattr(built_lib, n), n
        assert n not in _older()
    src = open(HEADER).read()
    assert set(re.findall(r"^int (sacenv_\w+)\s*\(", src, re.M)) == set(NAMES)        # the declarations
    assert int(re.search(r"#define SACENV_REPLAY_PRIO_VERSION (\d+)", src).group(1)) == _lib.REPLAY_PRIO_VERSION == 1
    assert int(re.search(r"#define SACENV_REPLAY_PRIO_KEY1 (0x[0-9A-Fa-f]+)ull", src).group(1), 16) \
        == _lib.REPLAY_PRIO_KEY1 == prio_oracle.KEY1
    assert len({0, _lib.NOISE_KEY1, _lib.SELECT_KEY1, _lib.REPLAY_PRIO_KEY1}) == 4       # a key word of its own
    assert int(re.search(r"#define SACENV_REPLAY_PRIO_MAX_LEVELS (\d+)", src).group(1)) == _lib.REPLAY_PRIO_MAX_LEVELS
    # the older headers do not move
    assert _lib.ABI_VERSION == 20 == built_lib.sacenv_abi_version()
    assert _lib.REPLAY_POP_VERSION == 1 and _lib.REPLAY_SHARE_VERSION == 1
    # two headers more, no source more
    assert "sacenv_prioritized_replay.h" in _build.PUBLIC_HEADERS and "sacenv_replay_prio.h" in _build.HEADERS
    rel = [r for r, _ in _build.deps()]
    assert os.path.join("include", "sacenv_prioritized_replay.h") in rel
    assert os.path.join("sac-agent_amd", "csrc", "sacenv_replay_prio.h") in rel
    assert len(_build.SOURCES) == 10
    assert sorted(_build.SOURCES) == sorted(f for f in os.listdir(_build.CSRC) if f.endswith(".hip"))
    assert "PrioritizedPopulationReplay" in sacenv.__all__
    from sacenv.prioritized import PrioritizedPopulationReplay
    assert sacenv.PrioritizedPopulationReplay is PrioritizedPopulationReplay


def test_lib_loads_a_library_without_the_prioritized_entry_points(built_lib, tmp_path):
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
    assert len(_lib.require(_lib.REPLAY_SHARE_EXPORTS, "sacenv_population_share.h", lib)) == 2
    with pytest.raises(_lib.SacenvError, match="sacenv_prioritized_replay.h"):
        _lib.require(_lib.REPLAY_PRIO_EXPORTS, "sacenv_prioritized_replay.h", lib)
    assert len(_lib.require(_lib.REPLAY_PRIO_EXPORTS, "sacenv_prioritized_replay.h", built_lib)) == len(NAMES)


@pytest.mark.parametrize("M", [1, 64, 65, 100, 4096, 4097, 1_000_000, (1 << 31) - 1])
def test_layout_is_the_oracles(built_lib, M):
    from sacenv import _lib
    L = _lib.replay_prio_layout(_params(M=M), 3)
    want = prio_oracle.layout(M)
    assert L.levels == want["levels"] <= _lib.REPLAY_PRIO_MAX_LEVELS
    assert list(L.count)[: L.levels] == want["count"] and list(L.offset)[: L.levels] == want["offset"]
    assert not any(list(L.count)[L.levels:]) and not any(list(L.offset)[L.levels:])
    assert L.member_bytes == want["member_bytes"] and L.total_bytes == 3 * L.member_bytes
    assert L.member_bytes % 256 == 0 and all(o % 256 == 0 for o in want["offset"])
    assert want["count"][-1] <= 64 and (L.levels == 1 or want["count"][-2] > 64)
    if M == 1_000_000:
        assert want["count"] == [1_000_000, 15_625, 245, 4]


BAD_PARAMS = (dict(M=0), dict(M=-5), dict(M=1 << 31), dict(D=0), dict(A=0))


def test_argument_errors_without_gpu(built_lib):
    """Every rule of the entry points, none of which launches (there is no device here). Pointers
    are plain numbers with the alignment under test."""
    from sacenv import _lib
    lib, cap = built_lib, 64
    pp = ctypes.byref(_params())
    AR, ST, X = 1 << 20, 2 << 20, 3 << 20          # (256-B aligned)
    sd = (ctypes.c_uint64 * 64)(*range(64))
    inf, nan = float("inf"), float("nan")

    def layout(p=pp, m=2, out=ctypes.byref(_lib.ReplayPrioLayout())):
        return lib.sacenv_replay_prio_layout(p, m, out)

    def init(p=pp, m=2, st=ST):
        return lib.sacenv_replay_prio_init(p, m, st, None)

    def mark(p=pp, m=2, ar=AR, st=ST, cntr=0, n=8):
        return lib.sacenv_replay_prio_mark_stored(p, m, ar, st, cntr, n, None)

    def set_(p=pp, m=2, st=ST, batch=8, idx=X, leaf=X):
        return lib.sacenv_replay_prio_set(p, m, st, batch, idx, leaf, None)

    def update(p=pp, m=2, st=ST, batch=8, idx=X, sq1=X, sq2=X, stride=8, alpha=0.6, eps=1e-3):
        return lib.sacenv_replay_prio_update_td(p, m, st, batch, idx, sq1, sq2, stride, alpha, eps, None)

    def sample(p=pp, m=2, ar=AR, st=ST, batch=8, call=0, seeds=sd, idx=X, leaf=X, w=X, beta=0.4, o=X):
        return lib.sacenv_replay_prio_sample(p, m, ar, st, batch, call, seeds, idx, leaf, w, beta, o, o, o, o, o, None)

    # the parameters and the members come first, for every call
    for call in (layout, init, mark, set_, update, sample):
        assert call(p=None) == E_NULL
        for m in (0, -1, cap + 1):
            assert call(m=m) == E_SIZE, (call.__name__, m)
        for bad in BAD_PARAMS:
            assert call(p=ctypes.byref(_params(**bad))) == E_SIZE, (call.__name__, bad)
    assert layout(out=None) == E_NULL and layout() == 0 and layout(m=1) == 0 and layout(m=cap) == 0
    assert init(st=None) == E_NULL and init(st=ST + 64) == E_SIZE
    # mark: cntr, n, no rows, NULL, alignment
    assert mark(cntr=-2) == E_RANGE and mark(cntr=-2, n=-1) == E_RANGE      # cntr before n
    assert mark(n=-1) == E_SIZE and mark(n=-1, st=None) == E_SIZE
    assert mark(n=0) == 0 and mark(n=0, st=None) == 0 and mark(n=0, m=cap + 1) == E_SIZE
    assert mark(st=None) == E_NULL and mark(st=None, ar=AR + 64, cntr=-1) == E_NULL
    assert mark(cntr=-1, ar=None) == E_NULL          # the device count lives in the arena
    assert mark(st=ST + 128) == E_SIZE and mark(cntr=-1, ar=AR + 64) == E_SIZE
    # set: batch, no rows, NULL, alignment
    assert set_(batch=-1) == E_SIZE and set_(batch=-1, idx=None) == E_SIZE
    assert set_(batch=0) == 0 and set_(batch=0, st=None, idx=None, leaf=None) == 0
    for k in ("st", "idx", "leaf"):
        assert set_(**{k: None}) == E_NULL, k
    assert set_(st=ST + 16) == E_SIZE and set_(st=ST + 16, idx=None) == E_NULL    # NULL before alignment
    # update_td: batch and stride, then alpha and eps, then no rows, NULL, alignment
    assert update(batch=-1) == E_SIZE and update(stride=-1) == E_SIZE and update(batch=-1, alpha=nan) == E_SIZE
    for bad in (-0.1, inf, -inf, nan):
        assert update(alpha=bad) == E_RANGE and update(eps=bad) == E_RANGE, bad
        assert update(alpha=bad, batch=0) == E_RANGE and update(alpha=bad, idx=None) == E_RANGE
    assert update(alpha=0.0, eps=0.0, batch=0) == 0 and update(batch=0, st=None, idx=None, sq1=None) == 0
    for k in ("st", "idx", "sq1"):
        assert update(**{k: None}) == E_NULL, k
    assert update(st=ST + 16) == E_SIZE and update(st=ST + 16, sq1=None) == E_NULL
    # sample: batch, call and beta, no rows, NULL, alignment and size
    assert sample(batch=-1) == E_SIZE and sample(batch=-1, call=-2) == E_SIZE
    assert sample(call=-2) == E_RANGE and sample(call=-2, idx=None) == E_RANGE
    for bad in (-0.1, inf, nan):
        assert sample(beta=bad) == E_RANGE and sample(beta=bad, batch=0) == E_RANGE, bad
    assert sample(batch=0) == 0 and sample(batch=0, ar=None, st=None, idx=None, leaf=None, seeds=None) == 0
    assert sample(batch=0, m=cap + 1) == E_SIZE
    for k in ("ar", "st", "seeds", "idx", "leaf"):
        assert sample(**{k: None}) == E_NULL, k
    assert sample(ar=AR + 64) == E_SIZE and sample(st=ST + 64) == E_SIZE and sample(st=ST + 64, leaf=None) == E_NULL
    assert sample(batch=(1 << 31) - 1) == E_SIZE       # (2^31 - 1) x 13 >= 2^32 elements
    # the accessor of the learn scratch
    sp = _lib.SacParams(obs_dim=11, n_actions=1, hidden=256, batch=256)
    o1, o2 = ctypes.c_int64(), ctypes.c_int64()
    f = lib.sacenv_replay_prio_learn_rows
    assert f(None, ctypes.byref(o1), ctypes.byref(o2)) == E_NULL
    assert f(ctypes.byref(sp), None, ctypes.byref(o2)) == E_NULL and f(ctypes.byref(sp), ctypes.byref(o1), None) == E_NULL
    assert f(ctypes.byref(_lib.SacParams(obs_dim=11, n_actions=1, hidden=256, batch=64)), ctypes.byref(o1),
             ctypes.byref(o2)) == E_SIZE
    assert f(ctypes.byref(sp), ctypes.byref(o1), ctypes.byref(o2)) == 0
    L = _lib.sac_layout(sp)
    # two consecutive [batch] rows, the last two of the row fields, inside the scratch
    assert o2.value == o1.value + 256 and o1.value >= 16 * 256 * 256
    assert (o2.value + 256 + 16 * 256) * 4 <= L.scratch_bytes


def test_stratum_bounds_are_exact_floors():
    """lo_j == T j // B with no product past 64 bits (the oracle asserts that), for T up to 2^51
    and B up to 4096."""
    rng = np.random.default_rng(5)
    Ts = [0, 1, 2, 63, 64, 65, 4095, (1 << 31) - 1, 1 << 31, (1 << 51) - 1, 1 << 51]
    Ts += [int(x) for x in rng.integers(0, 1 << 51, 40)]
    for T in Ts:
        for B in (1, 2, 33, 64, 255, 256, 1000, 4095, 4096):
            js = {0, 1, B // 2, B - 1} | {int(x) for x in rng.integers(0, B, 6)}
            for j in js:
                lo, hi = prio_oracle.stratum(T, B, j)
                assert lo == T * j // B and hi == T * (j + 1) // B, (T, B, j)
            assert prio_oracle.stratum(T, B, B - 1)[1] == T and prio_oracle.stratum(T, B, 0)[0] == 0


def _filled(M, stored, seed):
    rng = np.random.default_rng(seed)
    t = prio_oracle.Tree(M)
    t.set(np.arange(stored), rng.integers(1, 1 << 20, stored))
    if stored > 3:
        t.set([1, stored - 2], [prio_oracle.CAP, 1])               # the ends of the leaf range
    return t


@pytest.mark.parametrize("M,stored", [(64, 64), (65, 65), (100, 37), (4097, 4097), (4097, 1)])
@pytest.mark.parametrize("B", [1, 33, 64, 256])
def test_every_draw_lands_on_a_stored_row(M, stored, B):
    t = _filled(M, stored, M + stored)
    T = t.total()
    for call in (0, 7):
        idx, leaf, ts = t.draw(B, call, 1, 99)
        assert len(ts) == B and all(0 <= x < T for x in ts)
        assert ((idx >= 0) & (idx < stored)).all() and (leaf > 0).all()
        assert np.array_equal(leaf, np.array(t.leaf, np.uint32)[idx])
        flat = t.draw(B, call, 1, 99, descend=False)                 # the walk down the levels = the running sum
        assert np.array_equal(flat[0], idx) and np.array_equal(flat[1], leaf) and flat[2] == ts
        # slot j's t lies in stratum j
        for j, x in enumerate(ts):
            lo, hi = prio_oracle.stratum(T, B, j)
            assert lo <= x < max(hi, lo + 1)
    w = prio_oracle.weights(leaf, 0.4)
    assert w.dtype == np.float32 and w.max() == 1.0 and (w > 0).all()
    assert np.array_equal(prio_oracle.Tree(M).draw(B, 0, 0, 1)[0], np.full(B, -1))   # an empty tree draws nothing


def test_oracle_draws_follow_the_priorities():
    """400 calls of B = 64 on leaves (1, 2, 3, 4) x 65536 over 66 rows: every row's count within 5
    standard deviations of calls B p_i."""
    M, B, calls = 66, 64, 400
    t = prio_oracle.Tree(M)
    t.set(np.arange(M), [(1 + i % 4) * 65536 for i in range(M)])
    counts = np.zeros(M, np.int64)
    for call in range(calls):
        counts += np.bincount(t.draw(B, call, 0, 2024)[0], minlength=M)
    n = calls * B
    p = np.array(t.leaf, np.float64) / t.total()
    sd = np.sqrt(n * p * (1 - p))                 # (stratified draws vary less than independent ones)
    assert counts.sum() == n and (np.abs(counts - n * p) <= 5 * sd).all(), np.abs(counts - n * p) / sd


def test_oracle_writes():
    t = prio_oracle.Tree(100)
    t.mark_stored(0, 37)
    assert t.leaf[:37] == [65536] * 37 and not any(t.leaf[37:])
    t.set([5, 5, -1, 100, 7, 5], [10, 20, 30, 40, 0, 1 << 33])        # the last 5 wins; 0 and 2^33 are clamped
    assert t.leaf[5] == prio_oracle.CAP and t.leaf[7] == 1 and t.max_leaf == prio_oracle.CAP
    t.mark_stored(90, 20)                                             # wraps
    assert all(t.leaf[i] == prio_oracle.CAP for i in list(range(90, 100)) + list(range(10)))
    t.mark_stored(0, 250)                                             # n > M: rows (0 + 150 + j) % 100
    assert all(v == prio_oracle.CAP for v in t.leaf)
    lv = prio_oracle.td_leaves(np.array([0, 1, 4, np.nan, np.inf, -1, 1e-12], np.float32), None, 1.0, 0.0)
    assert list(lv) == [1, 65536, 131072, 1, prio_oracle.CAP, 1, 1]
    lv = prio_oracle.td_leaves(np.array([4.0], np.float32), np.array([16.0], np.float32), 0.5, 1.0)
    assert list(lv) == [131072]                                       # (0.5 (2 + 4) + 1)^0.5 = 2


def test_python_side_without_a_device(built_lib, monkeypatch):
    """Pooling and a wrong replay type are refused before anything is built or launched."""
    from sacenv.agent import AgentConfig
    from sacenv.population import NativeSACPopulation
    from sacenv.prioritized import PrioritizedPopulationReplay
    bare = object.__new__(PrioritizedPopulationReplay)               # (no device: nothing is built)
    with pytest.raises(ValueError, match="pool_rows"):
        PrioritizedPopulationReplay.sample(bare, 64, pool_rows=8)
    with pytest.raises(ValueError, match="pool_rows"):
        PrioritizedPopulationReplay.sample_pool(bare, 64, 8)
    for bad in (dict(alpha=-1.0), dict(beta=float("nan")), dict(eps=float("inf"))):
        with pytest.raises(ValueError, match=next(iter(bad))):
            PrioritizedPopulationReplay(2, 1024, (11,), 1, device="cuda", **bad)
    cfgs = [AgentConfig(batch_size=256, max_size=1024) for _ in range(2)]
    import torch
    from sacenv import _lib
    monkeypatch.setattr(_lib, "cuda_device", lambda device, who: torch.device("cuda", 0))   # (no device is asked)
    with pytest.raises(TypeError, match="PopulationReplay"):
        NativeSACPopulation("cuda", cfgs, replay=object())
