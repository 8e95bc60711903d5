"""Population selection without a GPU (include/sacenv_selection.h, tests/selection_oracle.py).

* the header's functions are ``_lib.SELECTION_EXPORTS``, beside the 49 of include/sacenv.h and
  every older optional header; the build lists the new unit and header;
* ``SacenvSelect`` and the 64-B member record have the layout of their ctypes, numpy and
  ``struct`` mirrors;
* the numpy restatement, held to first principles: the ready members' ranks are a permutation,
  winners and losers are disjoint, every source is a winner, every new value lies in its range;
  one case worked by hand; the multiply-shift stays in [0, q);
* every argument error is found on the host, before anything is launched;
* a library without the new names still loads.
"""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import selection_oracle as sel
from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "sacenv_selection.h")
E_NULL, E_SIZE, E_RANGE = -1, -4, -5
HP0 = (0.004, 0.002, 0.97, 0.005)


def _select(**kw):
    from sacenv import _lib
    base = dict(members=4, quantile=1, lookback=50, reserved=0, min_episodes=5, member_floats=8, seed=0,
                factor=(0.8, 1.2), lo=sel.DEFAULT_LO, hi=sel.DEFAULT_HI)
    base.update(kw)
    for name, n in (("factor", 2), ("lo", 4), ("hi", 4)):
        base[name] = (ctypes.c_double * n)(*base[name])
    return _lib.Select(**base)


def _hp(P, seed=0):
    """[P][4] initial values inside the default ranges."""
    rng = np.random.default_rng(seed)
    return [[float(rng.uniform(lo, hi)) for lo, hi in zip(sel.DEFAULT_LO, sel.DEFAULT_HI)] for _ in range(P)]


def test_header_and_exports(built_lib):
    from sacenv import _build, _lib
    src = open(HEADER).read()
    names = set(re.findall(r"\b(sacenv_\w+)\s*\(", src))
    assert names == set(_lib.SELECTION_EXPORTS) and len(_lib.SELECTION_EXPORTS) == 3
    for older in (_lib.EXPORTS, _lib.EPISODE_EXPORTS, _lib.POPULATION_EXPORTS, _lib.REPLAY_POP_EXPORTS,
                  _lib.NOISE_EXPORTS, _lib.SCOREBOARD_EXPORTS):
        assert not names & set(older)
    for n in names:
        assert hasattr(built_lib, n), n

    def define(name, base=10):
        return int(re.search(rf"#define SACENV_{name} (\w+?)(?:ull)?\b", src).group(1), base)

    assert define("SELECTION_VERSION") == _lib.SELECTION_VERSION == 1
    assert define("SELECT_MAX_MEMBERS") == _lib.SELECT_MAX_MEMBERS == 64
    assert define("SELECT_HEADER_BYTES") == _lib.SELECT_HEADER_BYTES == sel.HEADER_BYTES == 32
    assert define("SELECT_MEMBER_BYTES") == _lib.SELECT_MEMBER_BYTES == sel.MEMBER_BYTES == 64
    assert define("SELECT_COPY_THREADS") == _lib.SELECT_COPY_THREADS
    assert define("SELECT_COPY_UNROLL") == _lib.SELECT_COPY_UNROLL
    assert define("SELECT_COPY_CHUNKS") == _lib.SELECT_COPY_CHUNKS
    key1 = define("SELECT_KEY1", 16)
    assert key1 == _lib.SELECT_KEY1 == sel.KEY1 == int.from_bytes(b"select", "big")
    assert key1 not in (0, _lib.NOISE_KEY1)                  # the replay sampler's and the noise's
    assert _lib.ABI_VERSION == 20 == built_lib.sacenv_abi_version()
    rel = [r for r, _ in _build.deps()]
    assert os.path.join("include", "sacenv_selection.h") in rel
    assert os.path.join("sac-agent_amd", "csrc", "sacenv_select.hip") in rel
    assert os.path.join("sac-agent_amd", "csrc", "sacenv_wave_core.h") in rel
    assert "sacenv_select.hip" in _build.SOURCES
    text = open(os.path.join(_build.CSRC, "sacenv_select.hip")).read()
    for inc in ("sacenv_board_core.h", "sacenv_philox.h", "sacenv_selection.h", "sacenv_wave_core.h"):
        assert f'#include "{inc}"' in text
    assert "void philox4x64_10" not in text                  # one copy of the generator
    shared = open(os.path.join(_build.CSRC, "sacenv_wave_core.h")).read()    # (the copy's body lives there)
    assert not re.search(r"atomic\w*\s*\(", text + shared)   # no atomics: the bytes are the same run to run
    import sacenv
    from sacenv.selection import PopulationSelection
    assert sacenv.PopulationSelection is PopulationSelection and "PopulationSelection" in sacenv.__all__


def test_structs_match_c_layout(tmp_path):
    """offsetof / sizeof of SacenvSelect and SacenvSelectMember, from gcc on the header, against
    the ctypes mirrors, the numpy record dtype and the oracle's struct format."""
    from sacenv import _lib
    from sacenv.selection import STATE_DTYPE
    pairs = (("SacenvSelect", _lib.Select), ("SacenvSelectMember", _lib.SelectMember))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sacenv_selection.h"', "int main(void) {"]
    for cname, py in pairs:
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[0]: int(l.split()[1]) for l in out if l.strip()}
    assert got["SacenvSelect"] == ctypes.sizeof(_lib.Select) == 120
    assert got["SacenvSelectMember"] == ctypes.sizeof(_lib.SelectMember) == STATE_DTYPE.itemsize == 64
    for cname, py in pairs:
        for fname, _ in py._fields_:
            assert got[f"{cname}.{fname}"] == getattr(py, fname).offset, (cname, fname)
    for fname, _ in _lib.SelectMember._fields_:
        assert STATE_DTYPE.fields[fname][1] == getattr(_lib.SelectMember, fname).offset, fname
    rec = np.frombuffer(struct.pack(sel.MEMBER_FORMAT, 1, 2, 3, 4, 5, 0, 6.0, 7.0, 8.0, 9.0), STATE_DTYPE)[0]
    assert [int(rec[f]) for f in ("since", "replaced", "source_now", "rank_now", "parent")] == [1, 2, 3, 4, 5]
    assert rec["hp"].tolist() == [6.0, 7.0, 8.0, 9.0]


def test_the_empty_state_packs_as_the_header_says():
    ora = sel.SelectionOracle([HP0, HP0], 1, 1)
    raw = ora.pack()
    assert len(raw) == 32 + 2 * 64 and raw[:32] == bytes(32)
    assert struct.unpack(sel.MEMBER_FORMAT, raw[32:96]) == (0, 0, -1, -1, -1, 0, *HP0)


@pytest.mark.parametrize("family", sel.FAMILIES)
@pytest.mark.parametrize("P,q", [(2, 1), (3, 1), (5, 1), (5, 2), (16, 4), (63, 1), (63, 31), (64, 32)])
def test_the_oracle_against_first_principles(P, q, family):
    """Three rounds on a board whose members finish episodes in between. After each: the ready
    members' ranks are a permutation of 0..R-1 ordered by (avg descending, index); the losers are
    the last q ranks and the winners the first q, disjoint; every source is a winner; every new
    value lies in its range and is one of the two multiples of the source's old value, clipped;
    nobody else changes."""
    min_ep = 4
    lo, hi = sel.DEFAULT_LO, sel.DEFAULT_HI
    ora = sel.SelectionOracle(_hp(P, P + q), q, min_ep, seed=11 * P + q, lo=lo, hi=hi)
    episodes, avg = sel.board_family(family, P, q, min_ep, seed=P)
    replaced_total = 0
    for rnd in range(3):
        since, hp, parent, replaced = ora.since[:], [r[:] for r in ora.hp], ora.parent[:], ora.replaced[:]
        pairs = ora.step(episodes, avg)
        ready = [m for m in range(P) if episodes[m] - since[m] >= min_ep and avg[m] == avg[m]]
        R = len(ready)
        ranks = [ora.rank_now[m] for m in ready]
        assert sorted(ranks) == list(range(R))
        assert all(ora.rank_now[m] == -1 for m in range(P) if m not in ready)
        order = sorted(ready, key=lambda m: ora.rank_now[m])
        for a, b in zip(order, order[1:]):
            assert avg[a] > avg[b] or (avg[a] == avg[b] and a < b)
        losers = [l for l, _ in pairs]
        if rnd == 0 and family in ("exact", "short"):
            assert R == (2 * q if family == "exact" else 2 * q - 1)
        if R < 2 * q:
            assert not pairs
        else:
            assert losers == sorted(order[R - q:]) and ora.winners() == sorted(order[:q])
            assert not set(losers) & set(ora.winners())
        for l, s in pairs:
            assert s in ora.winners() and s != l
            assert ora.source_now[l] == ora.parent[l] == s and ora.since[l] == episodes[l]
            assert ora.replaced[l] == replaced[l] + 1
            for k in range(4):
                assert lo[k] <= ora.hp[l][k] <= hi[k]
                assert ora.hp[l][k] in [min(max(hp[s][k] * f, lo[k]), hi[k]) for f in ora.factor]
        for m in range(P):
            if m not in losers:
                assert (ora.source_now[m], ora.since[m], ora.hp[m], ora.parent[m], ora.replaced[m]) == \
                    (-1, since[m], hp[m], parent[m], replaced[m])
        replaced_total += len(pairs)
        assert (ora.round, ora.replaced_total) == (rnd + 1, replaced_total)
        episodes = episodes + np.arange(P) % 3 + (min_ep - 1)     # some of the replaced are ready again, some not
    if family in ("distinct", "equal", "zeros", "inf", "exact"):
        assert replaced_total >= q                                # the first round replaced


def test_ties_and_special_values_rank_as_the_rule_says():
    inf, nan = float("inf"), float("nan")
    assert sel.rank_ready([True] * 4, [3.75] * 4) == [0, 1, 2, 3]
    assert sel.rank_ready([True] * 4, [-0.0, 0.0, -0.0, 0.0]) == [0, 1, 2, 3]
    assert sel.rank_ready([True] * 4, [-inf, inf, 0.0, inf]) == [3, 0, 2, 1]
    assert sel.rank_ready([True, False, True, True], [1.0, 9.0, 2.0, 1.0]) == [1, -1, 0, 2]
    ora = sel.SelectionOracle([HP0] * 3, 1, 1)
    assert ora.step([5, 5, 5], [nan, 1.0, 2.0]) == [(1, 2)] and ora.rank_now == [-1, 1, 0]


def test_one_case_by_hand():
    """P = 4, q = 1, min_episodes = 2, seed 7, round 0. Means 3, 1, 2, 0.5 and member 1 with one
    episode only: ready are 0, 2, 3 with ranks 0, 1, 2; R = 3 >= 2, so member 3 (rank 2) loses to
    the member of rank ((w0 >> 32) * 1) >> 32 = 0, member 0. The factors are bits 0..3 of w1, the
    second word of numpy's own Philox block at counter (3, 0, 0, 0) under key (7, "select")."""
    hp = [[0.004, 0.002, 0.97, 0.005], [0.003, 0.003, 0.96, 0.002], [0.005, 0.001, 0.98, 0.009],
          [0.002, 0.004, 0.95, 0.001]]
    ora = sel.SelectionOracle(hp, 1, 2, seed=7)
    assert ora.step([9, 1, 4, 2], [3.0, 1.0, 2.0, 0.5]) == [(3, 0)]
    block = np.random.Philox(key=7 | sel.KEY1 << 64, counter=(3 - 1) % (1 << 256)).random_raw(4)
    w1 = int(block[1])
    f = [(0.8, 1.2)[(w1 >> k) & 1] for k in range(4)]
    want = [0.004 * f[0], 0.002 * f[1], min(0.97 * f[2], 0.99) if f[2] > 1 else max(0.97 * f[2], 0.95), 0.005 * f[3]]
    assert 0.001 <= want[0] <= 0.01 and 0.0008 <= want[1] <= 0.008 and 0.001 <= want[3] <= 0.01  # (no clip there)
    assert want[2] in (0.95, 0.99)                           # gamma: 0.776 and 1.164 both leave [0.95, 0.99]
    assert ora.hp == [hp[0], hp[1], hp[2], want]
    assert ora.pack() == struct.pack("<qqqq", 1, 1, 0, 0) + b"".join(
        struct.pack(sel.MEMBER_FORMAT, *row) for row in (
            (0, 0, -1, 0, -1, 0, *hp[0]), (0, 0, -1, -1, -1, 0, *hp[1]), (0, 0, -1, 1, -1, 0, *hp[2]),
            (2, 1, 0, 2, 0, 0, *want)))


def test_the_multiply_shift_stays_below_q():
    words = np.random.default_rng(5).integers(0, 2 ** 64, 100_000, dtype=np.uint64)
    words[:4] = (0, 2 ** 32 - 1, 2 ** 64 - 2 ** 32, 2 ** 64 - 1)
    for q in range(1, 33):
        j = ((words >> np.uint64(32)) * np.uint64(q)) >> np.uint64(32)
        assert int(j.max()) <= q - 1 and int(j[0]) == int(j[1]) == 0 and int(j[2]) == int(j[3]) == q - 1
        assert [sel.source_rank(int(w), q) for w in words[:64]] == j[:64].tolist()
        if q > 1:
            assert np.bincount(j.astype(np.int64), minlength=q).min() > 100_000 / q * 0.8     # every rank is drawn


def test_argument_errors_are_found_on_the_host(built_lib):
    """Each error returns its code before anything is launched (no device here): pointers are
    made-up addresses that are never followed."""
    from sacenv import _lib
    lib = built_lib
    n = ctypes.c_int64(-7)
    hp = (_lib.SacMember * 4)(*[_lib.SacMember(*HP0, 2.0) for _ in range(4)])
    good, p = _select(), 0x10000
    nan, inf = float("nan"), float("inf")
    assert lib.sacenv_select_bytes(ctypes.byref(good), ctypes.byref(n)) == 0 and n.value == 32 + 4 * 64
    assert lib.sacenv_select_bytes(None, ctypes.byref(n)) == E_NULL
    assert lib.sacenv_select_bytes(ctypes.byref(good), None) == E_NULL
    size = [dict(members=1), dict(members=65), dict(quantile=0), dict(quantile=3), dict(members=5, quantile=3),
            dict(lookback=0), dict(lookback=129), dict(min_episodes=0), dict(member_floats=0),
            dict(member_floats=-4), dict(member_floats=6)]
    rng = [dict(factor=(0.8, nan)), dict(factor=(inf, 1.2)), dict(factor=(0.0, 1.2)), dict(factor=(0.8, -1.2)),
           dict(lo=(nan, 0, 0, 0)), dict(hi=(1, 1, inf, 1)), dict(lo=(-inf, 0, 0, 0)),
           dict(lo=(0, 0, 0, 0.5), hi=(1, 1, 1, 0.25))]
    for code, cases in ((E_SIZE, size), (E_RANGE, rng)):
        for kw in cases:
            s = _select(**kw)
            assert lib.sacenv_select_bytes(ctypes.byref(s), ctypes.byref(n)) == code, kw
            assert lib.sacenv_select_init(ctypes.byref(s), hp, p, None) == code, kw
            assert lib.sacenv_select_step(ctypes.byref(s), p, p, p, None) == code, kw
    assert n.value == 32 + 4 * 64
    assert lib.sacenv_select_init(None, hp, p, None) == E_NULL
    assert lib.sacenv_select_init(ctypes.byref(good), None, p, None) == E_NULL
    assert lib.sacenv_select_init(ctypes.byref(good), hp, None, None) == E_NULL
    assert lib.sacenv_select_init(ctypes.byref(good), hp, p + 8, None) == E_RANGE
    for field in ("lr_actor", "lr_critic", "gamma", "tau"):
        for bad in (nan, inf, -inf):
            hp2 = (_lib.SacMember * 4)(*[_lib.SacMember(*HP0, 2.0) for _ in range(4)])
            setattr(hp2[3], field, bad)
            assert lib.sacenv_select_init(ctypes.byref(good), hp2, p, None) == E_RANGE, (field, bad)
    for args in ((None, p, p, p), (good, None, p, p), (good, p, None, p), (good, p, p, None)):
        a = [ctypes.byref(args[0]) if args[0] is not None else None, *args[1:]]
        assert lib.sacenv_select_step(*a, None) == E_NULL
    for k in range(3):
        ptrs = [p, p, p]
        ptrs[k] += 8
        assert lib.sacenv_select_step(ctypes.byref(good), *ptrs, None) == E_RANGE, k
    # the limits themselves pass
    for kw in (dict(members=2), dict(members=64, quantile=32), dict(lookback=128), dict(lo=(1, 1, 1, 1), hi=(1, 1, 1, 1))):
        assert lib.sacenv_select_bytes(ctypes.byref(_select(**kw)), ctypes.byref(n)) == 0, kw


def test_lib_loads_a_library_without_the_selection_entry_points(built_lib, tmp_path):
    """``SACENV_LIB`` may point at a build from before sacenv_selection.h (a stand-in that exports
    every older name and not the new ones); ``require`` then says what to do."""
    from sacenv import _lib
    older = (_lib.EXPORTS + _lib.EPISODE_EXPORTS + _lib.POPULATION_EXPORTS + _lib.REPLAY_POP_EXPORTS +
             _lib.NOISE_EXPORTS + _lib.SCOREBOARD_EXPORTS)
    body = ["int sacenv_abi_version(void) { return %d; }" % _lib.ABI_VERSION]
    body += [f"int {n}(void) {{ return 0; }}" for n in older if n != "sacenv_abi_version"]
    src = tmp_path / "old.c"
    src.write_text("\n".join(body))
    so = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = _lib.load(str(so))
    assert not any(hasattr(lib, n) for n in _lib.SELECTION_EXPORTS)
    assert all(hasattr(lib, n) for n in _lib.SCOREBOARD_EXPORTS)
    with pytest.raises(_lib.SacenvError, match="sacenv_selection.h"):
        _lib.require(_lib.SELECTION_EXPORTS, "sacenv_selection.h", lib)
    assert [f.__name__ for f in _lib.require(_lib.SELECTION_EXPORTS, "sacenv_selection.h")] == \
        list(_lib.SELECTION_EXPORTS)
