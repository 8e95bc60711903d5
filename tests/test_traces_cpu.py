"""Episode traces without a GPU (include/sacenv_traces.h, tests/traces_oracle.py).

* the header's functions are ``_lib.TRACES_EXPORTS``, beside the 49 of include/sacenv.h and every
  older optional header; the build lists the new unit and header;
* the descriptors and the member header have the layout of their ctypes, numpy and ``struct``
  mirrors;
* the numpy restatement, held to first principles: every episode listed, the first greatest
  taken; one case worked by hand;
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

import traces_oracle as to
from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "sacenv_traces.h")
E_NULL, E_SIZE, E_RANGE = -1, -4, -5


def _traces(**kw):
    from sacenv import _lib
    base = dict(n_envs=128, n_pad=128, members=2, envs_per_member=64, env_base=0, max_steps=8, call_steps=4, step0=0)
    base.update(kw)
    return _lib.Traces(**base)


def _steps(**kw):
    from sacenv import _lib
    base = dict(n_steps=1, step=0, rec_stride=0, obs_off=0, reward_off=44 * 128, done_off=48 * 128, term_off=49 * 128,
                final_stride=0)
    base.update(kw)
    return _lib.TraceSteps(**base)


def test_header_and_exports(built_lib):
    from sacenv import _build, _lib
    src = open(HEADER).read()
    names = set(re.findall(r"\b(sacenv_\w+)\s*\(", src))
    assert names == set(_lib.TRACES_EXPORTS) and len(_lib.TRACES_EXPORTS) == 3
    for older in (_lib.EXPORTS, _lib.EPISODE_EXPORTS, _lib.POPULATION_EXPORTS, _lib.REPLAY_POP_EXPORTS,
                  _lib.NOISE_EXPORTS, _lib.SCOREBOARD_EXPORTS, _lib.SELECTION_EXPORTS):
        assert not names & set(older)
    for n in names:
        assert hasattr(built_lib, n), n

    def define(name):
        return int(re.search(rf"#define SACENV_{name} (\d+)\b", src).group(1))

    assert define("TRACES_VERSION") == _lib.TRACES_VERSION == 1
    assert define("TRACES_MAX_MEMBERS") == _lib.TRACES_MAX_MEMBERS == 64
    assert define("TRACES_MAX_STEPS") == _lib.TRACES_MAX_STEPS
    assert define("TRACE_HEADER_BYTES") == _lib.TRACE_HEADER_BYTES == to.HEADER_BYTES == 64
    assert define("TRACE_ROW_BYTES") == _lib.TRACE_ROW_BYTES == to.ROW_BYTES == 64
    assert define("TRACE_STEP_BYTES") == _lib.TRACE_STEP_BYTES == 4 * (_lib.OBS_DIM + 2)
    assert _lib.ABI_VERSION == 20 == built_lib.sacenv_abi_version()        # sacenv.h is untouched
    rel = [r for r, _ in _build.deps()]
    assert os.path.join("include", "sacenv_traces.h") in rel
    assert os.path.join("sac-agent_amd", "csrc", "sacenv_traces.hip") in rel
    assert "sacenv_traces.hip" in _build.SOURCES and len(_build.SOURCES) == 10
    assert "sacenv_traces.h" in _build.PUBLIC_HEADERS
    text = open(os.path.join(_build.CSRC, "sacenv_traces.hip")).read()
    for inc in ("sacenv_traces.h", "sacenv_wave_core.h"):
        assert f'#include "{inc}"' in text
    assert not re.search(r'#include "[^"]+\.hip"', text)          # no source includes another
    assert not re.search(r"atomic\w*\s*\(", text)                 # no atomics decide anything
    import sacenv
    from sacenv.traces import BestEpisodes
    assert sacenv.BestEpisodes is BestEpisodes and "BestEpisodes" in sacenv.__all__


def test_structs_match_c_layout(tmp_path):
    """offsetof / sizeof of the three structs, from gcc on the header, against the ctypes mirrors,
    the numpy header dtype and the oracle's struct format."""
    from sacenv import _lib
    from sacenv.traces import HEADER_DTYPE, ROW_DTYPE
    pairs = (("SacenvTraces", _lib.Traces), ("SacenvTraceSteps", _lib.TraceSteps),
             ("SacenvTraceHeader", _lib.TraceHeader))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sacenv_traces.h"', "int main(void) {"]
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
    assert got["SacenvTraces"] == ctypes.sizeof(_lib.Traces) == 40
    assert got["SacenvTraceSteps"] == ctypes.sizeof(_lib.TraceSteps) == 64
    assert got["SacenvTraceHeader"] == ctypes.sizeof(_lib.TraceHeader) == HEADER_DTYPE.itemsize == 64
    for cname, py in pairs:
        for fname, _ in py._fields_:
            assert got[f"{cname}.{fname}"] == getattr(py, fname).offset, (cname, fname)
    for fname in HEADER_DTYPE.names:
        assert HEADER_DTYPE.fields[fname][1] == getattr(_lib.TraceHeader, fname).offset, fname
    rec = np.frombuffer(struct.pack(to.HEADER_FORMAT, 1, 2.5, 3, 4, 5, 6, 7, 0, 8), HEADER_DTYPE)[0]
    assert [rec[f].item() for f in HEADER_DTYPE.names] == [1, 2.5, 3, 4, 5, 6, 7, 8]
    assert ROW_DTYPE.itemsize == 64
    row = np.frombuffer(to.pack_row(np.arange(11), 0.5, -2.0), ROW_DTYPE)[0]
    assert row["obs"].tolist() == list(range(11)) and (row["action"], row["reward"]) == (0.5, -2.0)


def test_the_empty_state_packs_as_the_header_says():
    ora = to.TraceOracle(128, 2, 64, 8)
    got = ora.members()
    assert got == [(to.EMPTY, []), (to.EMPTY, [])]
    assert struct.unpack(to.HEADER_FORMAT, to.EMPTY) == (-1, float("-inf"), -1, 0, 0, 0, 0, 0, 0)
    assert to.EMPTY[48:] == bytes(16) and to.member_bytes(8) == 64 + 9 * 64


FAMILIES = ("distinct", "ties", "zeros", "nan", "inf", "decreasing")


def _family_steps(family, T, n, seed):
    """Steps whose episodes score what the family says: every reward is +0.0 but the ending
    step's, which is the score (one f32, so the f64 sum is that value)."""
    rng = np.random.default_rng(seed)
    done = rng.random((T, n)) < 0.2
    ends = np.argwhere(done)                         # (step, env) order
    E = len(ends)
    if family == "distinct":
        s = rng.permutation(E).astype(np.float32) - E // 2
    elif family == "ties":
        s = np.full(E, 3.75, np.float32)
    elif family == "zeros":
        s = np.where(rng.random(E) < 0.5, 0.0, -0.0).astype(np.float32)
    elif family == "nan":
        s = rng.integers(-5, 6, E).astype(np.float32)
        s[::3] = np.nan
    elif family == "inf":
        s = rng.integers(-5, 6, E).astype(np.float32)
        s[E // 4], s[E // 2], s[0] = np.inf, -np.inf, -np.inf
    else:
        s = -np.arange(E, dtype=np.float32)
    reward = np.zeros((T, n), np.float32)
    reward[done] = s
    return to.synthetic_steps(T, n, seed, done=done, reward=reward)


def _brute_force(st, n, P, N, step0=0, carry_score=None, carry_length=None):
    """Per member: every episode listed, the NaN scores dropped, the greatest score's first
    episode in (end_step, env) order -> (end_step, env, score, length, term, replaced), or None.
    `replaced`: the steps whose greatest score beats every earlier step's."""
    T = st["done"].shape[0]
    out = []
    for m in range(P):
        eps = []
        for e in range(m * N, min((m + 1) * N, n)):
            ks = np.flatnonzero(st["done"][:, e])
            lo = 0
            for k in ks:
                score = 0.0 if lo or carry_score is None else float(carry_score[e])
                with np.errstate(all="ignore"):
                    for r in st["reward"][lo: k + 1, e]:
                        score = float(np.float64(score) + np.float64(r))
                L = int(k + 1 - lo) + (0 if lo or carry_length is None else int(carry_length[e]))
                eps.append((step0 + int(k), e, score, L, int(st["term"][k, e])))
                lo = k + 1
        eps = sorted(x for x in eps if x[2] == x[2])
        if not eps:
            out.append(None)
            continue
        top = max(x[2] for x in eps)
        first = next(x for x in eps if x[2] == top)
        replaced, seen = 0, None
        for t in sorted({x[0] for x in eps}):
            here = max(x[2] for x in eps if x[0] == t)
            if seen is None or here > seen:
                replaced, seen = replaced + 1, here
        out.append((*first, replaced))
    assert T >= 1
    return out


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n,P,N", [(64, 1, 64), (70, 1, 70), (192, 2, 64), (192, 3, 64)])
def test_the_oracle_against_first_principles(n, P, N, family):
    T, R = 40, 6
    st = _family_steps(family, T, n, seed=n + P)
    rng = np.random.default_rng(5)
    carry_len = rng.integers(0, 4, n)
    carry = np.where(carry_len > 0, -0.0 if family == "zeros" else 0.0, 0.0)
    ora = to.TraceOracle(n, P, N, R, env_base=3, step0=10, carry_score=carry, carry_length=carry_len)
    ora.feed(st["obs"], st["reward"], st["done"], st["term"], st["final_obs"], st["actions"])
    want = _brute_force(st, n, P, N, 10, carry, carry_len)
    got = ora.members()
    assert any(w is not None for w in want)
    for m in range(P):
        header, rows = got[m]
        if want[m] is None:
            assert header == to.EMPTY and rows == []
            continue
        t, e, score, L, term, replaced = want[m]
        h = struct.unpack(to.HEADER_FORMAT, header)
        assert h[0] == t and h[2] == 3 + e and h[3] == L and h[4] == term and h[8] == replaced
        assert struct.pack("<d", h[1]) == struct.pack("<d", score)
        assert h[5] == len(rows) == L - h[6] + 1 and 1 <= h[5] <= R + 1
        if family == "decreasing":
            assert replaced == 1 and t == min(x for x in np.argwhere(st["done"][:, m * N: (m + 1) * N])[:, 0]) + 10
        if family == "ties":
            assert replaced == 1
    if family == "zeros":       # +0.0 and -0.0 are one score: the first ending stays
        assert all(struct.unpack(to.HEADER_FORMAT, g[0])[8] == 1 for g in got)


def test_one_case_by_hand():
    """Two envs, one member, R = 2, four steps from step 100. Env 0: rewards 1 2 | 3 4 (ends at
    steps 101 and 103: 3.0, 7.0); env 1: 5 | -1 .5 .5 (ends at 100 and 103: 5.0, 0.0). In
    (end_step, env) order the scores are 5, 3, 7, 0: 5 is kept at step 100, 7 replaces it at
    step 103, so replaced = 2 and the kept episode is env 0's second: row 0 the record's obs at
    step 101 with zeros, row 1 step 102's obs, action and reward 3, row 2 step 103's final_obs
    with its action and reward 4."""
    st = to.synthetic_steps(4, 2, seed=1, done=[[0, 1], [1, 0], [0, 0], [1, 1]],
                            reward=[[1, 5], [2, -1], [3, .5], [4, .5]])
    ora = to.TraceOracle(2, 1, 2, 2, env_base=40, step0=100)
    ora.feed(st["obs"], st["reward"], st["done"], st["term"], st["final_obs"], st["actions"])
    assert [x[:4] for x in ora.endings()] == [(100, 1, 5.0, 1), (101, 0, 3.0, 2), (103, 0, 7.0, 2), (103, 1, 0.0, 3)]
    (header, rows), = ora.members()
    assert header == struct.pack(to.HEADER_FORMAT, 103, 7.0, 40, 2, int(st["term"][3, 0]), 3, 0, 0, 2)
    assert rows == [to.pack_row(st["obs"][1, 0], 0.0, 0.0),
                    to.pack_row(st["obs"][2, 0], st["actions"][2, 0], 3.0),
                    to.pack_row(st["final_obs"][3, 0], st["actions"][3, 0], 4.0)]
    # with R = 1 the last two rows stay; attached at step 102 (carry 1.0 after one step) the
    # episode keeps its score and length and loses the rows the keeper never saw
    short = to.TraceOracle(2, 1, 2, 1, env_base=40, step0=100)
    short.feed(st["obs"], st["reward"], st["done"], st["term"], st["final_obs"], st["actions"])
    (h1, r1), = short.members()
    assert struct.unpack(to.HEADER_FORMAT, h1)[5:7] == (2, 1) and r1 == rows[1:]
    late = to.TraceOracle(2, 1, 2, 2, env_base=40, step0=103, obs0=st["obs"][2], carry_score=[3.0, -0.5],
                          carry_length=[1, 2])
    late.feed(*(st[f][3:] for f in ("obs", "reward", "done", "term", "final_obs", "actions")))
    (h2, r2), = late.members()
    assert struct.unpack(to.HEADER_FORMAT, h2) == (103, 7.0, 40, 2, int(st["term"][3, 0]), 1, 2, 0, 1)
    assert r2 == rows[2:]


def test_argument_errors_are_found_on_the_host(built_lib):
    """Each error returns its code before anything is launched (no device here): pointers are
    made-up addresses that are never followed."""
    lib = built_lib
    mb, sb = ctypes.c_int64(-7), ctypes.c_int64(-7)
    good, one, p = _traces(), _steps(), 0x10000
    R = ctypes.byref
    assert lib.sacenv_traces_bytes(R(good), R(mb), R(sb)) == 0
    assert mb.value == 2 * to.member_bytes(8) and sb.value == to.store_bytes(128, 8, 4)
    assert lib.sacenv_traces_bytes(None, R(mb), R(sb)) == E_NULL
    assert lib.sacenv_traces_bytes(R(good), None, R(sb)) == E_NULL
    assert lib.sacenv_traces_bytes(R(good), R(mb), None) == E_NULL
    size = [dict(n_envs=0), dict(n_pad=64), dict(n_pad=130, n_envs=130), dict(members=0), dict(members=65),
            dict(envs_per_member=0), dict(members=2, envs_per_member=65),        # a wave would straddle two members
            dict(members=3, envs_per_member=64),                                 # members x envs_per_member > n_envs
            dict(members=1, envs_per_member=129), dict(env_base=-1), dict(env_base=2 ** 31 - 100),
            dict(max_steps=0), dict(max_steps=(1 << 20) + 1), dict(call_steps=0), dict(call_steps=(1 << 20) + 1),
            dict(step0=-1)]
    for kw in size:
        t = _traces(**kw)
        assert lib.sacenv_traces_bytes(R(t), R(mb), R(sb)) == E_SIZE, kw
        assert lib.sacenv_traces_init(R(t), p, p, p, p, p, None) == E_SIZE, kw
        assert lib.sacenv_traces_update(R(t), R(one), p, p, p, p, p, None) == E_SIZE, kw
    assert mb.value == 2 * to.member_bytes(8)
    # init: the two buffers are required, the rest may be NULL; alignment
    assert lib.sacenv_traces_init(None, p, p, p, p, p, None) == E_NULL
    assert lib.sacenv_traces_init(R(good), p, p, p, None, p, None) == E_NULL
    assert lib.sacenv_traces_init(R(good), p, p, p, p, None, None) == E_NULL
    for k, off in ((0, 2), (1, 4), (2, 2), (3, 8), (4, 8)):
        ptrs = [p] * 5
        ptrs[k] += off
        assert lib.sacenv_traces_init(R(good), *ptrs, None) == E_RANGE, k
    # update
    for k in range(7):
        args = [R(good), R(one), p, p, p, p, p]
        args[k] = None
        assert lib.sacenv_traces_update(*args, None) == E_NULL, k
    for kw in (dict(n_steps=0), dict(n_steps=5, rec_stride=6400, final_stride=5632)):    # n_steps > call_steps
        assert lib.sacenv_traces_update(R(good), R(_steps(**kw)), p, p, p, p, p, None) == E_SIZE, kw
    many = dict(n_steps=4, rec_stride=6400, final_stride=5632)
    rng = [dict(obs_off=-4), dict(reward_off=-4), dict(done_off=-1), dict(term_off=-1), dict(rec_stride=-4),
           dict(final_stride=-4), dict(obs_off=2), dict(reward_off=2), dict(step=-1),
           dict(many, rec_stride=0), dict(many, rec_stride=6402), dict(many, final_stride=0),
           dict(many, final_stride=5634)]
    for kw in rng:
        assert lib.sacenv_traces_update(R(good), R(_steps(**kw)), p, p, p, p, p, None) == E_RANGE, kw
    assert lib.sacenv_traces_update(R(_traces(step0=9)), R(_steps(step=8)), p, p, p, p, p, None) == E_RANGE
    for k, off in ((0, 2), (1, 2), (2, 2), (3, 8), (4, 8)):
        ptrs = [p] * 5
        ptrs[k] += off
        assert lib.sacenv_traces_update(R(good), R(one), *ptrs, None) == E_RANGE, k
    # the limits themselves pass
    for kw in (dict(members=1, envs_per_member=70, n_envs=70), dict(members=64, envs_per_member=64, n_envs=4096, n_pad=4096),
               dict(max_steps=1 << 20, call_steps=1 << 20), dict(members=1, envs_per_member=1)):
        assert lib.sacenv_traces_bytes(R(_traces(**kw)), R(mb), R(sb)) == 0, kw


def test_lib_loads_a_library_without_the_traces_entry_points(built_lib, tmp_path):
    """``SACENV_LIB`` may point at a build from before sacenv_traces.h (a stand-in that exports
    every older name and not the new ones); ``require`` then says what to do."""
    from sacenv import _lib
    older = (_lib.EXPORTS + _lib.EPISODE_EXPORTS + _lib.POPULATION_EXPORTS + _lib.REPLAY_POP_EXPORTS +
             _lib.NOISE_EXPORTS + _lib.SCOREBOARD_EXPORTS + _lib.SELECTION_EXPORTS)
    body = ["int sacenv_abi_version(void) { return %d; }" % _lib.ABI_VERSION]
    body += [f"int {n}(void) {{ return 0; }}" for n in older if n != "sacenv_abi_version"]
    src = tmp_path / "old.c"
    src.write_text("\n".join(body))
    so = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = _lib.load(str(so))
    assert not any(hasattr(lib, n) for n in _lib.TRACES_EXPORTS)
    assert all(hasattr(lib, n) for n in _lib.SELECTION_EXPORTS)
    with pytest.raises(_lib.SacenvError, match="sacenv_traces.h"):
        _lib.require(_lib.TRACES_EXPORTS, "sacenv_traces.h", lib)
    assert [f.__name__ for f in _lib.require(_lib.TRACES_EXPORTS, "sacenv_traces.h")] == list(_lib.TRACES_EXPORTS)


def test_the_host_class_refuses_what_it_cannot_keep():
    """The constructor's refusals come before anything touches a device."""
    from sacenv.toys import VecToyEnv
    from sacenv.traces import BestEpisodes
    with pytest.raises(ValueError, match="VecBoatEnv"):
        BestEpisodes(object.__new__(VecToyEnv), members=1, envs_per_member=64)
