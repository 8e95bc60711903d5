"""The population replay's C interface without a GPU (include/sacenv_population_replay.h).

* the library exports the five entry points beside the 49 of include/sacenv.h and outside
  ``_lib.EXPORTS``, ``EPISODE_EXPORTS`` and ``POPULATION_EXPORTS`` (the ABI of sacenv.h does not
  move), and ``_lib.load`` still takes a library without them;
* ``SacenvReplayPopLayout`` has the layout of its ctypes mirror;
* ``sacenv_replay_pop_layout`` is P x ``sacenv_replay_layout``'s total;
* every argument error is found on the host, before anything is launched.
"""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "sacenv_population_replay.h")
E_NULL, E_SIZE, E_RANGE = -1, -4, -5
NAMES = ("sacenv_replay_pop_layout", "sacenv_replay_pop_init", "sacenv_replay_pop_store",
         "sacenv_replay_pop_sample", "sacenv_replay_pop_gather")


def _params(M=100, D=11, A=1, reward_f32=1, mask=2):
    from sacenv import _lib
    p = _lib.ReplayParams()
    p.mem_size, p.obs_dim, p.act_dim, p.reward_f32, p.terminal_mask = M, D, A, reward_f32, mask
    return p


def test_library_exports_the_population_replay_entry_points(built_lib):
    from sacenv import _build, _lib
    assert _lib.REPLAY_POP_EXPORTS == NAMES
    for n in NAMES:
        assert hasattr(built_lib, n), n
        assert n not in _lib.EXPORTS and n not in _lib.EPISODE_EXPORTS and n not in _lib.POPULATION_EXPORTS
    src = open(HEADER).read()
    assert set(re.findall(r"\b(sacenv_\w+)\s*\(", src)) == set(NAMES)
    assert int(re.search(r"#define SACENV_REPLAY_POP_VERSION (\d+)", src).group(1)) == _lib.REPLAY_POP_VERSION == 1
    assert int(re.search(r"#define SACENV_REPLAY_POP_MAX_MEMBERS (\d+)", src).group(1)) \
        == _lib.REPLAY_POP_MAX_MEMBERS == 64
    assert _lib.ABI_VERSION == 20 == built_lib.sacenv_abi_version()
    rel = [r for r, _ in _build.deps()]
    assert os.path.join("include", "sacenv_population_replay.h") in rel
    assert os.path.join("sac-agent_amd", "csrc", "sacenv_replay_pop.hip") in rel
    assert "sacenv_replay_pop.hip" in _build.SOURCES


def test_lib_loads_a_library_without_the_population_replay_entry_points(built_lib, tmp_path):
    """``SACENV_LIB`` may point at a build from before sacenv_population_replay.h (a stand-in
    that exports every older name and none of the five)."""
    from sacenv import _lib
    src = tmp_path / "old.c"
    body = ["int sacenv_abi_version(void) { return %d; }" % _lib.ABI_VERSION]
    older = _lib.EXPORTS + _lib.EPISODE_EXPORTS + _lib.POPULATION_EXPORTS
    body += [f"int {n}(void) {{ return 0; }}" for n in older if n != "sacenv_abi_version"]
    src.write_text("\n".join(body))
    so = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = _lib.load(str(so))
    assert lib.sacenv_abi_version() == _lib.ABI_VERSION
    assert not any(hasattr(lib, n) for n in NAMES)
    assert all(hasattr(lib, n) for n in _lib.POPULATION_EXPORTS)


def test_pop_layout_struct_matches_c_layout(tmp_path):
    """offsetof/sizeof from gcc on the header against the ctypes mirror."""
    from sacenv import _lib
    cname, py = "SacenvReplayPopLayout", _lib.ReplayPopLayout
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sacenv_population_replay.h"', "int main(void) {",
             f'printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _t in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[0]: int(l.split()[1]) for l in out if l.strip()}
    assert got[cname] == ctypes.sizeof(py) == 24
    assert [f for f, _ in py._fields_] == ["member_bytes", "total_bytes", "max_members", "pad"]
    for fname, _t in py._fields_:
        assert got[fname] == getattr(py, fname).offset, fname


@pytest.mark.parametrize("M,D,A", [(100, 11, 1), (1 << 14, 1, 1), (50, 14, 2)])
def test_pop_layout_follows_the_one_buffer_layout(built_lib, M, D, A):
    from sacenv import _lib
    p = _params(M, D, A)
    one = _lib.replay_layout(p)
    for P in (1, 3, 64):
        L = _lib.ReplayPopLayout()
        assert built_lib.sacenv_replay_pop_layout(ctypes.byref(p), P, ctypes.byref(L)) == 0
        assert L.member_bytes == one.total_bytes and L.member_bytes % 256 == 0
        assert L.total_bytes == P * L.member_bytes
        assert L.max_members == 64 and L.pad == 0
        got = _lib.replay_pop_layout(p, P)
        assert (got.member_bytes, got.total_bytes) == (L.member_bytes, L.total_bytes)


BAD_PARAMS = (dict(M=0), dict(M=-5), dict(M=1 << 31), dict(D=0), dict(A=0), dict(A=-1))


def test_argument_errors_without_gpu(built_lib):
    """Every rule of the five entry points, none of which launches (there is no device here).
    Pointers are plain numbers with the alignment under test."""
    lib, cap = built_lib, 64
    pp = ctypes.byref(_params())
    AR, X = 1 << 20, 3 << 20          # (256-B aligned)
    from sacenv import _lib
    L = _lib.ReplayPopLayout()
    seeds = (ctypes.c_uint32 * cap)()

    # layout
    assert lib.sacenv_replay_pop_layout(None, 2, ctypes.byref(L)) == E_NULL
    assert lib.sacenv_replay_pop_layout(pp, 2, None) == E_NULL
    for m in (0, -1, cap + 1):
        assert lib.sacenv_replay_pop_layout(pp, m, ctypes.byref(L)) == E_SIZE, m
    for bad in BAD_PARAMS:
        assert lib.sacenv_replay_pop_layout(ctypes.byref(_params(**bad)), 2, ctypes.byref(L)) == E_SIZE, bad

    # init
    assert lib.sacenv_replay_pop_init(None, 2, AR, seeds, None) == E_NULL
    assert lib.sacenv_replay_pop_init(pp, 2, None, seeds, None) == E_NULL
    assert lib.sacenv_replay_pop_init(pp, 2, AR, None, None) == E_NULL
    for m in (0, -2, cap + 1):
        assert lib.sacenv_replay_pop_init(pp, m, AR, seeds, None) == E_SIZE, m
    for off in (4, 64, 128):
        assert lib.sacenv_replay_pop_init(pp, 2, AR + off, seeds, None) == E_SIZE, off
    for bad in BAD_PARAMS:
        assert lib.sacenv_replay_pop_init(ctypes.byref(_params(**bad)), 2, AR, seeds, None) == E_SIZE, bad

    # store
    def store(p=pp, m=2, ar=AR, cntr=0, n=64, s=X, a=X, r=X, s2=X, fs=X, c=X, lt=X):
        return lib.sacenv_replay_pop_store(p, m, ar, cntr, n, s, a, r, s2, fs, c, lt, None)

    assert store(p=None) == E_NULL
    for k in ("ar", "s", "a", "r", "s2", "c"):
        assert store(**{k: None}) == E_NULL, k
    for m in (0, -1, cap + 1):
        assert store(m=m) == E_SIZE, m
    for bad in BAD_PARAMS:
        assert store(p=ctypes.byref(_params(**bad))) == E_SIZE, bad
    assert store(n=-1) == E_SIZE
    for cntr in (-2, -100):
        assert store(cntr=cntr) == E_RANGE, cntr
    assert store(ar=AR + 128) == E_SIZE
    assert store(n=0) == 0                               # no rows: OK, and nothing is launched
    assert store(n=0, cntr=-1) == 0
    assert store(n=0, ar=None, s=None, a=None, r=None, s2=None, c=None, fs=None, lt=None) == 0
    assert store(n=0, m=cap + 1) == E_SIZE               # the members are checked before the rows
    # a member's element count of one call: rows x (D + A + 1) (+ the dropped rows with last_term) < 2^32
    big = ctypes.byref(_params(M=(1 << 31) - 1))
    assert store(p=big, n=1 << 29) == E_SIZE             # 2^29 x 13 >= 2^32
    small = ctypes.byref(_params(M=4))
    assert store(p=small, n=1 << 32) == E_SIZE           # 4 rows stored, 2^32 - 4 bytes of last_term + 52

    # sample
    def sample(p=pp, m=2, ar=AR, batch=256, stored=10, idx=X, s=X, a=X, r=X, s2=X, t=X):
        return lib.sacenv_replay_pop_sample(p, m, ar, batch, stored, idx, s, a, r, s2, t, None)

    assert sample(p=None) == E_NULL
    for k in ("ar", "idx"):
        assert sample(**{k: None}) == E_NULL, k
    for m in (0, -1, cap + 1):
        assert sample(m=m) == E_SIZE, m
    for bad in BAD_PARAMS:
        assert sample(p=ctypes.byref(_params(**bad))) == E_SIZE, bad
    assert sample(batch=-1) == E_SIZE
    for stored in (0, -1):
        assert sample(stored=stored) == E_SIZE, stored
        assert sample(stored=stored, batch=0) == E_SIZE, stored
    assert sample(ar=AR + 64) == E_SIZE
    assert sample(batch=(1 << 31) - 1) == E_SIZE         # (2^31 - 1) x 13 >= 2^32
    assert sample(batch=0) == 0                          # nothing to draw: OK, nothing launched
    assert sample(batch=0, s=None, a=None, r=None, s2=None, t=None) == 0
    assert sample(batch=0, idx=None) == E_NULL           # idx is required, as in sacenv_replay_sample
    assert sample(batch=0, m=cap + 1) == E_SIZE

    # gather
    def gather(p=pp, m=2, ar=AR, batch=256, idx=X, s=X, a=X, r=X, s2=X, t=X):
        return lib.sacenv_replay_pop_gather(p, m, ar, batch, idx, s, a, r, s2, t, None)

    assert gather(p=None) == E_NULL
    for k in ("ar", "idx"):
        assert gather(**{k: None}) == E_NULL, k
    for m in (0, -1, cap + 1):
        assert gather(m=m) == E_SIZE, m
    for bad in BAD_PARAMS:
        assert gather(p=ctypes.byref(_params(**bad))) == E_SIZE, bad
    assert gather(batch=-1) == E_SIZE
    assert gather(ar=AR + 8) == E_SIZE
    assert gather(batch=(1 << 31) - 1) == E_SIZE
    assert gather(batch=0) == 0
    assert gather(batch=0, s=None, a=None, r=None, s2=None, t=None) == 0   # the outputs may be NULL
    assert gather(batch=0, m=cap + 1) == E_SIZE


def test_python_side_without_a_device(built_lib):
    """What the host classes refuse before touching the device."""
    import sacenv
    from sacenv.population_replay import PopulationReplay
    assert sacenv.PopulationReplay is PopulationReplay
    with pytest.raises(RuntimeError, match="GPU"):
        PopulationReplay(2, 100, (11,), 1, device="cpu")
