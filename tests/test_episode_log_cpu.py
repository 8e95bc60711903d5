"""The episode log's C ABI without a GPU (include/sacenv_episodes.h).

* the library exports both entry points, beside the 49 of include/sacenv.h and
  outside ``_lib.EXPORTS`` (the ABI of sacenv.h does not move);
* ``SacenvEpisodeScan`` has the layout of its ctypes mirror (gcc offsetof probe);
* every argument error is found on the host, before anything is launched.
"""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")


def _scan(**kw):
    from sacenv import _lib
    base = dict(n_envs=200, n_pad=256, n_steps=32, env_base=0, rec_stride=50 * 256, reward_off=44 * 256,
                done_off=48 * 256, term_off=49 * 256, step0=0, cap=1024)
    base.update(kw)
    return _lib.EpisodeScan(**base)


def test_library_exports_the_episode_entry_points(built_lib):
    from sacenv import _lib
    assert _lib.EPISODE_EXPORTS == ("sacenv_episodes_scratch_bytes", "sacenv_episodes_update")
    for n in _lib.EPISODE_EXPORTS:
        assert hasattr(built_lib, n), n
        assert n not in _lib.EXPORTS
    names = set(re.findall(r"\b(sacenv_\w+)\s*\(", open(os.path.join(INCLUDE, "sacenv.h")).read()))
    assert len(names) == 49 and names == set(_lib.EXPORTS)
    new = set(re.findall(r"\b(sacenv_\w+)\s*\(", open(os.path.join(INCLUDE, "sacenv_episodes.h")).read()))
    assert set(_lib.EPISODE_EXPORTS) <= new
    src = open(os.path.join(INCLUDE, "sacenv_episodes.h")).read()
    assert int(re.search(r"#define SACENV_EPISODES_VERSION (\d+)", src).group(1)) == _lib.EPISODES_VERSION == 1
    assert _lib.ABI_VERSION == 20 == built_lib.sacenv_abi_version()


def test_episode_scan_struct_matches_c_layout(tmp_path):
    """offsetof/sizeof of SacenvEpisodeScan, from gcc on the header, vs the ctypes mirror."""
    from sacenv import _lib
    py = _lib.EpisodeScan
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sacenv_episodes.h"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(SacenvEpisodeScan));',
             'printf("entry %d\\n", SACENV_EPISODE_ENTRY_BYTES);']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(SacenvEpisodeScan, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[0]: int(l.split()[1]) for l in out if l.strip()}
    assert got["sizeof"] == ctypes.sizeof(py) == 64
    assert got["entry"] == _lib.EPISODE_ENTRY_BYTES == 32
    for fname, _ in py._fields_:
        assert got[fname] == getattr(py, fname).offset, fname
    from sacenv.episodes import ENTRY_DTYPE
    assert ENTRY_DTYPE.itemsize == 32
    assert [ENTRY_DTYPE.fields[f][1] for f in ("end_step", "score", "env", "length", "term")] == [0, 8, 16, 20, 24]


def test_scratch_size_grows_with_steps_and_waves(built_lib):
    need = ctypes.c_int64()
    size = built_lib.sacenv_episodes_scratch_bytes
    got = {}
    for K, NP in ((1, 64), (1, 256), (32, 256), (256, 256), (256, 65536)):
        assert size(ctypes.byref(_scan(n_steps=K, n_pad=NP, n_envs=NP)), ctypes.byref(need)) == 0
        got[(K, NP)] = need.value
        assert need.value >= 16 * K * NP // 64      # a count and its scan (u64 each) per step and wave
        assert need.value % 16 == 0
    assert got[(1, 64)] < got[(1, 256)] < got[(32, 256)] < got[(256, 256)] < got[(256, 65536)]
    assert got[(256, 65536)] - got[(256, 256)] == 16 * 256 * (65536 - 256) // 64
    assert size(None, ctypes.byref(need)) == -1
    assert size(ctypes.byref(_scan()), None) == -1


def test_argument_errors_without_gpu(built_lib):
    """Every rule of sacenv_episodes_update, none of which launches (there is no device here).
    Pointers are plain numbers with the alignment under test."""
    update = built_lib.sacenv_episodes_update
    size = built_lib.sacenv_episodes_scratch_bytes
    need = ctypes.c_int64()
    assert size(ctypes.byref(_scan()), ctypes.byref(need)) == 0
    REC, CARRY, LOG, SCR = 1 << 20, 2 << 20, 3 << 20, 4 << 20

    def call(s=None, rec=REC, carry=CARRY, log=LOG, scr=SCR, nb=None):
        s = _scan() if s is None else s
        return update(ctypes.byref(s), rec, carry, log, scr, need.value if nb is None else nb, None)

    # NULL pointers
    assert update(None, REC, CARRY, LOG, SCR, need.value, None) == -1
    for k in ("rec", "carry", "log", "scr"):
        assert call(**{k: None}) == -1, k
    # sizes
    for bad in (dict(n_envs=0), dict(n_envs=257), dict(n_pad=200, n_envs=200), dict(n_pad=0, n_envs=0),
                dict(n_steps=0), dict(n_steps=-1), dict(cap=-1), dict(env_base=-1),
                dict(env_base=2**31 - 100),
                dict(n_steps=2**31 - 1, n_pad=64, n_envs=64),            # K x n_pad / 64 = 2^31 - 1: a size
                dict(n_steps=2**25, n_pad=4096, n_envs=4096)):           # = 2^31
        s = _scan(**bad)
        # (2^31 - 1 items is a size the library accepts: refused here for its scratch alone)
        want = 0 if bad.get("n_steps") == 2**31 - 1 else -4
        assert size(ctypes.byref(s), ctypes.byref(ctypes.c_int64())) == want, bad
        assert call(s) == -4, bad
    assert call(nb=need.value - 1) == -4
    assert call(nb=0) == -4
    # ranges
    for bad in (dict(reward_off=44 * 256 + 2), dict(reward_off=-4), dict(done_off=-1), dict(term_off=-1),
                dict(rec_stride=0), dict(rec_stride=-50 * 256), dict(rec_stride=50 * 256 + 2)):
        assert call(_scan(**bad)) == -5, bad
    assert call(rec=REC + 2) == -5
    assert call(log=LOG + 8) == -5
    assert call(carry=CARRY + 4) == -5
    assert call(scr=SCR + 8) == -5
    # one step needs no stride
    s1 = _scan(n_steps=1, rec_stride=0)
    assert size(ctypes.byref(s1), ctypes.byref(need)) == 0
    assert call(s1, nb=need.value - 1) == -4     # past every argument check, stopped by the scratch size


def test_lib_loads_a_library_without_the_episode_entry_points(built_lib, tmp_path):
    """``SACENV_LIB`` may point at a build from before sacenv_episodes.h: ``_lib.load`` binds the
    new names only where they exist (checked with a stand-in that exports the version alone)."""
    from sacenv import _lib
    src = tmp_path / "old.c"
    body = ["int sacenv_abi_version(void) { return %d; }" % _lib.ABI_VERSION]
    body += [f"int {n}(void) {{ return 0; }}" for n in _lib.EXPORTS if n != "sacenv_abi_version"]
    src.write_text("\n".join(body))
    so = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = _lib.load(str(so))
    assert lib.sacenv_abi_version() == _lib.ABI_VERSION
    assert not any(hasattr(lib, n) for n in _lib.EPISODE_EXPORTS)
