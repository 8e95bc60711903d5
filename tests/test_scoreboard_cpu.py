"""The population scoreboard without a GPU (include/sacenv_scoreboard.h).

* the header's functions are ``_lib.SCOREBOARD_EXPORTS``, beside the 49 of include/sacenv.h and
  every older optional header; the build lists the unit and its headers, and the episode log's
  unit defines none of them;
* ``SacenvBoard`` and the 128-B member record have the layout of their ctypes and numpy mirrors;
* the Python restatement (tests/scoreboard_oracle.py) against the literal lines of the
  reference (a list and ``np.mean(history[-L:])``), field by field and bit for bit, and the C++
  mean the kernels use, compiled for the host, against ``np.mean``;
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

import scoreboard_oracle as so
from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "sacenv_scoreboard.h")
LOOKBACKS = (1, 2, 7, 8, 9, 16, 17, 50, 127, 128)


def _board(**kw):
    from sacenv import _lib
    base = dict(members=4, envs_per_member=64, env_base=0, lookback=50, cap=1024, member_floats=0)
    base.update(kw)
    return _lib.Board(**base)


def _bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _same(a: float, b: float) -> bool:
    """Equal bit for bit; two NaNs count as equal (IEEE 754 leaves the sign and payload of a
    generated NaN open: inf - inf is the negative quiet NaN on x86 and the positive one on
    other hardware, and no comparison tells them apart)."""
    return (a != a and b != b) or _bits(a) == _bits(b)


def test_header_and_exports(built_lib):
    from sacenv import _build, _lib
    src = open(HEADER).read()
    names = set(re.findall(r"\b(sacenv_\w+)\s*\(", src))
    assert names == set(_lib.SCOREBOARD_EXPORTS) and len(_lib.SCOREBOARD_EXPORTS) == 4
    for older in (_lib.EXPORTS, _lib.EPISODE_EXPORTS, _lib.POPULATION_EXPORTS, _lib.REPLAY_POP_EXPORTS,
                  _lib.NOISE_EXPORTS):
        assert not names & set(older)
    for n in names:
        assert hasattr(built_lib, n), n
    assert int(re.search(r"#define SACENV_SCOREBOARD_VERSION (\d+)", src).group(1)) == _lib.SCOREBOARD_VERSION == 1
    assert int(re.search(r"#define SACENV_BOARD_MAX_LOOKBACK (\d+)", src).group(1)) == _lib.BOARD_MAX_LOOKBACK == 128
    assert int(re.search(r"#define SACENV_BOARD_MAX_MEMBERS (\d+)", src).group(1)) == _lib.BOARD_MAX_MEMBERS == 64
    main = set(re.findall(r"\b(sacenv_\w+)\s*\(", open(os.path.join(INCLUDE, "sacenv.h")).read()))
    assert len(main) == 49 and main == set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 20 == built_lib.sacenv_abi_version()
    rel = [r for r, _ in _build.deps()]
    assert os.path.join("include", "sacenv_scoreboard.h") in rel
    assert os.path.join("sac-agent_amd", "csrc", "sacenv_board_core.h") in rel
    assert "sacenv_board.hip" in _build.SOURCES
    assert os.path.join("sac-agent_amd", "csrc", "sacenv_board.hip") in rel
    text = open(os.path.join(_build.CSRC, "sacenv_board.hip")).read()
    for inc in ("sacenv_board_core.h", "sacenv_scoreboard.h"):
        assert f'#include "{inc}"' in text
    for n in names:                                          # each entry point is defined there, once
        assert len(re.findall(rf"^int {n}\(", text, re.M)) == 1, n
    assert "sacenv_board_" not in open(os.path.join(_build.CSRC, "sacenv_episodes.hip")).read()
    import sacenv
    from sacenv.scoreboard import MemberScoreboard
    assert sacenv.MemberScoreboard is MemberScoreboard and "MemberScoreboard" in sacenv.__all__


def test_structs_match_c_layout(tmp_path):
    """offsetof / sizeof of SacenvBoard and SacenvBoardMember, from gcc on the header, against the
    ctypes mirrors and the numpy record dtype."""
    from sacenv import _lib
    from sacenv.scoreboard import MEMBER_DTYPE
    pairs = (("SacenvBoard", _lib.Board), ("SacenvBoardMember", _lib.BoardMember))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sacenv_scoreboard.h"', "int main(void) {",
             'printf("header %d\\n", SACENV_BOARD_HEADER_BYTES);', 'printf("member %d\\n", SACENV_BOARD_MEMBER_BYTES);']
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
    assert got["header"] == _lib.BOARD_HEADER_BYTES == so.HEADER_BYTES == 32
    assert got["member"] == _lib.BOARD_MEMBER_BYTES == so.MEMBER_BYTES == MEMBER_DTYPE.itemsize == 128
    assert got["SacenvBoard"] == ctypes.sizeof(_lib.Board) == 32
    assert got["SacenvBoardMember"] == ctypes.sizeof(_lib.BoardMember) == 128
    for cname, py in pairs:
        for fname, _ in py._fields_:
            assert got[f"{cname}.{fname}"] == getattr(py, fname).offset, (cname, fname)
    for fname, _ in _lib.BoardMember._fields_:
        assert MEMBER_DTYPE.fields[fname][1] == getattr(_lib.BoardMember, fname).offset, fname
    # the oracle's struct format packs the same record
    vals = (1, 2, 3, 4, 5.0, 6.0, 7.0, 8, 0, *range(10, 18))
    rec = np.frombuffer(struct.pack(so.MEMBER_FORMAT, *vals), MEMBER_DTYPE)[0]
    assert [int(rec[f]) for f in ("episodes", "saves", "last_save_step", "last_end_step")] == [1, 2, 3, 4]
    assert [float(rec[f]) for f in ("last", "best", "avg")] == [5.0, 6.0, 7.0]
    assert int(rec["saved_now"]) == 8 and rec["terms"].tolist() == list(range(10, 18))


def _reference_loop(scores, end_steps, L):
    """main.py:99-108 as written: yields (avg, best, saves, last_save_step) after every episode."""
    score_history, best_score, saves, last_save = [], float("-inf"), 0, -1
    with np.errstate(all="ignore"):
        for score, end in zip(scores.tolist(), end_steps):
            score_history.append(score)
            avg_score = np.mean(score_history[-L:])
            if score > best_score:
                best_score = score
            if score > avg_score:
                saves, last_save = saves + 1, end
            yield float(avg_score), best_score, saves, last_save


@pytest.mark.parametrize("family", so.FAMILIES)
@pytest.mark.parametrize("L", LOOKBACKS)
def test_oracle_is_the_reference_loop(L, family):
    scores = so.scores(family, 300, L, seed=L)
    ends = [3 * i + 1 for i in range(300)]
    mem = so.Member()
    zero = up = down = 0
    with np.errstate(all="ignore"):
        for i, (avg, best, saves, last_save) in enumerate(_reference_loop(scores, ends, L)):
            mem.episode(scores[i], ends[i], 1 + i % 6, L)
            assert _same(mem.avg, avg), (i, mem.avg, avg)
            assert _same(mem.best, best), i
            assert (mem.saves, mem.last_save_step) == (saves, last_save), i
            s = float(scores[i])
            zero += s == avg
            up += s == np.nextafter(avg, np.inf)
            down += s == np.nextafter(avg, -np.inf)
    assert mem.episodes == 300 and sum(mem.terms) == 300 and mem.terms[0] == mem.terms[7] == 0
    if family == "equal":
        assert mem.saves == 0 and zero == 300
    if family == "negzero":
        assert mem.saves == 0 and _bits(mem.avg) == _bits(float(np.mean([-0.0] * min(L, 300)))) == _bits(0.0)
    if family == "nan":
        assert mem.best == mem.best               # a NaN never became best
    if family == "ties":
        assert zero > 0 and (L == 1 or (up > 0 and down > 0)), (zero, up, down)


def test_written_out_sum_is_numpys():
    """``np_mean`` against ``np.mean`` on random lists of every length 1..128."""
    rng = np.random.default_rng(1)
    for trial in range(4000):
        n = 1 + trial % 128
        xs = (10.0 ** rng.uniform(-3, 6, n) * rng.choice([-1.0, 1.0], n)).tolist()
        assert _bits(so.np_mean(xs)) == _bits(float(np.mean(xs))), n


def test_kernel_mean_compiled_for_the_host_is_numpys(tmp_path):
    """``sacenv_board::mean_np`` (csrc/sacenv_board_core.h), the function the update kernel calls,
    built with g++ under the library's ``-ffp-contract=off``: equal to ``np.mean`` bit for bit on
    windows of every length 1..128, the special values among them."""
    from sacenv import _build
    rng = np.random.default_rng(2)
    cases = []
    for trial in range(2000):
        n = 1 + trial % 128
        cases.append(10.0 ** rng.uniform(-3, 6, n) * rng.choice([-1.0, 1.0], n))
    for L in (1, 7, 8, 9, 50, 128):
        cases += [np.full(L, -0.0), np.full(L, 3.7), np.full(L, 3.75), so.scores("ties", L, L)]
    blob = b"".join(struct.pack("<i", len(c)) + np.asarray(c, "<f8").tobytes() for c in cases)
    (tmp_path / "in.bin").write_bytes(blob)
    src = tmp_path / "probe.cpp"
    src.write_text("""
#include <stdio.h>
#include "sacenv_board_core.h"
int main(int argc, char** argv) {
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  int n;
  double p[128];
  while (fread(&n, 4, 1, in) == 1) {
    if (n < 1 || n > 128 || fread(p, 8, n, in) != (size_t)n) return 1;
    const double m = sacenv_board::mean_np(p, n);
    fwrite(&m, 8, 1, out);
  }
  fclose(out);
  return 0;
}
""")
    exe = tmp_path / "probe"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", INCLUDE, "-I", _build.CSRC, str(src),
                    "-o", str(exe)], check=True)
    subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), "<f8")
    assert got.size == len(cases)
    for c, g in zip(cases, got):
        assert _bits(float(g)) == _bits(float(np.mean(c.tolist()))), len(c)


def test_oracle_cursor_overflow_and_pack():
    """The restatement's own bookkeeping: cursor, missed, rewind, envs outside the members, and
    the packed size."""
    from sacenv.episodes import ENTRY_DTYPE
    cap = 10
    entries = np.zeros(cap, ENTRY_DTYPE)
    entries["env"] = [0, 1, 2, 3, 4, 5, 6, 7, 1, 2]
    entries["score"] = np.arange(cap, dtype=np.float64)
    entries["end_step"] = np.arange(cap)
    entries["term"] = [1, 2, 3, 4, 5, 6, 7, 9, 1, 1]
    o = so.BoardOracle(2, 2, 3, cap, env_base=2)        # member 0: envs 2, 3; member 1: envs 4, 5
    assert o.update(4, entries) == [0] and (o.cursor, o.missed, o.calls) == (4, 0, 1)
    assert [m.episodes for m in o.members] == [2, 0]
    o.update(cap + 5, entries)
    assert (o.cursor, o.missed) == (cap + 5, 5) and [m.episodes for m in o.members] == [3, 2]
    o.update(cap + 5, entries)
    assert (o.cursor, o.missed, o.calls) == (cap + 5, 5, 3)
    o.update(3, entries)                                  # a total below the cursor: nothing new
    assert o.cursor == cap + 5 and [m.episodes for m in o.members] == [3, 2]
    o.rewind()
    o.update(3, entries)
    assert o.cursor == 3 and [m.episodes for m in o.members] == [4, 2]
    assert o.members[0].history == [2.0, 3.0, 9.0, 2.0]
    assert len(o.pack()) == 32 + 2 * 128 + 2 * 3 * 8
    ring0 = struct.unpack("<3d", o.pack()[32 + 256: 32 + 256 + 24])
    assert ring0 == (2.0, 3.0, 9.0)                       # episode 3 (score 2.0) in slot 3 % 3 = 0


def test_argument_errors_without_gpu(built_lib):
    """Every rule of the four entry points, none of which launches (there is no device here).
    Pointers are plain numbers with the alignment under test."""
    size, init, update, rewind = (getattr(built_lib, n) for n in
                                  ("sacenv_board_bytes", "sacenv_board_init", "sacenv_board_update",
                                   "sacenv_board_rewind"))
    need = ctypes.c_int64()
    assert size(ctypes.byref(_board()), ctypes.byref(need)) == 0
    assert need.value == 32 + 4 * 128 + 4 * 50 * 8
    assert size(ctypes.byref(_board(members=64, lookback=128)), ctypes.byref(need)) == 0
    assert need.value == 32 + 64 * 128 + 64 * 128 * 8
    LOG, BRD, W, S = 1 << 20, 2 << 20, 3 << 20, 4 << 20
    B = ctypes.byref
    # NULL
    assert size(None, B(need)) == -1 and size(B(_board()), None) == -1
    assert init(None, BRD, None) == -1 and init(B(_board()), None, None) == -1
    assert rewind(None, BRD, None) == -1 and rewind(B(_board()), None, None) == -1
    assert update(None, LOG, BRD, None, None, None) == -1
    assert update(B(_board()), None, BRD, None, None, None) == -1
    assert update(B(_board()), LOG, None, None, None, None) == -1
    # sizes
    for bad in (dict(members=0), dict(members=65), dict(lookback=0), dict(lookback=129), dict(envs_per_member=0),
                dict(env_base=-1), dict(cap=-1), dict(member_floats=6), dict(member_floats=-4)):
        b = _board(**bad)
        assert size(B(b), B(need)) == -4, bad
        assert init(B(b), BRD, None) == -4, bad
        assert update(B(b), LOG, BRD, None, None, None) == -4, bad
        assert rewind(B(b), BRD, None) == -4, bad
    # ranges
    assert init(B(_board()), BRD + 8, None) == -5
    assert rewind(B(_board()), BRD + 8, None) == -5
    assert update(B(_board()), LOG + 8, BRD, None, None, None) == -5
    assert update(B(_board()), LOG, BRD + 8, None, None, None) == -5
    mf = _board(member_floats=1028)
    assert update(B(mf), LOG, BRD, W + 4, S, None) == -5
    assert update(B(mf), LOG, BRD, W, S + 8, None) == -5
    assert update(B(mf), LOG, BRD, W, None, None) == -5      # exactly one of weights / snapshot
    assert update(B(mf), LOG, BRD, None, S, None) == -5


def test_lib_loads_a_library_without_the_scoreboard(built_lib, tmp_path):
    """``SACENV_LIB`` may point at a build from before sacenv_scoreboard.h: ``_lib.load`` binds the
    new names only where they exist (a stand-in that exports sacenv.h's names alone)."""
    from sacenv import _lib
    src = tmp_path / "old.c"
    body = ["int sacenv_abi_version(void) { return %d; }" % _lib.ABI_VERSION]
    body += [f"int {n}(void) {{ return 0; }}" for n in _lib.EXPORTS if n != "sacenv_abi_version"]
    src.write_text("\n".join(body))
    so_path = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so_path)], check=True)
    lib = _lib.load(str(so_path))
    assert lib.sacenv_abi_version() == _lib.ABI_VERSION
    assert not any(hasattr(lib, n) for n in _lib.SCOREBOARD_EXPORTS)
