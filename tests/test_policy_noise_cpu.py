"""The policy noise without a GPU (include/sacenv_noise.h, tests/noise_oracle.py).

* the library exports the header's one entry point beside the ABI of sacenv.h and outside the
  older export tuples, and ``_lib.load`` still takes a library without it;
* ``SacenvNoiseDraw`` has the layout of its ctypes mirror;
* every argument error is found on the host, before anything is launched;
* the contract itself, in its numpy restatement: within 1 f32 ulp of mpmath's exact values, the
  eleven statistics of noise_oracle.statistics within 5 sigma of N(0, 1)'s on the grid of seeds,
  streams and calls below (495 statistics: 5 sigma leaves a chance of about 3e-4 to a perfect
  generator, and the inputs are fixed), and the structure of the draws (prefix property;
  streams, calls and seeds apart).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import noise_oracle as no

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "sacenv_noise.h")
E_NULL, E_SIZE = -1, -4
NAMES = ("sacenv_noise_normal",)
SEEDS = (0, 1, 2, 2 ** 32 - 1, 2 ** 63 + 5)
STREAMS = (0, 1, 2)
CALLS = (0, 1, 2 ** 31)


def test_library_exports_the_noise_entry_point(built_lib):
    from sacenv import _build, _lib
    assert _lib.NOISE_EXPORTS == NAMES
    older = _lib.EXPORTS + _lib.EPISODE_EXPORTS + _lib.POPULATION_EXPORTS + _lib.REPLAY_POP_EXPORTS
    for n in NAMES:
        assert hasattr(built_lib, n), n
        assert n not in older
    src = open(HEADER).read()
    assert set(re.findall(r"\b(sacenv_\w+)\s*\(", src)) == set(NAMES)
    assert int(re.search(r"#define SACENV_NOISE_VERSION (\d+)", src).group(1)) == _lib.NOISE_VERSION == 1
    assert int(re.search(r"#define SACENV_NOISE_MAX_MEMBERS (\d+)", src).group(1)) == _lib.NOISE_MAX_MEMBERS == 64
    assert int(re.search(r"#define SACENV_NOISE_MAX_STREAMS (\d+)", src).group(1)) == _lib.NOISE_MAX_STREAMS == 4
    assert int(re.search(r"#define SACENV_NOISE_KEY1 (0x[0-9A-Fa-f]+)", src).group(1), 16) \
        == _lib.NOISE_KEY1 == no.KEY1 == int.from_bytes(b"noise", "big")
    for name, v in (("ACT", 0), ("LEARN1", 1), ("LEARN2", 2)):
        assert int(re.search(rf"#define SACENV_NOISE_{name} (\d+)", src).group(1)) == v \
            == getattr(_lib, "NOISE_" + name) == getattr(no, name)
    assert _lib.ABI_VERSION == 20 == built_lib.sacenv_abi_version()
    sacenv_h = open(os.path.join(INCLUDE, "sacenv.h")).read()
    assert int(re.search(r"#define SACENV_ABI_VERSION (\d+)", sacenv_h).group(1)) == 20
    rel = [r for r, _ in _build.deps()]
    assert os.path.join("include", "sacenv_noise.h") in rel
    assert os.path.join("sac-agent_amd", "csrc", "sacenv_noise.hip") in rel
    assert os.path.join("sac-agent_amd", "csrc", "sacenv_philox.h") in rel
    assert "sacenv_noise.hip" in _build.SOURCES and len(set(_build.SOURCES)) == len(_build.SOURCES)
    # one list: the library's units are the .hip files of csrc/, all of them and no other
    assert set(_build.SOURCES) == {f for f in os.listdir(_build.CSRC) if f.endswith(".hip")}
    assert "sacenv_philox.h" in _build.HEADERS
    # one copy of the generator: the replay unit and the noise unit include the shared header
    for f in ("sacenv_replay.hip", "sacenv_noise.hip"):
        text = open(os.path.join(_build.CSRC, f)).read()
        assert '#include "sacenv_philox.h"' in text and "void philox4x64_10" not in text, f


def test_lib_loads_a_library_without_the_noise_entry_point(built_lib, tmp_path):
    """``SACENV_LIB`` may point at a build from before sacenv_noise.h (a stand-in that exports
    every older name and not the new one)."""
    from sacenv import _lib
    src = tmp_path / "old.c"
    body = ["int sacenv_abi_version(void) { return %d; }" % _lib.ABI_VERSION]
    older = _lib.EXPORTS + _lib.EPISODE_EXPORTS + _lib.POPULATION_EXPORTS + _lib.REPLAY_POP_EXPORTS
    body += [f"int {n}(void) {{ return 0; }}" for n in older if n != "sacenv_abi_version"]
    src.write_text("\n".join(body))
    so = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = _lib.load(str(so))
    assert lib.sacenv_abi_version() == _lib.ABI_VERSION
    assert not any(hasattr(lib, n) for n in NAMES)
    assert all(hasattr(lib, n) for n in _lib.REPLAY_POP_EXPORTS)


def test_noise_draw_struct_matches_c_layout(tmp_path):
    """offsetof/sizeof from gcc on the header against the ctypes mirror."""
    from sacenv import _lib
    cname, py = "SacenvNoiseDraw", _lib.NoiseDraw
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sacenv_noise.h"', "int main(void) {",
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
    assert got[cname] == ctypes.sizeof(py) == 32
    assert [f for f, _ in py._fields_] == ["stream", "first_call", "calls", "n", "out"]
    for fname, _t in py._fields_:
        assert got[fname] == getattr(py, fname).offset, fname


def test_argument_errors_without_gpu(built_lib):
    """Every rule of sacenv_noise_normal; none launches (there is no device here). The output
    pointers are plain numbers with the alignment under test."""
    from sacenv import _lib
    lib, cap = built_lib, 64
    X = 3 << 20
    seeds = (ctypes.c_uint64 * cap)()

    def call(members=2, sd=seeds, n_draws=None, draws=((0, 0, 1, 8, X),)):
        arr = None
        if draws is not None:
            arr = (_lib.NoiseDraw * max(len(draws), 1))()
            for d, (stream, first, calls, n, out) in zip(arr, draws):
                d.stream, d.first_call, d.calls, d.n, d.out = stream, first, calls, n, out
        nd = len(draws) if n_draws is None else n_draws
        return lib.sacenv_noise_normal(members, sd, nd, arr, None)

    one = (0, 0, 1, 8, X)
    for m in (0, -1, cap + 1):
        assert call(members=m) == E_SIZE, m
    for nd in (0, -1, 5):
        assert call(n_draws=nd, draws=(one,) * 5) == E_SIZE, nd
    assert call(sd=None) == E_NULL
    assert call(draws=None, n_draws=1) == E_NULL
    assert call(members=cap + 1, sd=None) == E_SIZE          # the counts are checked before the pointers
    for calls in (0, -1):
        assert call(draws=((0, 0, calls, 8, X),)) == E_SIZE, calls
    assert call(draws=((0, 0, 1, -1, X),)) == E_SIZE
    assert call(draws=((0, 0, 1, 8, None),)) == E_NULL
    for off in (1, 2, 3):
        assert call(draws=((0, 0, 1, 8, X + off),)) == E_SIZE, off
    # calls x members x n >= 2^31
    assert call(members=2, draws=((0, 0, 1, 1 << 30, X),)) == E_SIZE
    assert call(members=64, draws=((0, 0, 1 << 15, 1 << 10, X),)) == E_SIZE
    assert call(members=1, draws=((0, 0, (1 << 31) - 1, 2, X),)) == E_SIZE
    # an error in a later draw is found before the earlier ones launch
    assert call(draws=(one, one, (2, 5, 0, 8, X))) == E_SIZE
    assert call(draws=(one, (1, 0, 1, 8, None))) == E_NULL
    assert call(draws=(one, one, one, (1, 0, 1, 8, X + 2))) == E_SIZE
    # nothing to draw: OK without a launch, whatever `out` is
    assert call(draws=((0, 0, 1, 0, None),)) == 0
    assert call(draws=((0, 0, 3, 0, None), (7, 1 << 40, 1, 0, X + 1))) == 0
    assert call(draws=((0, 0, 0, 0, None),)) == E_SIZE       # calls < 1 even with n == 0
    assert call(members=cap + 1, draws=((0, 0, 1, 0, None),)) == E_SIZE


def test_python_side_without_a_device(built_lib):
    import sacenv
    from sacenv.noise import ACT, LEARN1, LEARN2, PolicyNoise
    assert sacenv.PolicyNoise is PolicyNoise and "PolicyNoise" in sacenv.__all__
    assert (ACT, LEARN1, LEARN2) == (0, 1, 2) == (PolicyNoise.ACT, PolicyNoise.LEARN1, PolicyNoise.LEARN2)
    with pytest.raises(RuntimeError, match="GPU"):
        PolicyNoise([1, 2], device="cpu")
    for bad in ([], list(range(65)), [-1], [2 ** 64], [1.5]):
        with pytest.raises(ValueError):
            PolicyNoise(bad, device="cuda")


@pytest.fixture(scope="module")
def exact():
    """4 096 values in mpmath, over seeds, streams and calls (computed once)."""
    rows = [(s, st, c, 256) for s in (0, 1, 2 ** 32 - 1, 2 ** 63 + 5)
            for st, c in ((0, 0), (1, 2 ** 31), (2, 1), (0, 2 ** 40))]
    assert sum(r[3] for r in rows) == 4096
    return [(r, no.normal_mp(*r)) for r in rows]


def test_numpy_restatement_against_mpmath(exact):
    worst = differing = 0
    for row, want in exact:
        got = no.normal_np(*row)
        d = no.ulp_distance(got, want)
        worst, differing = max(worst, int(d.max())), differing + int((d != 0).sum())
        assert np.isfinite(got).all() and np.abs(got).max() < no.BOUND
        assert not got[want == 0].any()
    print(f"numpy vs mpmath on 4096 values: worst {worst} f32 ulp, {differing} not bit-equal")
    assert worst <= 1


def test_uniforms_are_exact_and_bounded():
    """u1 in (0, 1], u2 in [0, 1) at the words' extremes, and the bound on |z|."""
    top = np.uint64(2 ** 64 - 1)
    assert float(((top >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53) == 1.0
    assert float((top >> np.uint64(11)).astype(np.float64) * 2.0 ** -53) == 1.0 - 2.0 ** -53
    assert float((np.uint64(0) >> np.uint64(11)) + np.uint64(1)) * 2.0 ** -53 == 2.0 ** -53
    assert np.sqrt(-2.0 * np.log(2.0 ** -53)) == pytest.approx(np.sqrt(106 * np.log(2.0))) and \
        np.sqrt(106 * np.log(2.0)) < no.BOUND


@pytest.mark.parametrize("seed", SEEDS)
def test_statistics_within_five_sigma(seed):
    worst = ("", 0.0)
    for stream in STREAMS:
        for call in CALLS:
            x = no.normal_np(seed, stream, call, 1 << 20)
            assert np.isfinite(x).all() and np.abs(x).max() < no.BOUND
            for name, v in no.statistics(x).items():
                if abs(v) > abs(worst[1]):
                    worst = (f"{name} (stream {stream}, call {call})", v)
                assert abs(v) <= 5.0, (seed, stream, call, name, v)
    print(f"seed {seed}: worst {worst[1]:+.2f} sigma, {worst[0]}")


def test_structure_of_the_draws():
    base = no.normal_np(2, 0, 1, 200)
    assert np.array_equal(no.normal_np(2, 0, 1, 63), base[:63])          # prefix property
    n = 4096
    rows = {"stream 1": no.normal_np(2, 1, 1, n), "stream 2": no.normal_np(2, 2, 1, n),
            "call 2": no.normal_np(2, 0, 2, n), "call 0": no.normal_np(2, 0, 0, n),
            "seed 3": no.normal_np(3, 0, 1, n), "seed 1": no.normal_np(1, 0, 1, n)}
    ref = no.normal_np(2, 0, 1, n)
    names = list(rows)
    for k, a in enumerate(names):
        assert not np.array_equal(rows[a], ref), a
        assert abs(np.corrcoef(rows[a], ref)[0, 1]) < 0.08, a        # 5 / sqrt(4096)
        for b in names[k + 1:]:
            assert abs(np.corrcoef(rows[a], rows[b])[0, 1]) < 0.08, (a, b)
    # the replay sampler's blocks (key (seed, 0)) are other blocks
    from ctr_sampler import philox4x64_10
    ctr = np.zeros((4, 4), np.uint64)
    ctr[:, 0] = np.arange(4, dtype=np.uint64)
    ctr[:, 1] = np.uint64(1)
    assert not np.array_equal(philox4x64_10(ctr, 2, 0), no.words(2, 0, 1, 16))
