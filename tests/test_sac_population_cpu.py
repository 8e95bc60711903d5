"""The SAC population's C interface and draw rule without a GPU (include/sacenv_population.h,
sacenv/population.py).

* the library exports the four entry points beside the 49 of include/sacenv.h and outside
  ``_lib.EXPORTS`` (the ABI of sacenv.h does not move), and ``_lib.load`` still takes a library
  without them;
* ``SacenvSacMember`` and ``SacenvSacPopLayout`` have the layout of their ctypes mirrors;
* ``sacenv_sac_pop_layout`` follows its rounding rule against ``sacenv_sac_layout``;
* every argument error is found on the host, before anything is launched;
* ``sample_hpsets`` is the reference's draw rule (hyperparameter_tuner.py:20-43) on the ranges of
  configs/hp_configs.yaml (tests/golden/hp_configs.yaml is a copy of that file).
"""
import ctypes
import os
import random
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT

INCLUDE = os.path.join(ROOT, "include")
E_NULL, E_SIZE, E_RANGE = -1, -4, -5


def _params(obs_dim=11, batch=1024, **kw):
    from sacenv import _lib
    base = dict(obs_dim=obs_dim, n_actions=1, hidden=256, batch=batch, max_action=1.0, gamma=0.99, tau=0.005,
                reward_scale=10.0, lr_actor=0.005, lr_critic=0.0003, adam_beta1=0.9, adam_beta2=0.999,
                adam_eps=1e-8)
    base.update(kw)
    return _lib.SacParams(**base)


def test_library_exports_the_population_entry_points(built_lib):
    from sacenv import _lib
    assert _lib.POPULATION_EXPORTS == ("sacenv_sac_pop_layout", "sacenv_sac_pop_sync", "sacenv_sac_pop_act",
                                       "sacenv_sac_pop_learn")
    for n in _lib.POPULATION_EXPORTS:
        assert hasattr(built_lib, n), n
        assert n not in _lib.EXPORTS and n not in _lib.EPISODE_EXPORTS
    old = set(re.findall(r"\b(sacenv_\w+)\s*\(", open(os.path.join(INCLUDE, "sacenv.h")).read()))
    assert len(old) == 49 and old == set(_lib.EXPORTS)
    assert not old & set(_lib.POPULATION_EXPORTS)
    src = open(os.path.join(INCLUDE, "sacenv_population.h")).read()
    new = set(re.findall(r"\b(sacenv_\w+)\s*\(", src))
    assert new == set(_lib.POPULATION_EXPORTS)
    assert int(re.search(r"#define SACENV_POPULATION_VERSION (\d+)", src).group(1)) == _lib.POPULATION_VERSION == 1
    assert int(re.search(r"#define SACENV_SAC_POP_MAX_MEMBERS (\d+)", src).group(1)) == _lib.POPULATION_MAX_MEMBERS
    assert _lib.ABI_VERSION == 20 == built_lib.sacenv_abi_version()
    from sacenv import _build
    assert os.path.join("include", "sacenv_population.h") in [rel for rel, _ in _build.deps()]


def test_lib_loads_a_library_without_the_population_entry_points(built_lib, tmp_path):
    """``SACENV_LIB`` may point at a build from before sacenv_population.h (a stand-in that
    exports the names of sacenv.h alone)."""
    from sacenv import _lib
    src = tmp_path / "old.c"
    body = ["int sacenv_abi_version(void) { return %d; }" % _lib.ABI_VERSION]
    body += [f"int {n}(void) {{ return 0; }}" for n in _lib.EXPORTS if n != "sacenv_abi_version"]
    src.write_text("\n".join(body))
    so = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = _lib.load(str(so))
    assert lib.sacenv_abi_version() == _lib.ABI_VERSION
    assert not any(hasattr(lib, n) for n in _lib.POPULATION_EXPORTS)
    # what needs them says which header the library is older than; what the library has is handed out
    with pytest.raises(_lib.SacenvError, match=r"sacenv_population\.h"):
        _lib.require(_lib.POPULATION_EXPORTS, "sacenv_population.h", lib)
    with pytest.raises(_lib.SacenvError, match=r"sacenv_noise\.h"):
        _lib.require(("sacenv_sac_act",) + _lib.NOISE_EXPORTS, "sacenv_noise.h", lib)
    assert [f.__name__ for f in _lib.require(("sacenv_sac_act", "sacenv_sac_learn"), "sacenv.h", lib)] == \
        ["sacenv_sac_act", "sacenv_sac_learn"]
    assert [f.__name__ for f in _lib.require(_lib.POPULATION_EXPORTS, "sacenv_population.h")] == \
        list(_lib.POPULATION_EXPORTS)


def test_cuda_device_refuses_the_cpu_and_names_the_caller():
    import torch
    from sacenv import _lib
    assert issubclass(_lib.SacenvError, RuntimeError)
    for dev in ("cpu", torch.device("cpu")):
        with pytest.raises(_lib.SacenvError, match="X runs on a GPU"):
            _lib.cuda_device(dev, "X")
    assert _lib.cuda_device("cuda:1", "X") == torch.device("cuda", 1)      # an index given is kept, no device asked
    from sacenv.replay import _cuda_device
    assert _cuda_device is _lib.cuda_device


def test_population_structs_match_c_layout(tmp_path):
    """offsetof/sizeof of both structs, from gcc on the header, against the ctypes mirrors."""
    from sacenv import _lib
    pairs = (("SacenvSacMember", _lib.SacMember, 40), ("SacenvSacPopLayout", _lib.SacPopLayout, 40))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sacenv_population.h"', "int main(void) {"]
    for cname, py, _ in pairs:
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _t in py._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[0]: int(l.split()[1]) for l in out if l.strip()}
    for cname, py, size in pairs:
        assert got[cname] == ctypes.sizeof(py) == size, cname
        for fname, _t in py._fields_:
            assert got[f"{cname}.{fname}"] == getattr(py, fname).offset, (cname, fname)


@pytest.mark.parametrize("obs_dim,batch", [(11, 1024), (1, 256), (14, 768)])
def test_pop_layout_follows_the_single_agent_layout(built_lib, obs_dim, batch):
    from sacenv import _lib
    p = _params(obs_dim, batch)
    one = _lib.sac_layout(p)
    cap = _lib.POPULATION_MAX_MEMBERS
    for P in (1, 3, cap):
        L = _lib.SacPopLayout()
        assert built_lib.sacenv_sac_pop_layout(ctypes.byref(p), P, ctypes.byref(L)) == 0
        assert L.member_floats == (one.total_floats + 3) // 4 * 4
        assert L.scratch_bytes == (one.scratch_bytes + 15) // 16 * 16
        assert L.total_floats == P * L.member_floats
        assert L.total_scratch_bytes == P * L.scratch_bytes
        assert L.max_members == cap and L.pad == 0
        assert (4 * L.member_floats) % 16 == 0      # every member's slab is 16-B aligned in an aligned buffer
    L = _lib.SacPopLayout()
    for bad in (cap + 1, 0, -1):
        assert built_lib.sacenv_sac_pop_layout(ctypes.byref(p), bad, ctypes.byref(L)) == E_SIZE, bad
    assert built_lib.sacenv_sac_pop_layout(None, 1, ctypes.byref(L)) == E_NULL
    assert built_lib.sacenv_sac_pop_layout(ctypes.byref(p), 1, None) == E_NULL


BAD_PARAMS = (dict(hidden=128), dict(n_actions=2), dict(obs_dim=0), dict(obs_dim=15), dict(batch=0),
              dict(batch=255), dict(batch=384), dict(batch=(1 << 20) + 256))


def test_argument_errors_without_gpu(built_lib):
    """Every rule of the four entry points, none of which launches (there is no device here).
    Pointers are plain numbers with the alignment under test."""
    from sacenv import _lib
    lib, cap = built_lib, _lib.POPULATION_MAX_MEMBERS
    p, pp = _params(), ctypes.byref(_params())
    W, S, X = 1 << 20, 2 << 20, 3 << 20
    hp = (_lib.SacMember * cap)()
    L = _lib.SacPopLayout()

    # layout
    for bad in BAD_PARAMS:
        assert lib.sacenv_sac_pop_layout(ctypes.byref(_params(**bad)), 2, ctypes.byref(L)) == E_SIZE, bad

    # sync
    assert lib.sacenv_sac_pop_sync(None, 2, W, None) == E_NULL
    assert lib.sacenv_sac_pop_sync(pp, 2, None, None) == E_NULL
    for m in (0, -3, cap + 1):
        assert lib.sacenv_sac_pop_sync(pp, m, W, None) == E_SIZE, m
    assert lib.sacenv_sac_pop_sync(pp, 2, W + 4, None) == E_SIZE
    for bad in BAD_PARAMS:
        assert lib.sacenv_sac_pop_sync(ctypes.byref(_params(**bad)), 2, W, None) == E_SIZE, bad

    # act
    def act(p=pp, m=2, w=W, obs=X, n=64, eps=X, out=X, lp=X):
        return lib.sacenv_sac_pop_act(p, m, w, obs, n, eps, out, lp, None)

    assert act(p=None) == E_NULL
    for k in ("w", "obs", "eps", "out"):
        assert act(**{k: None}) == E_NULL, k
    for m in (0, -1, cap + 1):
        assert act(m=m) == E_SIZE, m
    assert act(n=-1) == E_SIZE
    assert act(w=W + 8) == E_SIZE
    for bad in BAD_PARAMS:
        want = 0 if "batch" in bad else E_SIZE      # the act entry point does not read the batch
        assert act(p=ctypes.byref(_params(**bad)), n=0) == want, bad
    assert act(n=0) == 0                            # no rows: OK, and nothing is launched
    assert act(n=0, w=None, obs=None, eps=None, out=None, lp=None) == 0
    assert act(n=0, m=cap + 1) == E_SIZE            # the members are checked before the rows

    # learn
    def learn(p=pp, m=2, hp=hp, w=W, scr=S, s=X, a=X, r=X, s2=X, d=X, e1=X, e2=X, step=1, losses=X):
        return lib.sacenv_sac_pop_learn(p, m, hp, w, scr, s, a, r, s2, d, e1, e2, step, losses, None)

    assert learn(p=None) == E_NULL
    for k in ("hp", "w", "scr", "s", "a", "r", "s2", "d", "e1", "e2"):
        assert learn(**{k: None}) == E_NULL, k
    for m in (0, -1, cap + 1):
        assert learn(m=m) == E_SIZE, m
    for bad in BAD_PARAMS:
        assert learn(p=ctypes.byref(_params(**bad))) == E_SIZE, bad
    assert learn(w=W + 4) == E_SIZE
    assert learn(scr=S + 8) == E_SIZE
    for step in (0, -1):
        assert learn(step=step) == E_RANGE, step
    assert p.batch == 1024    # (the params were only read)


def _golden_ranges():
    """The eight ``key: value`` lines of the agent section of hp_configs.yaml."""
    out = {}
    for line in open(os.path.join(GOLDEN, "hp_configs.yaml")):
        m = re.match(r"^\s+(\w+_(?:min|max)):\s*([0-9.eE+-]+)\s*$", line)
        if m:
            out[m.group(1)] = float(m.group(2))
    return out


def test_hp_ranges_are_the_reference_file():
    import dataclasses
    from sacenv.population import HPRanges
    want = _golden_ranges()
    assert len(want) == 8
    assert dataclasses.asdict(HPRanges()) == want


@pytest.mark.parametrize("seed", [0, 20240])
def test_sample_hpsets_is_the_reference_draw_rule(seed):
    import sacenv
    from sacenv.agent import AgentConfig
    from sacenv.population import HPRanges, sample_hpsets
    assert sacenv.sample_hpsets is sample_hpsets
    P, r = 5, _golden_ranges()
    got = sample_hpsets(P, seed)
    rng = random.Random(seed)
    base = AgentConfig()
    assert len(got) == P
    for cfg in got:
        want = [round(rng.uniform(r[k + "_min"], r[k + "_max"]), 4) for k in ("alpha", "beta", "gamma", "tau")]
        assert [cfg.lr_alpha, cfg.lr_beta, cfg.gamma, cfg.tau] == want
        for v, k in zip(want, ("alpha", "beta", "gamma", "tau")):
            assert r[k + "_min"] <= v <= r[k + "_max"], (k, v)
            assert round(v, 4) == v and len(repr(v).split(".")[1]) <= 4, (k, v)
        assert (cfg.batch_size, cfg.max_size, cfg.reward_scale) == (base.batch_size, base.max_size, base.reward_scale)
    assert len({(c.lr_alpha, c.lr_beta, c.gamma, c.tau) for c in got}) == P
    narrow = HPRanges(alpha_min=0.002, alpha_max=0.002)
    assert all(c.lr_alpha == 0.002 for c in sample_hpsets(3, seed, narrow))


def test_population_refuses_members_that_differ_in_a_shared_field():
    import dataclasses
    from sacenv.population import NativeSACPopulation, sample_hpsets
    cfgs = sample_hpsets(3, 1)
    for field, value in (("batch_size", 512), ("layer1_size", 128), ("max_size", 1000)):
        bad = list(cfgs)
        bad[1] = dataclasses.replace(bad[1], **{field: value})
        with pytest.raises(ValueError, match=field):
            NativeSACPopulation("cuda:0", bad, with_memory=False)
    with pytest.raises(ValueError):
        NativeSACPopulation("cuda:0", [], with_memory=False)
    with pytest.raises(ValueError, match="init_seeds"):
        NativeSACPopulation("cuda:0", cfgs, init_seeds=[1, 2], with_memory=False)
