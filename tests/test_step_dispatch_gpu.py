"""Every non-dense entry of the multi-step launch's kernel table, once.

``sacenv_boat_segment`` and ``sacenv_boat_rollout`` pick one ``k_rollout``
instantiation per launch from (wind curves 0/1/2) x (t from the index / carried)
x (rows: none, pooled, staged, a fresh record per step) x (lean / general), and
``sacenv_boat_segment_occupancy`` reports the resources of the same pick. Each
entry must equal the same number of ``sacenv_boat_step`` launches bit for bit
(the per-step kernel is pinned to the reference by tests/test_gpu_parity.py):
this tests the wiring of the table, not new behaviour.

Shape: 130 envs (two full owner waves and a padded one), 40 steps in one
launch, 13-step episodes, every 7th env's actions scaled by 12 so rudders
break: every wave sees truncations, early terminations, restarts and quiet
steps. Experiments 1, 4, 6 (0, 1, 2 curves) x dt 0.25 (t from the index) and
0.1 (carried t) x the four kinds of rows x no options (lean where it exists)
and record_reward64 (general): 48 cases. The dense entries (more owner waves
than SIMDs) stay with test_segment_gpu.py::test_dense_segment_equals_steps.
Reference: environment/boat_env.py:67-126.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

N, K, EPISODE = 130, 40, 13
STATE = ("s_x", "s_y", "s_r", "v_x", "v_y", "v_r", "rudder", "ep_reward", "t", "index")
RECORD = ("obs", "reward", "done", "term")
COUNTS = ("counters", "cons", "last_term")
WITH_TRANS = {"plain": 0, "trans": 1, "stage": 2, "rollout": 0}


def _env(gpu, exp, dt, opt):
    from sacenv import VecBoatEnv
    base = {"experiment": exp, "test_mode": 0}
    if dt != 0.25:
        base.update(dt=dt, t_max=20.0)
    return VecBoatEnv({"base_settings": base}, N, seed=5, device=gpu, max_episode_steps=EPISODE,
                      n_helpers=64, auto_refill=False, record_reward64=opt == "reward64")


@pytest.fixture(scope="module")
def actions(gpu):
    g = torch.Generator(device=gpu)
    g.manual_seed(N)
    t = torch.rand((K, N), generator=g, device=gpu) * 2 - 1
    t[:, ::7] *= 12.0
    return t


@pytest.fixture(scope="module")
def reference(gpu, actions):
    """Per (exp, dt, opt), computed once and left unchanged: an env after K step_async
    launches, and one after K step_pooled_async launches with every step's pooled row,
    record and terminal obs."""
    from sacenv import _lib
    cache = {}

    def get(exp, dt, opt):
        key = (exp, dt, opt)
        if key not in cache:
            stepped, pooled = _env(gpu, exp, dt, opt), _env(gpu, exp, dt, opt)
            rows = torch.zeros((K, _lib.trans_bytes(exp) * pooled.n_pad), dtype=torch.uint8, device=gpu)
            records = torch.zeros((K, pooled.record.numel()), dtype=torch.uint8, device=gpu)
            finals = torch.zeros((K, N, _lib.OBS_DIM), dtype=torch.float32, device=gpu)
            for k in range(K):
                stepped.step_async(actions[k])
                pooled.step_pooled_async(actions[k], rows[k])
                records[k].copy_(pooled.record)
                finals[k].copy_(pooled.final_obs)
            torch.cuda.synchronize()
            cache[key] = (stepped, pooled, rows, records, finals)
        return cache[key]

    return get


def _same(a, b, names, where):
    for name in names:
        assert torch.equal(getattr(a, name), getattr(b, name)), f"{name} differs ({where})"


@pytest.mark.parametrize("opt", ["none", "reward64"])
@pytest.mark.parametrize("rows", ["plain", "trans", "stage", "rollout"])
@pytest.mark.parametrize("dt", [0.25, 0.1])
@pytest.mark.parametrize("exp", [1, 4, 6])
def test_table_entry_equals_steps(exp, dt, rows, opt, gpu, built_lib, actions, reference):
    from sacenv import _lib
    from sacenv.dist import TransitionLayout
    stepped, pooled, ref_rows, ref_records, ref_finals = reference(exp, dt, opt)
    env = _env(gpu, exp, dt, opt)
    NP = env.n_pad
    where = f"exp {exp}, dt {dt}, {rows}, {opt}"
    carried = STATE + ("final_ep_reward",) + COUNTS + (("reward64",) if opt == "reward64" else ())
    if rows == "plain":
        env.segment_async(actions, K)
        torch.cuda.synchronize()
        _same(env, stepped, carried + RECORD + ("final_obs",), where)
    elif rows == "trans":
        got = torch.zeros_like(ref_rows)
        env.segment_async(actions, K, trans=got.view(-1), trans_stride=got.shape[1])
        torch.cuda.synchronize()
        _same(env, pooled, carried + RECORD + ("final_obs",), where)
        for k in range(K):
            assert torch.equal(got[k], ref_rows[k]), f"pooled row {k} ({where})"
    elif rows == "stage":
        stage = torch.zeros(NP * K * 64, dtype=torch.uint8, device=gpu)
        env.segment_async(actions, K, stage=stage)
        torch.cuda.synchronize()
        _same(env, pooled, carried + RECORD + ("final_obs",), where)
        words = stage.view(torch.float32).view(NP, K, 16)[:N]
        codes = stage.view(NP, K, 64)[:N, :, 4 * 13]      # term: the low byte of word 13
        lay = TransitionLayout(N, NP, exp)
        for k in range(K):
            s_next, reward, action, term, _ = lay.views(ref_rows[k])
            assert torch.equal(words[:, k, :_lib.OBS_DIM], s_next), f"staged row {k}: s' ({where})"
            assert torch.equal(words[:, k, 11], reward), f"staged row {k}: reward ({where})"
            assert torch.equal(words[:, k, 12], action), f"staged row {k}: action ({where})"
            assert torch.equal(codes[:, k], term), f"staged row {k}: term ({where})"
    else:
        fin = torch.zeros((K, NP, _lib.OBS_DIM), dtype=torch.float32, device=gpu)
        records, _ = env.rollout(actions, final_obs=fin)
        torch.cuda.synchronize()
        _same(env, pooled, carried, where)       # (a rollout leaves the env's own record alone)
        for k in range(K):
            got, want = env.record_views(records[k]), pooled.record_views(ref_records[k])
            for name, x, y in zip(RECORD, got, want):
                assert torch.equal(x, y), f"record {k}: {name} ({where})"
            ended = want[2] != 0
            assert torch.equal(fin[k, :N][ended], ref_finals[k][ended]), f"terminal obs of step {k} ({where})"
        for name, x, y in zip(RECORD, env.record_views(records[K - 1]), pooled.record_views(pooled.record)):
            assert torch.equal(x, y), f"last record: {name} ({where})"
    env.check_status()
    assert int(stepped.counters.sum()) > 0 and int(stepped.cons.min()) >= K // EPISODE
    # the resources reported are those of a kernel of the same table
    out = [ctypes.c_int32() for _ in range(4)]
    rc = built_lib.sacenv_boat_segment_occupancy(ctypes.byref(env.params), WITH_TRANS[rows],
                                                 *[ctypes.byref(o) for o in out])
    per_cu, grid, vgprs, lds_bytes = (o.value for o in out)
    assert rc == 0
    assert grid == 3 and 0 < vgprs <= 512 and lds_bytes > 0, (per_cu, grid, vgprs, lds_bytes)
