"""The persistent segment launch's lean instantiation, and the dispatch that picks it.

``sacenv_boat_segment`` runs its open loop with the launch's options compiled
in (no optional outputs, autoreset on, experiment != 2, fuel != 0: the "lean"
instantiation) exactly when the launch's parameters allow it, and the general
loop otherwise. Either way the launch must equal the same number of
``sacenv_boat_step`` launches bit for bit (the per-step kernel is pinned to
the reference by tests/test_gpu_parity.py).

Shapes: 192 envs (three owner waves) and 130 (a padded last wave); 300 steps
as a 256-step segment, its refill, and a 44-step short launch; 37-step
episodes and some rudders that break at once, so every wave sees truncations,
early terminations, restarts, and steps in which none of its lanes ends.
Experiments: 6 (two wind curves, lean), 1 (no curve, lean), 2 (never lean).
Options: none (lean where the experiment allows), the reward64 + accel
outputs (general), autoreset off (general).
Reference: environment/boat_env.py:67-126.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 300
STATE = ("s_x", "s_y", "s_r", "v_x", "v_y", "v_r", "rudder", "ep_reward", "t", "index")
OUTPUTS = ("obs", "reward", "done", "term", "final_obs", "final_ep_reward")


@pytest.fixture(scope="module")
def action_tables(gpu):
    """One [300, N] action table per env count, shared by every case (read only)."""
    out = {}
    for N in (192, 130):
        g = torch.Generator(device=gpu)
        g.manual_seed(N)
        t = torch.rand((STEPS, N), generator=g, device=gpu) * 2 - 1
        t[:, ::7] *= 12.0          # some rudders break at once: early terminations
        out[N] = t
    return out


def _assert_same(a, b, names, where):
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x, y), f"{name} differs {where}"


@pytest.mark.parametrize("variant", ["plain", "outputs", "no_autoreset"])
@pytest.mark.parametrize("exp", [6, 1, 2])
@pytest.mark.parametrize("N", [192, 130])
def test_segment_equals_steps_by_option(N, exp, variant, gpu, built_lib, action_tables):
    from sacenv import VecBoatEnv, _lib
    assert _lib.REFILL_PERIOD == 256
    cfg = {"base_settings": {"experiment": exp, "test_mode": 0}}
    kw = dict(seed=5, device=gpu, max_episode_steps=37, n_helpers=64, auto_refill=False,
              autoreset=variant != "no_autoreset",
              record_accel=variant == "outputs", record_reward64=variant == "outputs")
    seg, ref = VecBoatEnv(cfg, N, **kw), VecBoatEnv(cfg, N, **kw)
    table = action_tables[N]
    names = STATE + OUTPUTS + ("counters", "cons", "last_term")
    if variant == "outputs":
        names += ("accel", "reward64")
    k = 0
    for K in (256, STEPS - 256):
        rows = table[k: k + K]
        seg.segment_async(rows, K)
        for j in range(K):
            ref.step_async(rows[j])
        if kw["autoreset"]:
            seg.refill()
            ref.refill()
        k += K
        torch.cuda.synchronize()
        _assert_same(seg, ref, names, f"after step {k} (N={N}, exp {exp}, {variant})")
    seg.check_status()
    ref.check_status()
    # the run exercised what it claims to: episodes ended by truncation and by the
    # termination chain, and (autoreset) envs restarted
    assert int(ref.counters.sum()) > 0
    if kw["autoreset"]:
        assert int(ref.cons.min()) >= STEPS // 37
