"""Pins the float64 SAC oracle (oracle/sac_f64.py) to VecSAC on the CPU.

tests/test_agent_cpu.py pins ``VecSAC`` to the reference agent's recorded learn() calls; here
the oracle is held to ``VecSAC("cpu")`` on the batches the GPU module uses
(oracle/sac_f64_cases.py), per element and in the same unit:

* gradients: after ``learn()`` every optimised net's ``.grad`` is exactly its own loss's
  gradient (the ``zero_grad`` order), and ``|grad - g_f64| <= c 2^-24 S_max(tensor)``; where
  ``S == 0`` (dead ReLU units) both are exactly 0;
* ``policy_f64`` against ``Actor.sample_normal`` in float32, in the action / log-prob units;
* the kink filter: what it keeps and rejects, and its 25 % cap; the second step's |x| limit;
* the constants of oracle/sac_f64_cases.py are 4x what profiles/r10_sac_f64_margins.json
  recorded for torch (tools/sac_f64_margins.py writes that file).

c is 4x torch's own worst (c_ref 10.07 -> 40.3), so torch passes with that margin on any host;
the filter rejected 14.6 % (obs_dim 11), 15.5 % (14) and 10.2 % (1) of the candidate rows
(9.4 % with tied critics, 12.7 % at the second step, whose |x| limit rejects 62.2 % besides).
"""
import json
import os

import pytest
import torch

import sac_f64_cases as K
from conftest import ROOT
from sac_f64 import kink_free_rows, learn_f64

PROFILE = os.path.join(ROOT, "profiles", "r10_sac_f64_margins.json")


@pytest.fixture(scope="module")
def reference():
    out = {}
    for name in K.CASES:
        out.update(K.torch_reference(name))
    return out


@pytest.mark.parametrize("name", list(K.CASES) + [K.STEP2_NAME])
def test_oracle_gradients_match_vecsac_per_element(reference, name):
    fig = reference[name]
    print(name, fig["c_ref"])
    assert fig["dead_elements"] > 0 and fig["dead_nonzero"] == 0   # the exact-zero check has elements to bite on
    bad = {k: v for k, v in fig["c_ref"].items() if not v <= K.C_GRAD}
    assert not bad, bad


@pytest.mark.parametrize("name", list(K.CASES) + [K.STEP2_NAME])
def test_row_filter_stays_under_its_cap(reference, name):
    assert 0.0 < reference[name]["rejected_share"] <= K.MAX_REJECT


@pytest.mark.parametrize("name", list(K.CASES) + [K.STEP2_NAME])
def test_adam_restatement_matches_torch_step(reference, name):
    for which in ("adam_ulps_own_grad", "adam_ulps_read_back"):
        bad = {q: u for q, u in reference[name][which].items() if not u <= K.ADAM_ULPS[q]}
        assert not bad, (which, bad)


def test_policy_f64_matches_sample_normal():
    act = K.torch_act_reference()
    print(act)
    assert act["c_a_ref"] <= K.C_ACT and act["c_l_ref"] <= K.C_LOGP


def _agent(name):
    from sacenv.agent import VecSAC
    case = K.CASES[name]
    return case, VecSAC("cpu", K.agent_config(case), obs_dim=case["obs_dim"], max_action=case["max_action"],
                        init_seed=case["seed"], with_memory=False)


def test_row_filter_keeps_exactly_the_rows_with_margin():
    case, agent = _agent("d11_m1_b256")
    sd = K.cpu_state_dicts(agent)
    s, a, r, s2, e1, e2 = K.candidate_pool(11, 384, 5)
    d = torch.zeros(384, dtype=torch.bool)
    args = (sd, (s, a, r, s2, d), (e1, e2), K.case_cfg(case), 1.0)
    f = learn_f64(*args, grads=False)
    keep, share = kink_free_rows(*args, K.DELTA_Z, K.DELTA_Q)
    ok = (f["min_abs_z"] >= K.DELTA_Z) & (f["dq_sample"] >= K.DELTA_Q) & (f["dq_rsample"] >= K.DELTA_Q)
    assert torch.equal(keep, torch.nonzero(ok).view(-1))
    assert share == pytest.approx(1 - keep.numel() / 384)
    # per-row: a row's verdict does not depend on the rows around it
    sub = keep[:100]
    keep2, share2 = kink_free_rows(sd, (s[sub], a[sub], r[sub], s2[sub], d[sub]), (e1[sub], e2[sub]),
                                   K.case_cfg(case), 1.0, K.DELTA_Z, K.DELTA_Q)
    assert keep2.numel() == 100 and share2 == 0.0
    # without the min margin no fewer rows pass; a huge margin rejects all
    keep3, _ = kink_free_rows(*args, K.DELTA_Z, None)
    assert set(keep.tolist()) <= set(keep3.tolist())
    assert kink_free_rows(*args, 1e3, K.DELTA_Q)[0].numel() == 0


def test_select_batch_enforces_the_cap(monkeypatch):
    case, agent = _agent("d11_m1_b256")
    monkeypatch.setattr(K, "DELTA_Z", 1e-2)   # rejects far more than a quarter of the rows
    with pytest.raises(AssertionError, match="rejected"):
        K.select_batch(K.cpu_state_dicts(agent), case, case["seed"])


def test_done_pattern_covers_every_block():
    for rows in (256, 512, 768):
        d = K.done_pattern(rows, 3).view(-1, 16)
        assert bool(d.any(1).all()) and bool((~d).any(1).all())
        assert 0.05 <= float(d.float().mean()) <= 0.15


def test_dead_units_have_zero_scale_and_zero_gradient():
    """A unit whose bias keeps it off for every row: S == 0 and the gradient is exactly 0, in
    the oracle and in VecSAC."""
    case, agent = _agent("d11_m1_b256")
    with torch.no_grad():
        for net in (agent.actor, agent.critic_1, agent.value):
            net.fc1.bias[3] = -100.0
            net.fc2.bias[200] = -100.0
    sd = K.cpu_state_dicts(agent)
    batch, noise, _ = K.select_batch(sd, case, case["seed"])
    f = learn_f64(sd, batch, noise, K.case_cfg(case), 1.0)
    agent.learn(batch, noise)
    for n, head in (("actor", "mean"), ("critic_1", "q"), ("value", "v")):
        net = getattr(agent, n)
        for k, idx in (("fc1.weight", 3), ("fc1.bias", 3), ("fc2.weight", 200), ("fc2.bias", 200)):
            assert float(f["S"][n][k][idx].abs().max()) == 0.0, (n, k)
            assert float(f["grad"][n][k][idx].abs().max()) == 0.0, (n, k)
            assert float(dict(net.named_parameters())[k].grad[idx].abs().max()) == 0.0, (n, k)
        assert float(f["S"][n]["fc2.weight"][:, 3].max()) == 0.0          # nothing flows from a dead input
        assert float(f["S"][n][f"{head}.weight"][0, 200]) == 0.0
        assert float(f["S"][n]["fc2.weight"].max()) > 0.0
    # S bounds |g| everywhere (a sum is at most the sum of the absolute values)
    for n in K.OPTIMISED:
        for k, g in f["grad"][n].items():
            assert bool((g.abs() <= f["S"][n][k] * (1 + 1e-12)).all()), (n, k)


def test_second_step_rows_stay_out_of_saturation():
    """The second step's rows: |x| <= X_LIMIT at both draws, kink-free, and both rejected shares
    reported apart (the kink filter's cap is on its own share of the whole pool)."""
    case, agent = _agent(K.STEP2)
    agent.learn(*K.step_batch(K.cpu_state_dicts(agent), case, 1)[:2])
    sd = K.cpu_state_dicts(agent)
    batch, noise, shares = K.step_batch(sd, case, 2)
    f = learn_f64(sd, batch, noise, K.case_cfg(case), case["max_action"], grads=False)
    assert float(f["abs_x_sample"].max()) <= K.X_LIMIT and float(f["abs_x_rsample"].max()) <= K.X_LIMIT
    assert float(f["min_abs_z"].min()) >= K.DELTA_Z
    assert float(torch.minimum(f["dq_sample"], f["dq_rsample"]).min()) >= K.DELTA_Q
    assert 0.0 < shares["kink"] <= K.MAX_REJECT and 0.0 < shares["saturated"] < 1.0
    # without the limit the same weights give rows far into saturation (why the limit is there)
    wide = K.select_batch(sd, case, case["seed"] + 100, K.DELTA_Q)
    g = learn_f64(sd, wide[0], wide[1], K.case_cfg(case), case["max_action"], grads=False)
    assert float(g["abs_x_rsample"].max()) > 8.0 and wide[2]["saturated"] == 0.0


@pytest.mark.parametrize("name,step", [("d11_m1_b256", 1), ("d14_m05_b768", 1), ("d11_m1_b256", 2)])
def test_bar_notices_one_dropped_row(name, step):
    """The bar has teeth, at the second step too: a reduction that leaves one batch row out moves
    the weight tensors by far more than c units (the oracle's own figures, no kernel involved).
    Printed beside it: the same change under the norm-relative bar of test_sac_native_gpu.py
    (1e-3 of the norm)."""
    case, agent = _agent(name)
    if step == 2:
        agent.learn(*K.step_batch(K.cpu_state_dicts(agent), case, 1)[:2])
    sd = K.cpu_state_dicts(agent)
    batch, noise, _ = K.step_batch(sd, case, step)
    cfg, M, B = K.case_cfg(case), case["max_action"], case["batch"]
    f = learn_f64(sd, batch, noise, cfg, M)
    for r in (0, B // 2 + 5, B - 1):
        one = learn_f64(sd, tuple(t[r:r + 1] for t in batch), tuple(t[r:r + 1] for t in noise), cfg, M)
        units = K.dropped_row_units(f, one, B)
        rel = {f"{n}.{k}": float((g / B).norm() / f["grad"][n][k].norm()) for n in K.OPTIMISED
               for k, g in one["grad"][n].items()}
        print(f"{name} step {step} row {r}: {min(units.values()):.0f} .. {max(units.values()):.0f} units (bar {K.C_GRAD}); "
              f"norm-relative {min(rel.values()):.1e} .. {max(rel.values()):.1e} (bar 1e-3)")
        for k, v in units.items():
            if k.endswith("fc2.weight") or k.endswith("fc1.weight"):
                assert v > 10 * K.C_GRAD, (k, v)
        assert max(units.values()) > 100 * K.C_GRAD


def test_dead_moment_check_reads_an_exact_zero():
    """dead_nonzero_from_moments on non-zero moments: a zero gradient passes, one ulp does not."""
    import numpy as np
    f = {"S": {n: {} for n in K.OPTIMISED}}
    f["S"]["actor"]["fc1.bias"] = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    m0 = {"actor": {"fc1.bias": np.array([0.3, -1e-5, 0.7], np.float32)}}
    lw = np.float32(K.LERP_W)
    m1 = {"actor": {"fc1.bias": m0["actor"]["fc1.bias"] + lw * (np.float32(0) - m0["actor"]["fc1.bias"])}}
    assert K.dead_nonzero_from_moments(m1, m0, f) == 0
    m1["actor"]["fc1.bias"][2] += 1.0     # a live element may move
    assert K.dead_nonzero_from_moments(m1, m0, f) == 0
    m1["actor"]["fc1.bias"][1] = np.nextafter(m1["actor"]["fc1.bias"][1], np.float32(1))
    assert K.dead_nonzero_from_moments(m1, m0, f) == 1


def test_tie_case_splits_min_in_half():
    """critic_2 == critic_1: every row ties, and the oracle's actor gradient is the one of
    -q1 alone (half through each critic), as torch.min's backward gives it."""
    case, agent = _agent("d11_m1_b256_tie")
    K.tie_critics(agent)
    sd = K.cpu_state_dicts(agent)
    batch, noise, _ = K.select_batch(sd, case, case["seed"], None)
    f = learn_f64(sd, batch, noise, K.case_cfg(case), 1.0)
    assert float(f["dq_rsample"].max()) == 0.0 and float(f["dq_sample"].max()) == 0.0
    for k in f["grad"]["critic_1"]:
        assert torch.equal(f["grad"]["critic_1"][k], f["grad"]["critic_2"][k])
    sd["critic_2"]["q.bias"] = sd["critic_2"]["q.bias"] + 10.0     # q2 = q1 + 10: min is q1 on every row
    f1 = learn_f64(sd, batch, noise, K.case_cfg(case), 1.0)
    for k, g in f["grad"]["actor"].items():
        assert float((g - f1["grad"]["actor"][k]).abs().max()) <= 1e-12 * f["S_max"]["actor"][k], k


def test_constants_are_four_times_the_recorded_reference():
    with open(PROFILE) as fh:
        ref = json.load(fh)["reference"]
    for const, key in ((K.C_GRAD, "c"), (K.C_ACT, "c_a"), (K.C_LOGP, "c_l")):
        assert ref[key] <= const <= 1.01 * ref[key], key
    assert ref["adam_ulps_bound"] == K.ADAM_ULPS
    assert ref["delta_z"] == K.DELTA_Z == 1e-5 and ref["delta_q"] == K.DELTA_Q == 1e-5
    assert ref["x_limit_step2"] == K.X_LIMIT
    assert set(ref["cases"]) == set(K.CASES) | {K.STEP2_NAME}
    assert all(c["rejected_share"] <= K.MAX_REJECT for c in ref["cases"].values())
