"""sacenv_sac.hip element by element against the float64 oracle (oracle/sac_f64.py).

What is compared, and in which unit (oracle/sac_f64_cases.py has the code):

* **Gradients, per element.** A fresh NativeSAC has zero Adam moments, so after its first
  learn() ``exp_avg == lerp_w * g`` with ``lerp_w = float32(1 - 0.9)`` and
  ``g = exp_avg / lerp_w`` reads every element of every gradient to one ulp, with Adam at its
  defaults. The second step reads ``g2 = m1 + (m2 - m1) / lerp_w``. The bar is
  ``|g - g_f64| <= c 2^-24 S_max(tensor)``, S being the abs-sum of the element's per-row
  contributions (``|grad_out|^T |layer_in|``), and exactly 0 where S == 0 (dead ReLU units).
  One dropped batch row at B = 768 moves an element by ~1e-3 S, hundreds of times the bar.
* **Losses** in the same unit, the scale being the mean |per-row term|.
* **Adam, per element**: torch.optim.Adam's foreach form restated in numpy float32 from the
  kernel's own g; exp_avg_sq, the parameter and the soft-updated target within a few ulps.
* **Kernel copies**: after learn(), choose_action and a further learn() agree bit for bit with
  an agent rebuilt from state_dicts() + sync() (a stale w2f / w2tf / target copy would show).
* **sacenv_sac_act with a log_prob buffer** per row: action within
  ``c_a 2^-24 max_action (1 + |x|)``, log_prob within
  ``c_l 2^-24 (1 + |lp| + 2 / (1 - a^2 + 1e-6))`` (the last term is the float32 conditioning of
  the reference's own log(1 - a^2 + 1e-6) at saturation).

Batches are kink-free rows (every fc1 / fc2 pre-activation at least 1e-5 from zero, |q1 - q2|
at least 1e-5 at both draws; the filter may reject at most 25 % of a candidate pool), so all
implementations take the same ReLU masks and min branches and float32 rounding theory applies.
The second step's rows are also kept out of tanh saturation, |x| <= 3 at both draws (after one
default Adam step sigma is 2..5.6; where tanh rounds to +-1 no float32 implementation follows
float64, torch is 51 822 units off on unfiltered rows). The limit comes from the conditioning
of log(1 - a^2 + 1e-6), not from a measurement (oracle/sac_f64_cases.py); what it rejects is
reported apart from the kink filter's share.

The constants are 4x what torch CPU float32 shows against the oracle on these inputs
(tools/sac_f64_margins.py, profiles/r10_sac_f64_margins.json):

  case               rejected   c_ref (torch)   native worst (MI355X)   native Adam ulps (v, p, target)
  d11_m1_b256         14.6 %        8.4             3.6                      5,  6, 0
  d14_m05_b768        15.5 %       10.1             4.6                      5,  4, 0
  d1_m1_b512          10.2 %        7.5             4.1                      5,  4, 0
  d11_m1_b256_tie      9.4 %        7.5             3.5                      5,  4, 0
  d11_m1_b256_step2   12.7 %        7.2             3.3                      6, 12, 0
                      (+ 62.2 % of the pool over the |x| limit)

  c = 40.3 (4 x 10.07), one bar for every gradient and loss of every case;
  c_a = 40.6 (4 x 10.14), native worst 9.8; c_l = 11.9 (4 x 2.96), native worst 3.2;
  Adam ulps: torch's own step sits 5 (exp_avg_sq), 6 (parameter), 0 (target) from the
  restatement; allowed 10, 12 and 2. For exp_avg_sq this is wider than restating torch's step
  from its own .grad would give (0..1 ulp, so 2): the native test can only read g back from
  exp_avg, which is ambiguous by one ulp, and exp_avg_sq squares it; torch read back the same
  way sits 5 ulps off, and the larger of the two readings sets the bound.
  Every case has elements with S == 0 (33k..129k); none has a non-zero gradient.

Every figure per tensor is in the profile's ``native`` half (recorded with
SACENV_F64_RECORD=<file> set for a run of this module).
"""
import ctypes as C
import json
import os

import pytest
import torch

import sac_f64_cases as K
from sac_f64 import learn_f64, policy_f64

pytestmark = pytest.mark.gpu

_RUNS: dict = {}      # case name -> figures of its one GPU run (shared by the tests of the case)
_RECORD: dict = {}    # what SACENV_F64_RECORD writes


def _native(gpu, case):
    from sacenv.sac_native import NativeSAC
    return NativeSAC(gpu, K.agent_config(case), obs_dim=case["obs_dim"], max_action=case["max_action"],
                     init_seed=case["seed"], with_memory=False)


def _state(nat) -> dict:
    """{"p", "m", "v"} of a NativeSAC as numpy copies."""
    out = {"p": K.np_state(nat.state_dicts())}
    for w, key in (("m", "exp_avg"), ("v", "exp_avg_sq")):
        out[w] = K.np_state({n: nat.adam_state(n)[key] for n in K.OPTIMISED})
    return out


def _rebuilt(gpu, case, nat):
    """A second agent from nat's state_dicts() and Adam state: its kernel copies come from sync()."""
    twin = _native(gpu, case)
    for n, sd in K.cpu_state_dicts(nat).items():
        getattr(twin, n).load_state_dict(sd)
    twin.load_optimizer_state(nat.optimizer_state())
    twin.sync()
    return twin


def _to(gpu, batch, noise):
    return tuple(t.to(gpu) for t in batch), tuple(t.to(gpu) for t in noise)


def _step(gpu, name, case, nat, step):
    """One learn() of ``nat`` on kink-free rows at its current weights, against the oracle."""
    sd = K.cpu_state_dicts(nat)
    batch, noise, shares = K.step_batch(sd, case, step)
    f = learn_f64(sd, batch, noise, K.case_cfg(case), case["max_action"])
    before = _state(nat)
    twin = _rebuilt(gpu, case, nat) if step > 1 else None
    gb, gn = _to(gpu, batch, noise)
    losses = [float(x) for x in nat.learn(gb, gn)]
    torch.cuda.synchronize()
    after = _state(nat)
    g = {n: {k: K.grad_from_moments(after["m"][n][k], None if step == 1 else before["m"][n][k])
             for k in after["m"][n]} for n in K.OPTIMISED}
    units, _ = K.grad_units(g, f)
    units.update(K.loss_units(losses, f))
    dead_bad = K.dead_nonzero_from_moments(after["m"], before["m"], f)   # exact, also on non-zero moments
    g32 = {n: {k: v.float().numpy() for k, v in g[n].items()} for n in K.OPTIMISED}
    fig = {"rejected_share": shares["kink"], "saturated_share": shares["saturated"], "units": units,
           "dead_elements": K.dead_elements(f), "dead_nonzero": dead_bad, "losses": losses,
           "done_share": float(batch[4].float().mean()), "inputs": (gb, gn),
           "adam_ulps": K.adam_ulps(before, after, g32, step, nat.cfg)}
    if twin is not None:   # the same step on the agent rebuilt before it: bit for bit
        tl = [float(x) for x in twin.learn(gb, gn)]
        torch.cuda.synchronize()
        fig["twin_learn_equal"] = bool(torch.equal(twin.weights, nat.weights)) and tl == losses
    _RECORD.setdefault("cases", {})[name] = {
        "rejected_share": shares["kink"], "saturated_share": shares["saturated"], "worst": max(units.values()),
        "units": units, "adam_ulps": fig["adam_ulps"], "dead_nonzero": dead_bad}
    return fig


def _run(gpu, name):
    """Case ``name`` once, also when it fails (the failure is kept and raised again: one fault
    means one run on the card)."""
    if name not in _RUNS:
        try:
            _RUNS[name] = _run_once(gpu, name)
        except Exception as e:
            _RUNS[name] = e
            raise
    if isinstance(_RUNS[name], Exception):
        raise _RUNS[name]
    return _RUNS[name]


def _run_once(gpu, name):
    """Step 1 against the oracle, the rebuilt agent's choose_action, and a second step on both
    agents (for K.STEP2 on freshly filtered rows, against the oracle too)."""
    case = K.CASES[name]
    nat = _native(gpu, case)
    if case["tie"]:
        K.tie_critics(nat)
        nat.sync()
    out = {"step1": _step(gpu, name, case, nat, 1)}
    twin = _rebuilt(gpu, case, nat)
    # the whole buffer: parameters, moments, target and the fragment-order copies of every fc2
    out["twin_buffer_equal"] = bool(torch.equal(twin.weights, nat.weights))
    obs, eps = K.act_inputs(case["obs_dim"], 200)
    out["twin_act_equal"] = bool(torch.equal(nat.choose_action(obs.to(gpu), eps.to(gpu)),
                                             twin.choose_action(obs.to(gpu), eps.to(gpu))))
    if name == K.STEP2:
        out["step2"] = _step(gpu, K.STEP2_NAME, case, nat, 2)
        out["twin_learn_equal"] = out["step2"]["twin_learn_equal"]
    else:   # the same rows again: bit equality needs no kink-free rows
        gb, gn = out["step1"]["inputs"]
        la, lb = nat.learn(gb, gn), twin.learn(gb, gn)
        torch.cuda.synchronize()
        out["twin_learn_equal"] = (bool(torch.equal(twin.weights, nat.weights))
                                   and [float(x) for x in la] == [float(x) for x in lb])
    return out


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    path = os.environ.get("SACENV_F64_RECORD")
    if path and _RECORD:
        with open(path, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)


def _check_units(name, fig):
    print(f"{name}: rejected {fig['rejected_share']:.3f} saturated {fig['saturated_share']:.3f} done {fig['done_share']:.3f} "
          f"worst {max(fig['units'].values()):.2f} units {fig['units']}")
    assert fig["rejected_share"] <= K.MAX_REJECT
    assert 0.05 <= fig["done_share"] <= 0.15
    assert fig["dead_elements"] > 0   # the exact-zero check below has elements to bite on
    assert fig["dead_nonzero"] == 0, "a gradient element whose every contribution is 0 is not exactly 0"
    bad = {k: v for k, v in fig["units"].items() if not v <= K.C_GRAD}
    assert not bad, (name, bad)


def _check_adam(name, fig):
    print(f"{name}: adam ulps {fig['adam_ulps']}")
    bad = {q: u for q, u in fig["adam_ulps"].items() if not u <= K.ADAM_ULPS[q]}
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", list(K.CASES))
def test_learn_gradients_and_losses_per_element(gpu, built_lib, name):
    _check_units(name, _run(gpu, name)["step1"])


def test_learn_second_step_gradients_per_element(gpu, built_lib):
    """Non-zero moments: g2 = m1 + (m2 - m1) / lerp_w, the oracle at the weights the kernel
    holds after step 1, rows filtered again at those weights."""
    _check_units(K.STEP2_NAME, _run(gpu, K.STEP2)["step2"])


@pytest.mark.parametrize("name", list(K.CASES))
def test_learn_adam_per_element(gpu, built_lib, name):
    _check_adam(name, _run(gpu, name)["step1"])


def test_learn_adam_second_step_per_element(gpu, built_lib):
    """Bias corrections at step = 2 on non-zero moments."""
    _check_adam(K.STEP2_NAME, _run(gpu, K.STEP2)["step2"])


@pytest.mark.parametrize("name", list(K.CASES))
def test_kernel_copies_match_a_rebuilt_agent(gpu, built_lib, name):
    """After learn(): choose_action, and a second learn() (the whole weights buffer: parameters,
    moments, target, fragment-order copies), against an agent rebuilt from state_dicts() + sync()."""
    r = _run(gpu, name)
    assert r["twin_buffer_equal"]
    assert r["twin_act_equal"]
    assert r["twin_learn_equal"]


def _act(nat, obs, eps, n, with_logp, pad=7, sentinel=-777.0):
    from sacenv import _lib
    out = torch.full((n + pad,), sentinel, dtype=torch.float32, device=nat.device)
    lp = torch.full((n + pad,), sentinel, dtype=torch.float32, device=nat.device)
    _lib.check(_lib.load().sacenv_sac_act(C.byref(nat.params), nat.weights.data_ptr(), obs.data_ptr(), n,
                                          eps.data_ptr(), out.data_ptr(), lp.data_ptr() if with_logp else None,
                                          nat._stream()))
    torch.cuda.synchronize()
    return out.cpu(), lp.cpu()


@pytest.mark.parametrize("policy", K.ACT_POLICIES)
@pytest.mark.parametrize("max_action", K.ACT_MAX_ACTIONS)
@pytest.mark.parametrize("obs_dim", K.ACT_OBS_DIMS)
def test_act_action_and_log_prob_per_row(gpu, built_lib, obs_dim, max_action, policy):
    from sacenv.sac_native import NativeSAC
    nat = NativeSAC(gpu, None, obs_dim=obs_dim, max_action=max_action, init_seed=obs_dim, with_memory=False)
    if policy == "wide":
        K.widen_policy(nat)
        nat.sync()
    actor = {k: v.detach().cpu().clone() for k, v in nat.actor.state_dict().items()}
    worst_a = worst_l = 0.0
    saturated = 0
    for n in K.ACT_ROWS:
        obs, eps = K.act_inputs(obs_dim, n)
        go, ge = obs.to(gpu).contiguous(), eps.to(gpu).reshape(-1).contiguous()
        out, lp = _act(nat, go, ge, n, True)
        assert bool((out[n:] == -777.0).all()) and bool((lp[n:] == -777.0).all()), "wrote past n"
        p = policy_f64(actor, obs, eps, max_action)
        ua, ul = K.act_units(out[:n], lp[:n], p, max_action)
        worst_a, worst_l = max(worst_a, ua), max(worst_l, ul)
        saturated += int((p["x"].abs() > 9).sum())
        out0, lp0 = _act(nat, go, ge, n, False)   # the NULL log_prob path: same actions, buffer untouched
        assert torch.equal(out0, out) and bool((lp0 == -777.0).all())
    print(f"act d{obs_dim} M{max_action} {policy}: action {worst_a:.2f} log_prob {worst_l:.2f} units, "
          f"{saturated} rows with |x| > 9")
    _RECORD.setdefault("act", {})[f"d{obs_dim}_m{max_action}_{policy}"] = {"action": worst_a, "log_prob": worst_l}
    if policy == "wide" and max_action == 1.0:
        assert saturated > 0   # the wide policy reaches full saturation (tanh(x) == 1 in float32)
    assert worst_a <= K.C_ACT, worst_a
    assert worst_l <= K.C_LOGP, worst_l
