"""float64 restatement of one SAC learn() with a weight per batch row on the critics' TD loss
(checker only; include/sacenv_weighted_learn.h, ``VecSAC.learn(weights=)``).

``learn_f64_weighted`` is oracle/sac_f64.py's ``learn_f64`` -- the same ``_Net`` / ``_Tape``, the same
order of the forward passes -- with the two critic rows ``w * 0.5 (q - q_hat)^2``. The tape's S follows
``|grad_out|``, so the weights flow into it; the critics' ``loss_scale`` is the mean |weighted row
term|. With ``weights == 1`` every figure equals ``learn_f64``'s, ``torch.equal``
(tests/test_weighted_learn_cpu.py).

``draw_weights`` gives the weights the tests use: (min leaf / leaf)^0.4 of the leaves
``prio_oracle.td_leaves`` forms from log-uniform TD errors, spanning about (0.05, 1].
"""
from __future__ import annotations

import numpy as np
import torch

import prio_oracle
from sac_f64 import _LAYERS, OPTIMISED, _cfg, _draw, _f32_then_d, _Net, _sigma, _Tape

ORDER = ("value", "actor", "critic_1", "critic_2")
BETA = 0.4


def draw_weights(rows: int, seed: int, beta: float = BETA) -> torch.Tensor:
    """f32 [rows]: the importance weights of a batch whose TD errors are log-uniform on
    [1e-3, 300] (alpha 0.6, eps 1e-3); the largest is 1.0, the smallest about 0.06."""
    rng = np.random.default_rng(seed)
    td1 = np.exp(rng.uniform(np.log(1e-3), np.log(300.0), rows))
    td2 = td1 * np.exp(rng.uniform(-0.5, 0.5, rows))
    leaf = prio_oracle.td_leaves((td1 ** 2).astype(np.float32), (td2 ** 2).astype(np.float32), 0.6, 1e-3)
    return torch.from_numpy(prio_oracle.weights(leaf, beta))


def learn_f64_weighted(state_dicts: dict, batch, noise, weights, cfg, max_action: float) -> dict:
    """``learn_f64(state_dicts, batch, noise, cfg, max_action)`` with the critic losses
    ``0.5 mean(w (q - q_hat)^2)``; ``weights`` [B], read as float32. Returns ``losses``,
    ``loss_scale``, ``rows``, ``grad`` / ``S`` / ``S_max`` ([net][param]) and ``min_abs_z``."""
    gamma, scale = _cfg(cfg)
    M = float(max_action)
    state, action, reward, state_, done = batch
    state, action, reward, state_ = (_f32_then_d(t) for t in (state, action, reward, state_))
    B = state.shape[0]
    action, reward = action.reshape(B, 1), reward.reshape(B)
    done = torch.as_tensor(done).detach().to("cpu").to(torch.bool).reshape(B)
    e1, e2 = (_f32_then_d(e).reshape(B, 1) for e in noise)
    w = _f32_then_d(weights).reshape(B)

    tape = _Tape(B)
    net = {n: _Net(n, state_dicts[n], tape) for n in _LAYERS}
    both = lambda s, a: (net["critic_1"].q(net["critic_1"].trunk(torch.cat([s, a], 1))).view(-1),  # noqa: E731
                         net["critic_2"].q(net["critic_2"].trunk(torch.cat([s, a], 1))).view(-1))

    tape.own = "value"
    value = net["value"].v(net["value"].trunk(state)).view(-1)
    tape.own = "actor"
    h = net["actor"].trunk(state)
    mu, sigma = net["actor"].mean(h), _sigma(net["actor"].std(h))
    tape.own = None
    with torch.no_grad():
        value_ = net["target_value"].v(net["target_value"].trunk(state_)).view(-1)
        value_ = torch.where(done, torch.zeros_like(value_), value_)
        _, a1, lp1 = _draw(mu, sigma, e1, M)
        q1s, q2s = both(state, a1)
        value_target = torch.min(q1s, q2s) - lp1.view(-1)
    value_rows = 0.5 * (value - value_target) ** 2

    _, a2, lp2 = _draw(mu, sigma, e2, M)
    q1r, q2r = both(state, a2)
    actor_rows = lp2.view(-1) - torch.min(q1r, q2r)

    q_hat = scale * reward + gamma * value_
    crit_rows = []
    for c in ("critic_1", "critic_2"):
        tape.own = c
        q = net[c].q(net[c].trunk(torch.cat([state, action], 1))).view(-1)
        crit_rows.append(w * (0.5 * (q - q_hat) ** 2))     # the one line that differs from learn_f64
    tape.own = None

    rows = {"value": value_rows, "actor": actor_rows, "critic_1": crit_rows[0], "critic_2": crit_rows[1]}
    out = {
        "losses": torch.stack([rows[n].mean() for n in ORDER]).detach(),
        "loss_scale": torch.stack([rows[n].abs().mean() for n in ORDER]).detach(),
        "rows": {n: rows[n].detach() for n in ORDER},
        "min_abs_z": tape.min_abs_z,
        "grad": {}, "S": {}, "S_max": {},
    }
    for n in OPTIMISED:
        names = [k for k, _ in net[n].named_parameters()]
        g = torch.autograd.grad(rows[n].mean(), list(net[n].parameters()))
        out["grad"][n] = dict(zip(names, g))
        out["S"][n] = {k: tape.S[n][k].reshape(gk.shape) for k, gk in out["grad"][n].items()}
        out["S_max"][n] = {k: float(s.max()) for k, s in out["S"][n].items()}
    return out


# ---------------------------------------------------------------- the bar and the torch reference

# The bar of the weighted critic gradients and losses, in the unit of oracle/sac_f64_cases.py
# (c 2^-24 S_max per tensor, c 2^-24 mean |row term| per loss): 4 x the worst that torch CPU float32
# (VecSAC.learn(weights=)) shows against learn_f64_weighted on these very inputs, c_ref_w = 10.08
# at the second step of d11_m1_b256; that it lands on the unweighted bar's 40.3 is measured, not
# assumed (tools/weighted_learn_margins.py -> profiles/weighted_learn_f64_margins.json;
# tests/test_weighted_learn_cpu.py holds the two together). The factor 4 is the margin the project
# gives its kernels over torch for a different but legitimate summation order.
C_W = 40.3
WEIGHTED = ("critic_1", "critic_2")


def case_weights(case: dict, step: int = 1) -> torch.Tensor:
    """The weights of the case's ``step``-th learn (a function of the case alone)."""
    return draw_weights(case["batch"], case["seed"] + 100 * (step - 1) + 5000)


def critic_units(units: dict) -> dict:
    """The figures the weights reach: both critics' tensors and losses."""
    return {k: v for k, v in units.items() if k.split(".")[0] in WEIGHTED or k in ("loss.critic_1", "loss.critic_2")}


def torch_reference_weighted(name: str) -> dict:
    """Case ``name`` (and for K.STEP2 its second step) on ``VecSAC("cpu").learn(weights=)`` in
    float32 against the weighted oracle, as ``sac_f64_cases.torch_reference`` does unweighted.
    Returns {case name: {"rejected_share", "c_ref" (critics' figures), "c_ref_max", "other_max"
    (the unweighted nets' figures), "dead_nonzero", "w_min", "w_max"}}."""
    import sac_f64_cases as K
    from sacenv.agent import VecSAC
    case = K.CASES[name]
    agent = VecSAC("cpu", K.agent_config(case), obs_dim=case["obs_dim"], max_action=case["max_action"],
                   init_seed=case["seed"], with_memory=False)
    if case["tie"]:
        K.tie_critics(agent)
    out = {}
    for step in (1, 2) if name == K.STEP2 else (1,):
        sd = K.cpu_state_dicts(agent)
        batch, noise, shares = K.step_batch(sd, case, step)
        w = case_weights(case, step)
        f = learn_f64_weighted(sd, batch, noise, w, K.case_cfg(case), case["max_action"])
        losses = agent.learn(batch, noise, w)
        own = {n: {k: p.grad.detach().clone() for k, p in getattr(agent, n).named_parameters()} for n in OPTIMISED}
        units, dead_bad = K.grad_units(own, f)
        units.update(K.loss_units(losses, f))
        crit = critic_units(units)
        out[name if step == 1 else K.STEP2_NAME] = {
            "rejected_share": shares["kink"], "saturated_share": shares["saturated"], "c_ref": crit,
            "c_ref_max": max(crit.values()), "other_max": max(v for k, v in units.items() if k not in crit),
            "dead_nonzero": dead_bad, "w_min": float(w.min()), "w_max": float(w.max())}
    return out


__all__ = ["learn_f64_weighted", "draw_weights", "case_weights", "critic_units", "torch_reference_weighted",
           "BETA", "C_W"]
