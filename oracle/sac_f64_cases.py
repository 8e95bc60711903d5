"""The cases, batches and error units of the SAC f64 parity tests (checker only).

Shared by tests/test_sac_f64_cpu.py, tests/test_sac_native_f64_gpu.py and
tools/sac_f64_margins.py, so that the reference margins are measured on
exactly the inputs the GPU tests use. See oracle/sac_f64.py for the oracle.
"""
from __future__ import annotations

import numpy as np
import torch

from sac_f64 import OPTIMISED, kink_free_rows, learn_f64, policy_f64

U24 = 2.0 ** -24          # the unit roundoff of float32
DELTA_Z = 1e-5            # fixed: 100x the largest fp32-vs-f64 error of a near-zero pre-activation
DELTA_Q = 1e-5
MAX_REJECT = 0.25         # the row filter may reject at most this share of a candidate pool
ORDER = ("value", "actor", "critic_1", "critic_2")   # learn()'s loss order

# learn() cases; "tie": critic_2's weights copied from critic_1 (every row an exact tie of min(q1, q2))
CASES = {
    "d11_m1_b256": dict(obs_dim=11, max_action=1.0, batch=256, seed=11, agent={}, tie=False),
    "d14_m05_b768": dict(obs_dim=14, max_action=0.5, batch=768, seed=14, tie=False,
                         agent=dict(gamma=0.9, reward_scale=2.0, tvn_parameter_modulation_tau=0.05,
                                    learning_rate_alpha=0.001, learning_rate_beta=0.002)),
    "d1_m1_b512": dict(obs_dim=1, max_action=1.0, batch=512, seed=1, agent={}, tie=False),
    "d11_m1_b256_tie": dict(obs_dim=11, max_action=1.0, batch=256, seed=11, agent={}, tie=True),
}
STEP2 = "d11_m1_b256"     # the case whose second step is checked too
STEP2_NAME = STEP2 + "_step2"

# sacenv_sac_act configurations
ACT_OBS_DIMS = (1, 11, 14)
ACT_MAX_ACTIONS = (1.0, 0.5)
ACT_ROWS = (1, 63, 64, 65, 200)     # around the 64-row workgroup
ACT_POLICIES = ("init", "wide")     # wide: mean.bias += 1.5, std.bias = 2


# The bars, in the units of the functions below: 4x the worst torch CPU float32 shows against
# the oracle on these very inputs (tools/sac_f64_margins.py -> profiles/r10_sac_f64_margins.json;
# tests/test_sac_f64_cpu.py holds the two together).
C_GRAD = 40.3          # gradients and losses: 4 x 10.07
C_ACT = 40.6           # action: 4 x 10.14
C_LOGP = 11.9          # log-prob: 4 x 2.96
# Adam restatement, ulps: max(2, 2 x torch's own step's distance) per quantity. The distance is
# the larger of two readings of torch's step: restated from its own .grad (0..1 ulp for
# exp_avg_sq) and from g read back from exp_avg, as the native test has to read it (5 ulps: g is
# ambiguous by one ulp, and exp_avg_sq squares it).
ADAM_ULPS = {"exp_avg_sq": 10.0, "param": 12.0, "target": 2.0}

# The second step's rows are also kept out of tanh saturation: |x| <= X_LIMIT at both draws.
# After one default Adam step (lr 0.005 on every weight) sigma is 2..5.6, and where tanh(x)
# rounds to +-1 the factor 2a / (1 - a^2 + 1e-6) * (1 - tanh^2) of the actor gradient is 0 in
# float32 and ~0.3 in float64, for any float32 implementation (torch on unfiltered rows: 51 822
# units). Like a kink this is a property of a row. The limit is fixed from the conditioning, not
# measured: a one-ulp error of tanh moves log(1 - a^2 + 1e-6) by 2^-24 * 2 / (1 - a^2), and
# 2 / (1 - tanh(3)^2) = 203; were every one of B = 256 rows at the limit, independent roundings
# would add up to 203 / sqrt(256) = 13 units, inside c. The share of rows it rejects is reported
# on its own; the kink filter's cap is unchanged.
X_LIMIT = 3.0
STEP2_POOL = 8         # the second step draws from 8 B candidates (the other cases from 1.5 B)


def agent_config(case: dict) -> dict:
    return {"agent": dict(case["agent"], batch_size=case["batch"])}


def cpu_state_dicts(agent) -> dict:
    return {n: {k: v.detach().cpu().clone() for k, v in sd.items()} for n, sd in agent.state_dicts().items()}


def tie_critics(agent) -> None:
    """critic_2 <- critic_1 in place (a NativeSAC needs sync() afterwards)."""
    with torch.no_grad():
        for p2, p1 in zip(agent.critic_2.parameters(), agent.critic_1.parameters()):
            p2.copy_(p1)


def widen_policy(agent) -> None:
    """Rows through partial and full tanh saturation and the top of the sigma range."""
    with torch.no_grad():
        agent.actor.mean.bias.add_(1.5)
        agent.actor.std.bias.fill_(2.0)


def candidate_pool(obs_dim: int, rows: int, seed: int):
    """(state, action, reward f64, new_state, eps1, eps2) of ``rows`` candidate rows."""
    g = torch.Generator().manual_seed(seed)
    s = torch.rand((rows, obs_dim), generator=g) * 1.2 - 0.1
    a = torch.rand((rows, 1), generator=g) * 2 - 1
    r = (torch.rand(rows, generator=g, dtype=torch.float64) - 0.8) * 3
    s2 = s + 0.01 * torch.randn((rows, obs_dim), generator=g)
    e1, e2 = torch.randn((rows, 1), generator=g), torch.randn((rows, 1), generator=g)
    return s, a, r, s2, e1, e2


def done_pattern(rows: int, seed: int) -> torch.Tensor:
    """About 10 % done rows; every 16-row block has at least one done and one not-done row."""
    g = torch.Generator().manual_seed(seed + 7919)
    d = torch.rand(rows, generator=g) < 0.04
    for b in range(rows // 16):
        d[16 * b + (5 * b + 3) % 16] = True
        d[16 * b + (5 * b + 4) % 16] = False
    return d


def select_batch(state_dicts: dict, case: dict, seed: int, delta_q=DELTA_Q, x_limit=None):
    """The first B kink-free rows (at ``state_dicts``) of a pool of 1.5 B candidates; with
    ``x_limit`` the rows must also have |x| <= x_limit at both draws, and the pool is STEP2_POOL B.
    Returns (batch, noise, shares): ``shares["kink"]`` is what the kink filter rejected of the
    whole pool (more than MAX_REJECT raises), ``shares["saturated"]`` what the |x| limit rejected."""
    B = case["batch"]
    s, a, r, s2, e1, e2 = candidate_pool(case["obs_dim"], 3 * B // 2 if x_limit is None else STEP2_POOL * B, seed)
    d = torch.zeros(s.shape[0], dtype=torch.bool)   # done plays no part in the margins
    pool = (state_dicts, (s, a, r, s2, d), (e1, e2), case_cfg(case), case["max_action"])
    keep, share = kink_free_rows(*pool, DELTA_Z, delta_q)
    if share > MAX_REJECT:
        raise AssertionError(f"the kink filter rejected {share:.1%} of the candidate rows (cap {MAX_REJECT:.0%})")
    shares = {"kink": share, "saturated": 0.0}
    if x_limit is not None:
        f = learn_f64(*pool, grads=False)
        ok = (f["abs_x_sample"] <= x_limit) & (f["abs_x_rsample"] <= x_limit)
        shares["saturated"] = 1.0 - float(ok.double().mean())
        keep = keep[ok[keep]]
    k = keep[:B]
    if k.numel() != B:
        raise AssertionError(f"only {k.numel()} of {s.shape[0]} candidate rows pass, {B} needed")
    return (s[k], a[k], r[k], s2[k], done_pattern(B, seed)), (e1[k], e2[k]), shares


def case_cfg(case: dict) -> dict:
    a = case["agent"]
    return {"gamma": a.get("gamma", 0.99), "reward_scale": a.get("reward_scale", 10.0)}


def case_delta_q(case: dict):
    return None if case["tie"] else DELTA_Q


def step_batch(state_dicts: dict, case: dict, step: int):
    """The batch of the case's ``step``-th learn() at ``state_dicts`` (select_batch's returns);
    the second step's rows are also held to X_LIMIT."""
    return select_batch(state_dicts, case, case["seed"] + 100 * (step - 1), case_delta_q(case),
                        X_LIMIT if step > 1 else None)


def dead_elements(f: dict) -> int:
    """How many parameter elements have S == 0 (what the exact-zero check has to bite on)."""
    return sum(int((S == 0).sum()) for n in OPTIMISED for S in f["S"][n].values())


# ---------------------------------------------------------------- error units

def grad_units(got: dict, f: dict):
    """{net.param: max |got - g_f64| / (2^-24 S_max)} and the number of elements with S == 0
    whose gradient is not exactly 0. ``got``: [net][param] float64 tensors."""
    units, dead_bad = {}, 0
    for n in OPTIMISED:
        for k, g64 in f["grad"][n].items():
            g = got[n][k].reshape(g64.shape).to(torch.float64)
            S = f["S"][n][k]
            dead = S == 0
            dead_bad += int((g[dead] != 0).sum())
            units[f"{n}.{k}"] = float((g - g64).abs().max() / (U24 * f["S_max"][n][k]))
    return units, dead_bad


def dead_nonzero_from_moments(m_new: dict, m_old: dict, f: dict) -> int:
    """The number of elements with S == 0 whose first moment did not move as a gradient of
    exactly 0 moves it: m_new == m_old + lerp_w (0 - m_old) in float32, bit for bit. (Reading
    g = m_old + (m_new - m_old) / lerp_w back cannot show an exact 0 once m_old != 0.)"""
    bad = 0
    for n in OPTIMISED:
        for k, S in f["S"][n].items():
            dead = (S == 0).numpy().reshape(-1)
            m0 = np.asarray(m_old[n][k], dtype=np.float32).reshape(-1)[dead]
            m1 = np.asarray(m_new[n][k], dtype=np.float32).reshape(-1)[dead]
            bad += int((m1 != m0 + np.float32(LERP_W) * (np.float32(0) - m0)).sum())
    return bad


def dropped_row_units(f: dict, f_row: dict, rows: int) -> dict:
    """What leaving one row out of the batch reductions does, in the gradient unit: f_row is
    learn_f64 of that row alone, so its share of the batch gradient is grad / rows."""
    return {f"{n}.{k}": float((g / rows).abs().max() / (U24 * f["S_max"][n][k]))
            for n in OPTIMISED for k, g in f_row["grad"][n].items()}


def loss_units(got, f: dict) -> dict:
    """{loss: |got - L_f64| / (2^-24 mean |per-row term|)}."""
    got = torch.as_tensor([float(x) for x in got], dtype=torch.float64)
    u = (got - f["losses"]).abs() / (U24 * f["loss_scale"])
    return {f"loss.{n}": float(x) for n, x in zip(ORDER, u)}


def act_units(action, log_prob, p: dict, max_action: float):
    """(max action error / (2^-24 M (1 + |x|)), max log-prob error / (2^-24 (1 + |lp| +
    2 / (1 - a^2 + 1e-6)))): the last term is the fp32 conditioning of log(1 - a^2 + 1e-6)."""
    a = torch.as_tensor(action).detach().cpu().reshape(-1).to(torch.float64)
    lp = torch.as_tensor(log_prob).detach().cpu().reshape(-1).to(torch.float64)
    ua = (a - p["action"]).abs() / (U24 * max_action * (1 + p["x"].abs()))
    ul = (lp - p["log_prob"]).abs() / (U24 * (1 + p["log_prob"].abs() + 2 / (1 - p["action"] ** 2 + 1e-6)))
    return float(ua.max()), float(ul.max())


def act_inputs(obs_dim: int, n: int):
    g = torch.Generator().manual_seed(1000 * obs_dim + n)
    obs = torch.rand((n, obs_dim), generator=g) * 1.2 - 0.1
    eps = torch.randn((n, 1), generator=g)
    return obs, eps


# ---------------------------------------------------------------- Adam, restated in numpy float32

LERP_W = float(np.float32(1.0 - 0.9))   # exp_avg.lerp_(grad, 1 - beta1), as float32


def grad_from_moments(m_new, m_old=None) -> torch.Tensor:
    """The gradient a lerp step used, from the first moment before and after it (float64):
    m_new = m_old + lerp_w (g - m_old). From zero moments g = m_new / lerp_w, to one ulp."""
    m_new = torch.as_tensor(m_new).detach().cpu().to(torch.float64)
    if m_old is None:
        return m_new / LERP_W
    m_old = torch.as_tensor(m_old).detach().cpu().to(torch.float64)
    return m_old + (m_new - m_old) / LERP_W


def adam_restate(p, m, v, g, step: int, lr: float, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's step in its foreach form (the one sacenv_sac.hip documents), float32
    throughout, Python-float scalars cast to float32 where torch casts them. Returns (p, m, v)."""
    f = np.float32
    p, m, v, g = (np.asarray(x, dtype=f) for x in (p, m, v, g))
    lerp_w, b2f, omb2 = f(1.0 - b1), f(b2), f(1.0 - b2)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    bc2s, epsf, nstep = f(bc2 ** 0.5), f(eps), f((lr / bc1) * -1.0)
    m = m + lerp_w * (g - m)
    v = v * b2f + (omb2 * g) * g
    den = np.sqrt(v) / bc2s + epsf
    p = p + nstep * (m / den)
    return p, m, v


def soft_update_restate(p, t, tau: float):
    f = np.float32
    return f(tau) * np.asarray(p, dtype=f) + f(1.0 - tau) * np.asarray(t, dtype=f)


def ulp_dist(a, b, *at) -> float:
    """max |a - b| in float32 ulps at the largest magnitude among a, b and ``at`` (the operands
    of the last addition: where they cancel, the result inherits their rounding)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    mag = np.maximum(np.abs(a), np.abs(b))
    for x in at:
        mag = np.maximum(mag, np.abs(np.asarray(x, dtype=np.float32)))
    mag = np.maximum(mag, np.finfo(np.float32).tiny)
    d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(mag).astype(np.float64)
    return float(d.max()) if d.size else 0.0


def adam_ulps(before: dict, after: dict, grads: dict, step: int, cfg, tau_target: bool = True) -> dict:
    """Element-by-element Adam check of one learn(): restate the step from ``grads`` (float32,
    [net][param]) and the state before it, and measure the distance to the state after it.
    ``before`` / ``after``: {"p": [net][param], "m": ..., "v": ...} with ``p`` holding all five
    nets. Returns the worst ulp distance of exp_avg_sq, of the parameters and of the target."""
    worst = {"exp_avg_sq": 0.0, "param": 0.0, "target": 0.0}
    for n in OPTIMISED:
        lr = cfg.lr_alpha if n == "actor" else cfg.lr_beta
        for k in before["p"][n]:
            p0, m0, v0 = (np.asarray(before[w][n][k], dtype=np.float32) for w in ("p", "m", "v"))
            g = np.asarray(grads[n][k], dtype=np.float32).reshape(p0.shape)
            p1, _, v1 = adam_restate(p0, m0, v0, g, step, lr)
            worst["exp_avg_sq"] = max(worst["exp_avg_sq"], ulp_dist(after["v"][n][k], v1))
            worst["param"] = max(worst["param"], ulp_dist(after["p"][n][k], p1, p0))
            if n == "value" and tau_target:
                t0 = before["p"]["target_value"][k]
                t1 = soft_update_restate(after["p"][n][k], t0, cfg.tau)
                worst["target"] = max(worst["target"], ulp_dist(after["p"]["target_value"][k], t1, t0))
    return worst


def np_state(tree: dict) -> dict:
    return {n: {k: v.detach().float().cpu().numpy().copy() for k, v in sd.items()} for n, sd in tree.items()}


# ---------------------------------------------------------------- torch CPU float32 against the oracle

def torch_state(agent) -> dict:
    """{"p", "m", "v"} of a VecSAC (zeros where an optimiser has no state yet)."""
    opts = dict(zip(OPTIMISED, (agent.opt_actor, agent.opt_c1, agent.opt_c2, agent.opt_value)))
    out = {"p": np_state(agent.state_dicts()), "m": {}, "v": {}}
    for n in OPTIMISED:
        net, st = getattr(agent, n), opts[n].state
        for w, key in (("m", "exp_avg"), ("v", "exp_avg_sq")):
            out[w][n] = {k: (st[p][key].detach().numpy().copy() if p in st else np.zeros(p.shape, np.float32))
                         for k, p in net.named_parameters()}
    return out


def torch_reference(name: str) -> dict:
    """Case ``name`` on VecSAC("cpu") in float32 against the oracle: c_ref per tensor and loss,
    the Adam restatement's ulp distances and the filter's rejected share; for STEP2 also its
    second step (under STEP2_NAME). Returns {case name: figures}."""
    from sacenv.agent import VecSAC
    case = CASES[name]
    agent = VecSAC("cpu", agent_config(case), obs_dim=case["obs_dim"], max_action=case["max_action"],
                   init_seed=case["seed"], with_memory=False)
    if case["tie"]:
        tie_critics(agent)
    out = {}
    for step in (1, 2) if name == STEP2 else (1,):
        sd = cpu_state_dicts(agent)
        batch, noise, shares = step_batch(sd, case, step)
        f = learn_f64(sd, batch, noise, case_cfg(case), case["max_action"])
        before = torch_state(agent)
        losses = agent.learn(batch, noise)
        after = torch_state(agent)
        own = {n: {k: p.grad.detach().clone() for k, p in getattr(agent, n).named_parameters()} for n in OPTIMISED}
        units, dead_bad = grad_units(own, f)
        units.update(loss_units(losses, f))
        # the Adam restatement from torch's own gradient, and from the gradient read back from
        # the first moment as the native test has to read it
        read = {n: {k: grad_from_moments(after["m"][n][k], None if step == 1 else before["m"][n][k]).float()
                    for k in own[n]} for n in OPTIMISED}
        ulps_own = adam_ulps(before, after, own, step, agent.cfg)
        ulps_read = adam_ulps(before, after, read, step, agent.cfg)
        out[name if step == 1 else STEP2_NAME] = {
            "rejected_share": shares["kink"], "saturated_share": shares["saturated"],
            "dead_elements": dead_elements(f), "c_ref": units, "c_ref_max": max(units.values()), "dead_nonzero": dead_bad,
            "adam_ulps_own_grad": ulps_own, "adam_ulps_read_back": ulps_read}
    return out


def torch_act_reference() -> dict:
    """Actor.sample_normal in float32 on the CPU against policy_f64 over the act configurations:
    the worst action and log-prob error in their units."""
    from sacenv.agent import VecSAC
    worst_a = worst_l = 0.0
    for D in ACT_OBS_DIMS:
        for M in ACT_MAX_ACTIONS:
            for pol in ACT_POLICIES:
                agent = VecSAC("cpu", None, obs_dim=D, max_action=M, init_seed=D, with_memory=False)
                if pol == "wide":
                    widen_policy(agent)
                for n in ACT_ROWS:
                    obs, eps = act_inputs(D, n)
                    with torch.no_grad():
                        a, lp = agent.actor.sample_normal(obs, reparameterize=False, eps=eps)
                    ua, ul = act_units(a, lp, policy_f64(agent.actor.state_dict(), obs, eps, M), M)
                    worst_a, worst_l = max(worst_a, ua), max(worst_l, ul)
    return {"c_a_ref": worst_a, "c_l_ref": worst_l}
