"""float64 restatement of one SAC ``learn()`` and of the policy draw (checker only).

Plain torch on the CPU in float64, restating ``sacenv/agent.py``
(``Actor.sample_normal``, ``VecSAC.learn``) — not the kernels of
``sacenv_sac.hip``. It is the high-precision side of the per-element parity
tests (tests/test_sac_f64_cpu.py, tests/test_sac_native_f64_gpu.py).

``policy_f64``  the tanh-squashed Normal draw per row.
``learn_f64``   the four losses, the gradient of every parameter of actor,
                critic_1, critic_2 and value (each at the starting parameters:
                the four losses of one learn() are independent, and the value
                target and q_hat are detached as VecSAC.learn does), and with
                them what a float32 implementation can be held to:

  * ``S[net][param]``: the abs-sum of the parameter's per-row contributions,
    ``|grad_out|^T |layer_in|`` for a weight and ``sum_r |grad_out|`` for a
    bias, from forward and backward hooks on the ``nn.Linear``s. fp32
    summation error is a multiple of ``2^-24 S``; S stays meaningful where the
    sum itself cancels, and ``S == 0`` (a dead ReLU unit) means the gradient is
    exactly 0. ``S_max[net][param]`` is its maximum over the tensor.
  * ``min_abs_z``: per row, the smallest |pre-activation| over every fc1 / fc2
    evaluation the learn makes (actor, value, target on new_state, both
    critics at the stored, the sample() and the rsample() action).
  * ``dq_sample`` / ``dq_rsample``: per row, |q1 - q2| at the two draws.
  * ``abs_x_sample`` / ``abs_x_rsample``: per row, |x| before the tanh squash at the two
    draws (how far the row sits into saturation).

``kink_free_rows`` keeps the rows whose margins are at least ``delta_z`` /
``delta_q``. On such rows every implementation takes the same ReLU masks and
the same ``min`` branch, the gradient is a smooth function of the inputs and
fp32 rounding theory applies; a pre-activation within fp32 error of zero may
legitimately flip and move a gradient element by ~1/B. Kink-freeness is a
property of a row, so a B-row batch is the first B accepted rows of a pool.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

F64 = torch.float64
LOG_STD_MIN, LOG_STD_MAX = -5.0, 2.0   # networks.py:50-56
REPARAM_NOISE = 1e-6
OPTIMISED = ("actor", "critic_1", "critic_2", "value")
_LAYERS = {"actor": ("fc1", "fc2", "mean", "std"), "critic_1": ("fc1", "fc2", "q"),
           "critic_2": ("fc1", "fc2", "q"), "value": ("fc1", "fc2", "v"),
           "target_value": ("fc1", "fc2", "v")}


def _d(x) -> torch.Tensor:
    """Any array-like as a CPU float64 tensor (a float32 value converts exactly)."""
    return torch.as_tensor(x).detach().to("cpu", F64)


def _f32_then_d(x) -> torch.Tensor:
    """As VecSAC.learn reads a batch field: cast to float32 first (reward arrives as float64)."""
    return torch.as_tensor(x).detach().to("cpu").to(torch.float32).to(F64)


class _Tape:
    """What the hooks on the nn.Linears collect over one learn_f64()."""

    def __init__(self, rows: int):
        self.min_abs_z = torch.full((rows,), math.inf, dtype=F64)
        self.own = None   # the net whose own loss the current forward belongs to
        self.S = {n: {} for n in OPTIMISED}


class _Net(nn.Module):
    """One of the five MLPs in float64, layers named as sacenv.agent names them."""

    def __init__(self, name: str, sd: dict, tape: _Tape | None):
        super().__init__()
        self.net_name = name
        for lname in _LAYERS[name]:
            w, b = _d(sd[f"{lname}.weight"]), _d(sd[f"{lname}.bias"])
            lin = nn.Linear(w.shape[1], w.shape[0]).to(F64)
            with torch.no_grad():
                lin.weight.copy_(w)
                lin.bias.copy_(b)
            if tape is not None:
                lin.register_forward_hook(self._hook(lname, tape))
            setattr(self, lname, lin)

    def _hook(self, lname: str, tape: _Tape):
        net = self.net_name

        def fwd(_mod, inputs, out):
            if lname in ("fc1", "fc2"):
                tape.min_abs_z = torch.minimum(tape.min_abs_z, out.detach().abs().min(dim=1).values)
            if tape.own == net and out.requires_grad:
                x = inputs[0].detach().abs()

                def bwd(g):   # backward hook on the layer's output: d loss / d out, per row
                    ga = g.detach().abs()
                    tape.S[net][f"{lname}.weight"] = ga.t() @ x
                    tape.S[net][f"{lname}.bias"] = ga.sum(0)
                out.register_hook(bwd)
        return fwd

    def trunk(self, x):
        return torch.relu(self.fc2(torch.relu(self.fc1(x))))


def _sigma(raw):
    log_std = LOG_STD_MIN + 0.5 * (LOG_STD_MAX - LOG_STD_MIN) * (torch.tanh(raw) + 1)
    return log_std.exp()


def _draw(mu, sigma, eps, max_action: float):
    """Actor.sample_normal after the heads: x = mean + eps * std, the squash, the log-prob."""
    x = mu + eps * sigma
    action = torch.tanh(x) * max_action
    lp = -((x - mu) ** 2) / (2 * sigma ** 2) - sigma.log() - math.log(math.sqrt(2 * math.pi))
    lp = lp - torch.log(1 - action.pow(2) + REPARAM_NOISE)
    return x, action, lp


@torch.no_grad()
def policy_f64(actor_state_dict: dict, obs, eps, max_action: float) -> dict:
    """``Actor.sample_normal(obs, eps=eps)`` per row: action, log_prob, x, mu, sigma ([N] each)."""
    net = _Net("actor", actor_state_dict, None)
    obs = _f32_then_d(obs)
    eps = _f32_then_d(eps).reshape(-1, 1)
    h = net.trunk(obs)
    mu, sigma = net.mean(h), _sigma(net.std(h))
    x, action, lp = _draw(mu, sigma, eps, float(max_action))
    return {k: v.reshape(-1) for k, v in (("action", action), ("log_prob", lp), ("x", x), ("mu", mu),
                                           ("sigma", sigma))}


def _cfg(cfg):
    get = (lambda k: cfg[k]) if isinstance(cfg, dict) else (lambda k: getattr(cfg, k))
    return float(get("gamma")), float(get("reward_scale"))


def learn_f64(state_dicts: dict, batch, noise, cfg, max_action: float, grads: bool = True) -> dict:
    """One ``VecSAC.learn(batch, noise)`` at the weights of ``state_dicts`` in float64.

    ``cfg`` gives ``gamma`` and ``reward_scale`` (an AgentConfig or a dict). Returns a dict:
    ``losses`` (value, actor, critic_1, critic_2), ``loss_scale`` (mean |per-row term| of each),
    ``grad`` / ``S`` / ``S_max`` ([net][param]), ``min_abs_z``, ``dq_*``, ``abs_x_*``
    and the per-row ``rows`` terms. ``grads=False`` stops after the forward passes."""
    gamma, scale = _cfg(cfg)
    M = float(max_action)
    state, action, reward, state_, done = batch
    state, action, reward, state_ = (_f32_then_d(t) for t in (state, action, reward, state_))
    B = state.shape[0]
    action, reward = action.reshape(B, 1), reward.reshape(B)
    done = torch.as_tensor(done).detach().to("cpu").to(torch.bool).reshape(B)
    e1, e2 = (_f32_then_d(e).reshape(B, 1) for e in noise)

    tape = _Tape(B)
    net = {n: _Net(n, state_dicts[n], tape) for n in _LAYERS}
    both = lambda s, a: (net["critic_1"].q(net["critic_1"].trunk(torch.cat([s, a], 1))).view(-1),  # noqa: E731
                         net["critic_2"].q(net["critic_2"].trunk(torch.cat([s, a], 1))).view(-1))

    # value loss: 0.5 mse(value(state), min q(state, sample()) - log_prob), target detached
    tape.own = "value"
    value = net["value"].v(net["value"].trunk(state)).view(-1)
    tape.own = "actor"     # one actor forward serves both draws (same weights, same state)
    h = net["actor"].trunk(state)
    mu, sigma = net["actor"].mean(h), _sigma(net["actor"].std(h))
    tape.own = None
    with torch.no_grad():
        value_ = net["target_value"].v(net["target_value"].trunk(state_)).view(-1)
        value_ = torch.where(done, torch.zeros_like(value_), value_)   # value_[done] = 0.0
        x1, a1, lp1 = _draw(mu, sigma, e1, M)                        # sample(): no gradient
        q1s, q2s = both(state, a1)
        value_target = torch.min(q1s, q2s) - lp1.view(-1)
    value_rows = 0.5 * (value - value_target) ** 2

    # actor loss: mean(log_prob - min q) at the rsample() draw
    x2, a2, lp2 = _draw(mu, sigma, e2, M)
    q1r, q2r = both(state, a2)
    actor_rows = lp2.view(-1) - torch.min(q1r, q2r)

    # critic losses: 0.5 mse(q(state, action), reward_scale * reward + gamma * value_)
    q_hat = scale * reward + gamma * value_
    crit_rows = []
    for c in ("critic_1", "critic_2"):
        tape.own = c
        q = net[c].q(net[c].trunk(torch.cat([state, action], 1))).view(-1)
        crit_rows.append(0.5 * (q - q_hat) ** 2)
    tape.own = None

    rows = {"value": value_rows, "actor": actor_rows, "critic_1": crit_rows[0], "critic_2": crit_rows[1]}
    order = ("value", "actor", "critic_1", "critic_2")   # VecSAC.learn's return order
    out = {
        "losses": torch.stack([rows[n].mean() for n in order]).detach(),
        "loss_scale": torch.stack([rows[n].abs().mean() for n in order]).detach(),
        "rows": {n: rows[n].detach() for n in order},
        "min_abs_z": tape.min_abs_z,
        "dq_sample": (q1s - q2s).abs().detach(),
        "dq_rsample": (q1r - q2r).abs().detach(),
        "abs_x_sample": x1.abs().view(-1).detach(),
        "abs_x_rsample": x2.abs().view(-1).detach(),
    }
    if not grads:
        return out
    out["grad"], out["S"], out["S_max"] = {}, {}, {}
    for n in OPTIMISED:
        names = [k for k, _ in net[n].named_parameters()]
        g = torch.autograd.grad(rows[n].mean(), list(net[n].parameters()))
        out["grad"][n] = dict(zip(names, g))
        out["S"][n] = {k: tape.S[n][k].reshape(gk.shape) for k, gk in out["grad"][n].items()}
        out["S_max"][n] = {k: float(s.max()) for k, s in out["S"][n].items()}
    return out


def kink_free_rows(state_dicts: dict, batch, noise, cfg, max_action: float, delta_z: float = 1e-5,
                   delta_q: float | None = 1e-5):
    """(indices of the rows of a candidate batch that are kink-free, rejected share).

    A row is kept when every fc1 / fc2 pre-activation it produces is at least ``delta_z``
    from zero and |q1 - q2| is at least ``delta_q`` at both draws (``delta_q=None``: the
    ``min`` margin is not asked for, as when the two critics are equal on purpose)."""
    f = learn_f64(state_dicts, batch, noise, cfg, max_action, grads=False)
    ok = f["min_abs_z"] >= delta_z
    if delta_q is not None:
        ok &= (f["dq_sample"] >= delta_q) & (f["dq_rsample"] >= delta_q)
    return torch.nonzero(ok).view(-1), 1.0 - float(ok.double().mean())


__all__ = ["policy_f64", "learn_f64", "kink_free_rows", "OPTIMISED"]
