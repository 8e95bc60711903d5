"""The SAC agent on the fp32 MFMA kernels of sacenv_sac.hip.

``NativeSAC`` has ``VecSAC``'s surface (sacenv/agent.py: ``choose_action``,
``learn(batch, noise)``, ``update_network_parameters``, ``state_dicts``, the five
``nn.Module`` attributes, a ``DeviceReplayBuffer`` as ``memory``), but
``choose_action`` is one ``sacenv_sac_act`` launch and ``learn`` is one
``sacenv_sac_learn`` call (four launches): ContinuousAgent.learn
(agent/continuous_agent.py:96-154) with all five networks, the four Adam
states (torch.optim.Adam, continuous_agent.py / networks.py:29-31 defaults)
and the target soft update in one device weights buffer.

The modules' parameters are views of that buffer (``SlabNets``), so ``state_dict()`` and the
reference's checkpoint format see the live weights; a host write into them
must be followed by ``sync()`` (the kernels keep a transposed copy of each
256x256 layer). Initial weights are the reference agent's for the same
``init_seed`` (the nets are built as VecSAC builds them).

``_SacCore`` is what the one agent shares with ``NativeSACPopulation`` (sacenv/population.py):
everything in front of a launch, over a leading member axis.

There is no CPU path: without libsacenv.so or a GPU this class raises.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from .agent import AgentConfig, VecSAC, load_models, save_models
from .noise import ACT, LEARN1, LEARN2, PolicyNoise

# torch parameter names per net, in the C layout's tensor order (w1, b1, w2, b2, head 0, head 1)
_TENSORS = {
    "actor": ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "mean.weight", "mean.bias",
              "std.weight", "std.bias"),
    "critic": ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "q.weight", "q.bias"),
    "value": ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "v.weight", "v.bias"),
}
_SHAPE = {"actor": 0, "critic_1": 1, "critic_2": 1, "value": 2, "target_value": 2}
_KIND = {"actor": "actor", "critic_1": "critic", "critic_2": "critic", "value": "value",
         "target_value": "value"}


def _shape(*dims) -> str:
    return "[" + ", ".join(map(str, dims)) + "]"


class SlabNets:
    """The five ``nn.Module``s of one agent, their parameters views of its weights slab
    (``slab``: f32 ``[>= layout.total_floats]``, laid out by ``sacenv_sac_layout``).

    The nets are built as ``VecSAC`` builds them under ``init_seed`` (from torch's global CPU
    generator without one); ``build`` copies those initial weights into the slab, else the slab
    keeps what it holds. ``NativeSAC`` and ``PopulationMember`` are ``SlabNets`` with counters;
    on its own (``MemberScoreboard``: a snapshot's slab) it is at step 0 with no noise seed."""

    NETS = VecSAC.NETS
    adam_step = act_calls = 0
    noise_seed = None

    def __init__(self, slab, params, layout, cfg, device, init_seed, build: bool):
        self.weights, self.params, self.layout, self.cfg = slab, params, layout, cfg
        ref = VecSAC("cpu", cfg, obs_dim=params.obs_dim, n_actions=1, max_action=params.max_action,
                     init_seed=init_seed, with_memory=False)
        for i, name in enumerate(self.NETS):
            mod = getattr(ref, name)
            for dotted, view in self._views(layout.net[i], name).items():
                if build:  # the reference's initial weights
                    view.copy_(mod.state_dict()[dotted].reshape(view.shape))
                sub, pname = dotted.split(".")
                setattr(getattr(mod, sub), pname, nn.Parameter(view, requires_grad=False))
            setattr(self, name, mod.to(device))

    def _views(self, base: int, name: str) -> dict:
        """Net ``name``'s tensors as views of the slab, for the copy of the net at ``base``
        (the parameters, or one of the Adam moments)."""
        s, kind = _SHAPE[name], _KIND[name]
        ins = {"actor": self.params.obs_dim, "critic": self.params.obs_dim + 1,
               "value": self.params.obs_dim}[kind]
        H = _lib.SAC_HIDDEN
        shapes = ((H, ins), (H,), (H, H), (H,), (1, H), (1,), (1, H), (1,))
        out = {}
        for k, pname in enumerate(_TENSORS[kind]):
            off = base + self.layout.tensor[s][k]
            n = 1
            for d in shapes[k]:
                n *= d
            out[pname] = self.weights[off: off + n].view(*shapes[k])
        return out

    def adam_state(self, name: str) -> dict:
        """exp_avg / exp_avg_sq views of an optimised net (as torch.optim.Adam's state)."""
        i = self.NETS.index(name)
        if i > 3:
            raise KeyError(name)
        return {"exp_avg": self._views(self.layout.adam_m[i], name),
                "exp_avg_sq": self._views(self.layout.adam_v[i], name)}

    def state_dicts(self) -> dict:
        return {n: getattr(self, n).state_dict() for n in self.NETS}

    def optimizer_state(self) -> dict:
        """The Adam moments of the four optimised nets and the step count (CPU copies)."""
        out = {"step": torch.tensor(self.adam_step, dtype=torch.int64)}
        if self.noise_seed is not None:  # the act draw's call count: a resumed agent draws on
            out["act_calls"] = torch.tensor(self.act_calls, dtype=torch.int64)
        for n in self.NETS[:4]:
            for which, views in self.adam_state(n).items():
                out.update({f"{n}.{which}.{k}": v.detach().cpu().clone() for k, v in views.items()})
        return out

    def load_optimizer_state(self, state: dict) -> None:
        """The moments into the slab; the owner of the counters takes ``step`` and ``act_calls``."""
        for n in self.NETS[:4]:
            for which, views in self.adam_state(n).items():
                for k, v in views.items():
                    v.copy_(state[f"{n}.{which}.{k}"].reshape(v.shape))


class _SacCore:
    """What ``NativeSAC`` and ``NativeSACPopulation`` share: ``lead`` agents -- ``()``: the one,
    ``(P,)``: a population's -- in one ``[*lead, floats]`` weights buffer, acting and learning in
    one set of launches. Every input and output has ``lead`` in front of the one agent's shape.

    A subclass sizes the buffers (``_sizes``), binds its entry points (``_sync``, ``_act``,
    ``_learn`` and the arguments in front of the weights pointer, ``_head`` / ``_learn_head``:
    resolved once, a ctypes lookup per call is measurable) and samples its own replay memory
    (``_sample``)."""

    def __init__(self, lead: tuple, cfg: AgentConfig, device, obs_dim: int, n_actions: int, max_action: float,
                 adam_eps: float, noise_seeds):
        if cfg.layer1_size != _lib.SAC_HIDDEN or cfg.layer2_size != _lib.SAC_HIDDEN:
            raise ValueError(f"the SAC kernels are built for {_lib.SAC_HIDDEN}-wide layers")
        if n_actions != 1:
            raise ValueError("the SAC kernels take one action dimension (the boat's)")
        self.device = _lib.cuda_device(device, type(self).__name__)
        self.lead, self._k, self._agents = lead, len(lead), lead[0] if lead else 1
        # lr_*, gamma, tau and reward_scale are one agent's: a population's entry points take its
        # members' from their own table and do not read these
        self.params = _lib.SacParams(
            obs_dim=obs_dim, n_actions=1, hidden=_lib.SAC_HIDDEN, batch=cfg.batch_size,
            max_action=float(max_action), gamma=cfg.gamma, tau=cfg.tau,
            reward_scale=cfg.reward_scale, lr_actor=cfg.lr_alpha, lr_critic=cfg.lr_beta,
            adam_beta1=0.9, adam_beta2=0.999, adam_eps=float(adam_eps))
        self._pp = C.byref(self.params)
        self._B, self._D = int(cfg.batch_size), int(obs_dim)   # (a ctypes field costs more than an attribute)
        self.layout = _lib.sac_layout(self.params)             # inside one agent's slab
        floats, scratch_bytes = self._sizes()
        self.weights = torch.zeros((*lead, floats), dtype=torch.float32, device=self.device)
        self.scratch = torch.empty(scratch_bytes // 4, dtype=torch.float32, device=self.device)
        self.losses = torch.zeros((*lead, 4), dtype=torch.float32, device=self.device)
        # one step and one act count for all agents. Counter-based policy noise (sacenv/noise.py),
        # one seed per agent: the draws of choose_action and learn are a function of (seed,
        # act_calls / adam_step) alone; without seeds, torch's device stream
        self.adam_step = self.act_calls = 0
        self.noise = None if noise_seeds is None else PolicyNoise(noise_seeds, self.device)

    def _stream(self):
        return _lib.stream_handle(self.device)

    def sync(self) -> None:
        """Refresh the kernels' transposed 256x256 layers after a host write to the weights."""
        _lib.check(self._sync(*self._head, self.weights.data_ptr(), self._stream()))

    def _f32(self, x, n: int, what: str):
        """f32, contiguous, on the device: ``n`` values, the member axis (if any) first."""
        t = torch.as_tensor(x, device=self.device).to(torch.float32).contiguous()
        if t.numel() != n or (self._k and t.shape[0] != self._agents):
            raise ValueError(f"{what} must hold {n} values as {_shape(*self.lead, '...')}, got {list(t.shape)}")
        return t

    @torch.no_grad()
    def choose_action(self, obs, eps=None):
        """``[*lead, n, obs_dim] -> [*lead, n, 1]`` (continuous_agent.py:57-61): every agent acts
        on its own n rows, one launch. ``eps``: the n standard normal draws per agent."""
        obs = torch.as_tensor(obs, device=self.device).to(torch.float32).contiguous()
        k, lead = self._k, self.lead
        if obs.dim() != k + 2 or (k and obs.shape[0] != self._agents) or obs.shape[-1] != self._D:
            raise ValueError(f"obs must be {_shape(*lead, 'n', self._D)}, got {list(obs.shape)}")
        n = obs.shape[k]
        if eps is not None:
            eps = self._f32(eps, self._agents * n, "eps")
        elif self.noise is not None:
            eps = self.noise.normal(ACT, self.act_calls, n)    # [1, agents, n]: [*lead, n] as it lies
        else:
            eps = torch.randn((*lead, n), device=self.device)
        out = torch.empty((*lead, n, 1), dtype=torch.float32, device=self.device)
        _lib.check(self._act(*self._head, self.weights.data_ptr(), obs.data_ptr(), n, eps.data_ptr(),
                             out.data_ptr(), None, self._stream()))
        self.act_calls += 1  # every accepted call is one act, wherever its eps came from
        return out

    def noise_for_step(self, n: int):
        """``(eps [*lead, n], (e1, e2) [*lead, B] each)``: what the next ``choose_action`` on n
        rows per agent and the next ``learn`` would draw, from one launch; changes no state (pass
        them as ``eps=`` and ``noise=``)."""
        if self.noise is None:
            raise RuntimeError("noise_for_step needs noise seeds (noise_seed= / noise_seeds=)")
        B, lead = self._B, self.lead
        eps, e1, e2 = self.noise.draw([(ACT, self.act_calls, n), (LEARN1, self.adam_step, B),
                                       (LEARN2, self.adam_step, B)])
        return eps.view(*lead, n), (e1.view(*lead, B), e2.view(*lead, B))

    def act_noise(self, K: int, n: int) -> torch.Tensor:
        """f32 ``[K, *lead, n]``: row k is what the k-th ``choose_action`` from now would draw
        (the table ``ClosedLoop.run`` takes); changes no state."""
        if self.noise is None:
            raise RuntimeError("act_noise needs noise seeds (noise_seed= / noise_seeds=)")
        return self.noise.normal(ACT, self.act_calls, n, calls=K).view(K, *self.lead, n)

    _learn_weighted = None   # the entry point of sacenv_weighted_learn.h, bound at the first weighted learn

    def _row_weights(self, weights):
        """``weights`` as the kernels read them; the shape is checked before a device is touched."""
        want = (*self.lead, self._B)
        shape = tuple(getattr(weights, "shape", None) or torch.as_tensor(weights).shape)
        if shape != want:
            raise ValueError(f"weights must be {_shape(*want)}, got {list(shape)}")
        if self._learn_weighted is None:
            self._learn_weighted = _lib.weighted_learn_fn(self._learn_weighted_name)
        return self._f32(weights, self._agents * self._B, "weights")

    @torch.no_grad()
    def learn(self, batch=None, noise=None, *, weights=None, losses: bool = True):
        """continuous_agent.py:96-154 as VecSAC.learn, for every agent. ``batch`` = (state
        ``[*lead, B, D]``, action ``[*lead, B(, 1)]``, reward ``[*lead, B]``, new_state, done);
        else the agents' own replay memory is sampled (None while it holds < B rows). ``noise``
        = (eps1, eps2), each ``[*lead, B(, 1)]``. ``weights``: f32 ``[*lead, B]``, a weight per
        batch row on the critics' TD loss (include/sacenv_weighted_learn.h: the importance weights
        of a prioritized sample; the per-row squared TD errors in the scratch stay raw); ``None``
        is the unweighted call. Returns the (value, actor, critic 1, critic 2)
        losses as independent tensors -- the one agent's as four device scalars, a population's
        as ``[P, 4]`` -- or with ``losses=False`` the f32 ``[*lead, 4]`` loss buffer itself (no
        copy launch: the next learn() rewrites it)."""
        if weights is not None:
            weights = self._row_weights(weights)
        B, k = self._B, self._k
        if batch is None:
            batch = self._sample()
            if batch is None:
                return None
        state, action, reward, state_, done = batch
        rows = self._agents * B
        state = self._f32(state, rows * self._D, "state")
        state_ = self._f32(state_, rows * self._D, "new_state")
        action = self._f32(action, rows, "action")
        reward = torch.as_tensor(reward, device=self.device).to(torch.float64).contiguous()
        done = torch.as_tensor(done, device=self.device).to(torch.uint8).contiguous()
        if reward.numel() != rows or done.numel() != rows or (
                k and not reward.shape[0] == done.shape[0] == self._agents):
            raise ValueError(f"reward and done must be {_shape(*self.lead, B)}, got {list(reward.shape)} and "
                             f"{list(done.shape)}")
        if noise is not None:
            e1, e2 = self._f32(noise[0], rows, "noise[0]"), self._f32(noise[1], rows, "noise[1]")
        elif self.noise is not None:   # [1, agents, B] each: [*lead, B] as they lie
            e1, e2 = self.noise.draw([(LEARN1, self.adam_step, B), (LEARN2, self.adam_step, B)])
        else:
            e1, e2 = torch.randn((*self.lead, B), device=self.device), torch.randn((*self.lead, B), device=self.device)
        step = self.adam_step + 1  # committed only once the call is accepted
        if weights is None:
            _lib.check(self._learn(
                *self._learn_head, self.weights.data_ptr(), self.scratch.data_ptr(), state.data_ptr(),
                action.data_ptr(), reward.data_ptr(), state_.data_ptr(), done.data_ptr(), e1.data_ptr(),
                e2.data_ptr(), step, self.losses.data_ptr(), self._stream()))
        else:
            _lib.check(self._learn_weighted(
                *self._learn_head, self.weights.data_ptr(), self.scratch.data_ptr(), state.data_ptr(),
                action.data_ptr(), reward.data_ptr(), state_.data_ptr(), done.data_ptr(), e1.data_ptr(),
                e2.data_ptr(), step, self.losses.data_ptr(), weights.data_ptr(), self._stream()))
        self.adam_step = step
        if not losses:
            return self.losses
        out = self.losses.clone()
        return out if k else tuple(out.unbind(0))


class NativeSAC(_SacCore, SlabNets):
    """ContinuousAgent (continuous_agent.py:9-154) on libsacenv's SAC kernels."""

    _learn_weighted_name = "sacenv_sac_learn_weighted"

    def __init__(self, device, config=None, *, obs_dim: int = 11, n_actions: int = 1,
                 max_action: float = 1.0, init_seed: int | None = None, buffer_seed: int = 0,
                 with_memory: bool = True, adam_eps: float = 1e-8, noise_seed: int | None = None):
        cfg = AgentConfig.from_any(config)
        _SacCore.__init__(self, (), cfg, device, obs_dim, n_actions, max_action, adam_eps,
                          None if noise_seed is None else [noise_seed])
        self.noise_seed = None if noise_seed is None else int(noise_seed)
        lib = _lib.load()
        self._sync, self._act, self._learn = lib.sacenv_sac_sync, lib.sacenv_sac_act, lib.sacenv_sac_learn
        self._head = self._learn_head = (self._pp,)
        SlabNets.__init__(self, self.weights, self.params, self.layout, cfg, self.device, init_seed, True)
        self.sync()
        self.memory = None
        if with_memory:
            from .replay import DeviceReplayBuffer
            self.memory = DeviceReplayBuffer(cfg.max_size, (obs_dim,), n_actions, device=self.device,
                                             seed=buffer_seed)

    @classmethod
    def from_slab(cls, device, cfg, slab, *, obs_dim: int, max_action: float, adam_eps: float, noise_seed,
                  adam_step: int = 0, act_calls: int = 0) -> "NativeSAC":
        """A stand-alone agent (no memory) with a copy of ``slab`` -- a member's row of a
        population's weights, or of a snapshot of them -- as its weights, Adam moments and kernel
        copies, at the given step and act count."""
        agent = cls(device, cfg, obs_dim=obs_dim, max_action=max_action, with_memory=False, adam_eps=adam_eps,
                    noise_seed=noise_seed)
        agent.weights.copy_(slab[: agent.weights.numel()])
        agent.adam_step, agent.act_calls = adam_step, act_calls
        return agent

    def _sizes(self):
        return self.layout.total_floats, self.layout.scratch_bytes

    def _sample(self):
        if self.memory is None or self.memory.mem_cntr < self._B:
            return None
        return self.memory.sample(self._B, as_bool=False)[:5]

    @torch.no_grad()
    def update_network_parameters(self, tau=None):
        """continuous_agent.py:63-77 (learn() applies it in-kernel)."""
        tau = self.cfg.tau if tau is None else tau
        for tp, p in zip(self.target_value.parameters(), self.value.parameters()):
            tp.copy_(tau * p.clone() + (1 - tau) * tp.clone())
        # the target's fc2.weight has a kernel copy in fragment order (role_critic_loss
        # reads it): refresh it, or the next learn() would use the stale target
        self.sync()

    @torch.no_grad()
    def choose_action_handoff(self, obs, eps, out, *, obs_ready, obs_want: int, act_ready, act_value: int,
                              status=None) -> None:
        """``choose_action`` as the producer of a closed loop with ``VecBoatEnv.segment_async``
        (``sacenv_sac_act_handoff``): the 64 rows of block b (owner wave b's envs) are read once
        ``obs_ready[b] >= obs_want`` and ``act_ready[b] = act_value`` is published once their
        actions in ``out`` (f32 [N], device) are visible. Enqueued on the current stream."""
        n = obs.shape[0]
        if obs.dtype != torch.float32 or not obs.is_contiguous() or obs.shape[1] != self.params.obs_dim:
            raise ValueError(f"obs must be a contiguous float32 [N, {self.params.obs_dim}] tensor")
        for name, t, cnt in (("eps", eps, n), ("out", out, n)):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != cnt or t.device != self.device:
                raise ValueError(f"{name} must be a contiguous float32 device tensor of {cnt} values")
        _lib.check(_lib.load().sacenv_sac_act_handoff(
            self._pp, self.weights.data_ptr(), obs.data_ptr(), n, eps.data_ptr(), out.data_ptr(),
            obs_ready.data_ptr(), int(obs_want), act_ready.data_ptr(), int(act_value),
            None if status is None else status.data_ptr(), self._stream()))

    def load_optimizer_state(self, state: dict) -> None:
        super().load_optimizer_state(state)
        self.adam_step = int(state["step"])
        if self.noise_seed is not None and "act_calls" in state:
            self.act_calls = int(state["act_calls"])

    def save_models(self, experiment_dir: str, optimizer: bool = False) -> None:
        """ContinuousAgent.save_models (continuous_agent.py:79-84), the reference's files."""
        save_models(self, experiment_dir, optimizer)

    def load_models(self, experiment_dir: str, optimizer: bool = False) -> None:
        """ContinuousAgent.load_models (continuous_agent.py:86-91): the parameters are views
        of the weights buffer, so load_state_dict writes it in place; then sync()."""
        load_models(self, experiment_dir, optimizer)


__all__ = ["NativeSAC", "SlabNets"]
