"""A population of SAC agents on the kernels of sacenv_sac_pop.hip: the agent side of the
reference's hyper-parameter search (``main.py -p N``, main.py:215-235).

The search trains N agents that differ in the actor and critic learning rates, gamma and
tau (utils/hyperparameter_tuner.py:20-43, ranges in configs/hp_configs.yaml), three OS
processes at a time. ``NativeSACPopulation`` holds P such agents in one weights buffer
(``[P, member_floats]``, each row laid out as one ``NativeSAC``'s) and runs them in lockstep:
``choose_action`` is one launch and ``learn`` four, for all members (include/
sacenv_population.h). Member m computes what a ``NativeSAC`` with member m's config computes,
bit for bit (tests/test_sac_population_gpu.py); ``export_member`` / ``from_agents`` move
members in and out.

``sample_hpsets`` restates the reference's draw rule. There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import random
from dataclasses import dataclass

import torch

from . import _lib
from .agent import AgentConfig, VecSAC, load_models, save_models
from .noise import ACT, LEARN1, LEARN2, PolicyNoise
from .sac_native import NativeSAC, _set_param

_COMMON = ("batch_size", "layer1_size", "layer2_size", "max_size")


@dataclass(frozen=True)
class HPRanges:
    """configs/hp_configs.yaml (agent section): the ranges the search draws from."""
    alpha_min: float = 0.001
    alpha_max: float = 0.01
    beta_min: float = 0.0008
    beta_max: float = 0.008
    gamma_min: float = 0.95
    gamma_max: float = 0.99
    tau_min: float = 0.001
    tau_max: float = 0.01


def sample_hpsets(P: int, seed, ranges: HPRanges = HPRanges(), base=None) -> list:
    """P ``AgentConfig``s as HPTuner draws them (hyperparameter_tuner.py:12-43): per member, in
    the order alpha, beta, gamma, tau, ``round(rng.uniform(lo, hi), 4)`` from one
    ``random.Random(seed)``; every other field from ``base``."""
    rng = random.Random(seed)
    base = AgentConfig.from_any(base)
    out = []
    for _ in range(int(P)):
        alpha = round(rng.uniform(ranges.alpha_min, ranges.alpha_max), 4)
        beta = round(rng.uniform(ranges.beta_min, ranges.beta_max), 4)
        gamma = round(rng.uniform(ranges.gamma_min, ranges.gamma_max), 4)
        tau = round(rng.uniform(ranges.tau_min, ranges.tau_max), 4)
        out.append(dataclasses.replace(base, lr_alpha=alpha, lr_beta=beta, gamma=gamma, tau=tau))
    return out


def _common_configs(configs) -> list:
    cfgs = [AgentConfig.from_any(c) for c in configs]
    if not cfgs:
        raise ValueError("a population needs at least one member")
    for f in _COMMON:
        vals = {getattr(c, f) for c in cfgs}
        if len(vals) != 1:
            raise ValueError(f"{f} must agree across the members of a population, got {sorted(vals)}")
    return cfgs


class PopulationMember:
    """Member m: the five ``nn.Module``s on views of its slab, as ``NativeSAC`` has them."""

    NETS = NativeSAC.NETS
    _views = NativeSAC._views
    adam_state = NativeSAC.adam_state
    state_dicts = NativeSAC.state_dicts
    optimizer_state = NativeSAC.optimizer_state

    def __init__(self, pop, m: int, cfg: AgentConfig, init_seed, build: bool):
        self.population, self.index, self.cfg = pop, m, cfg
        self.params, self.layout = pop.params, pop.layout
        self.weights = pop.weights[m]
        ref = VecSAC("cpu", cfg, obs_dim=pop.params.obs_dim, n_actions=1, max_action=pop.params.max_action,
                     init_seed=init_seed, with_memory=False)
        for i, name in enumerate(self.NETS):
            mod = getattr(ref, name)
            for pname, view in self._views(self.weights, self.layout.net[i], name).items():
                if build:  # the reference's initial weights under init_seed (NativeSAC.__init__)
                    view.copy_(mod.state_dict()[pname].reshape(view.shape))
                _set_param(mod, pname, view)
            setattr(self, name, mod.to(pop.device))

    @property
    def adam_step(self) -> int:
        return self.population.adam_step

    @property
    def act_calls(self) -> int:
        return self.population.act_calls

    @property
    def noise_seed(self):
        seeds = self.population.noise_seeds
        return None if seeds is None else seeds[self.index]

    def load_optimizer_state(self, state: dict) -> None:
        for n in self.NETS[:4]:
            for which, views in self.adam_state(n).items():
                for k, v in views.items():
                    v.copy_(state[f"{n}.{which}.{k}"].reshape(v.shape))
        self.loaded_step = int(state["step"])  # the population commits it (one step for all members)
        self.loaded_act_calls = int(state["act_calls"]) if "act_calls" in state else None

    def hpset(self) -> dict:
        """The four searched values under the reference's config keys (tuned_configs.yaml)."""
        c = self.cfg
        return {"learning_rate_alpha": c.lr_alpha, "learning_rate_beta": c.lr_beta, "gamma": c.gamma,
                "tvn_parameter_modulation_tau": c.tau}


class NativeSACPopulation:
    """P ``NativeSAC`` agents learning in lockstep, in one set of launches."""

    def __init__(self, device, configs, *, obs_dim: int = 11, max_action: float = 1.0, init_seeds=None,
                 buffer_seeds=None, with_memory: bool = True, adam_eps: float = 1e-8, replay=None,
                 noise_seeds=None, _build: bool = True):
        cfgs = _common_configs(configs)
        P = self.P = len(cfgs)
        cfg = cfgs[0]
        if cfg.layer1_size != _lib.SAC_HIDDEN or cfg.layer2_size != _lib.SAC_HIDDEN:
            raise ValueError(f"the SAC kernels are built for {_lib.SAC_HIDDEN}-wide layers")
        if P > _lib.POPULATION_MAX_MEMBERS:
            raise ValueError(f"a population holds at most {_lib.POPULATION_MAX_MEMBERS} members, got {P}")
        for name, seeds in (("init_seeds", init_seeds), ("buffer_seeds", buffer_seeds),
                            ("noise_seeds", noise_seeds)):
            if seeds is not None and len(seeds) != P:
                raise ValueError(f"{name} must hold one seed per member")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.SacenvError("NativeSACPopulation runs on the GPU only (libsacenv SAC kernels)")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        if replay is not None:
            # one PopulationReplay for all members (sacenv/population_replay.py): checked before
            # anything is built or launched
            from .population_replay import PopulationReplay
            if not isinstance(replay, PopulationReplay):
                raise TypeError("replay must be a PopulationReplay")
            for what, have, want in (("members", replay.P, P), ("max_size", replay.mem_size, cfg.max_size),
                                     ("obs_dim", replay.params.obs_dim, obs_dim), ("n_actions", replay.n_actions, 1),
                                     ("device", replay.device, self.device)):
                if have != want:
                    raise ValueError(f"the replay's {what} ({have}) must be the population's ({want})")
        self.configs = cfgs
        # the fields the members share; lr_*, gamma, tau and reward_scale here are member 0's and
        # are not read by the population entry points (they take self._hp)
        self.params = _lib.SacParams(
            obs_dim=obs_dim, n_actions=1, hidden=_lib.SAC_HIDDEN, batch=cfg.batch_size,
            max_action=float(max_action), gamma=cfg.gamma, tau=cfg.tau, reward_scale=cfg.reward_scale,
            lr_actor=cfg.lr_alpha, lr_critic=cfg.lr_beta, adam_beta1=0.9, adam_beta2=0.999,
            adam_eps=float(adam_eps))
        self._hp = (_lib.SacMember * P)(*[
            _lib.SacMember(lr_actor=c.lr_alpha, lr_critic=c.lr_beta, gamma=c.gamma, tau=c.tau,
                           reward_scale=c.reward_scale) for c in cfgs])
        self.layout = _lib.sac_layout(self.params)          # inside a member's slab
        PL = self.pop_layout = _lib.sac_pop_layout(self.params, P)
        self.weights = torch.zeros((P, PL.member_floats), dtype=torch.float32, device=self.device)
        self.scratch = torch.empty(PL.total_scratch_bytes // 4, dtype=torch.float32, device=self.device)
        self.losses = torch.zeros((P, 4), dtype=torch.float32, device=self.device)
        self.adam_step = 0
        # counter-based policy noise (sacenv/noise.py), one seed per member: member m draws what a
        # NativeSAC(noise_seed=noise_seeds[m]) draws; one act_calls for all, as one adam_step
        self.noise_seeds = None if noise_seeds is None else tuple(int(s) for s in noise_seeds)
        self.noise = None
        if noise_seeds is not None:
            self.noise = PolicyNoise(self.noise_seeds, self.device)
        self.act_calls = 0
        self.members = [PopulationMember(self, m, cfgs[m], None if init_seeds is None else init_seeds[m], _build)
                        for m in range(P)]
        if _build:
            self.sync()
        self.memory = None
        self._pop_replay = replay is not None
        if replay is not None:
            self.memory = replay
        elif with_memory:
            from .replay import DeviceReplayBuffer
            self.memory = [DeviceReplayBuffer(cfg.max_size, (obs_dim,), 1, device=self.device,
                                              seed=m if buffer_seeds is None else buffer_seeds[m])
                           for m in range(P)]

    def __len__(self) -> int:
        return self.P

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _native(self):
        lib = _lib.load()
        if not hasattr(lib, "sacenv_sac_pop_learn"):
            raise _lib.SacenvError("this libsacenv.so was built before sacenv_population.h")
        return lib

    def sync(self) -> None:
        """Refresh every member's kernel copies of the 256x256 layers after a host write."""
        _lib.check(self._native().sacenv_sac_pop_sync(C.byref(self.params), self.P, self.weights.data_ptr(),
                                                   self._stream()))

    def _f32(self, x, n, what):
        """f32, contiguous, on the device; ``n`` values with the member axis first."""
        t = torch.as_tensor(x, device=self.device).to(torch.float32).contiguous()
        if t.numel() != n or t.shape[0] != self.P:
            raise ValueError(f"{what} must hold {n} values as [{self.P}, ...], got {list(t.shape)}")
        return t

    @torch.no_grad()
    def choose_action(self, obs, eps=None):
        """[P, n, obs_dim] -> [P, n, 1]: member m acts on its own n rows, one launch."""
        obs = torch.as_tensor(obs, device=self.device).to(torch.float32).contiguous()
        D = self.params.obs_dim
        if obs.dim() != 3 or obs.shape[0] != self.P or obs.shape[2] != D:
            raise ValueError(f"obs must be [{self.P}, n, {D}], got {list(obs.shape)}")
        n = obs.shape[1]
        if eps is not None:
            eps = self._f32(eps, self.P * n, "eps")
        elif self.noise is not None:
            eps = self.noise.normal(ACT, self.act_calls, n)[0]
        else:
            eps = torch.randn((self.P, n), device=self.device)
        out = torch.empty((self.P, n, 1), dtype=torch.float32, device=self.device)
        _lib.check(self._native().sacenv_sac_pop_act(C.byref(self.params), self.P, self.weights.data_ptr(),
                                                  obs.data_ptr(), n, eps.data_ptr(), out.data_ptr(), None,
                                                  self._stream()))
        self.act_calls += 1  # every accepted call is one act, wherever its eps came from
        return out

    def noise_for_step(self, n: int):
        """``(eps [P, n], (e1, e2) [P, B] each)``: what the next ``choose_action`` on n rows per
        member and the next ``learn`` would draw, from one launch; changes no state."""
        if self.noise is None:
            raise RuntimeError("noise_for_step needs a population built with noise_seeds")
        B = self.configs[0].batch_size
        eps, e1, e2 = self.noise.draw([(ACT, self.act_calls, n), (LEARN1, self.adam_step, B),
                                       (LEARN2, self.adam_step, B)])
        return eps[0], (e1[0], e2[0])

    def act_noise(self, K: int, n: int) -> torch.Tensor:
        """f32 [K, P, n]: row k is what the k-th ``choose_action`` from now would draw; changes
        no state."""
        if self.noise is None:
            raise RuntimeError("act_noise needs a population built with noise_seeds")
        return self.noise.normal(ACT, self.act_calls, n, calls=K)

    def remember(self, m: int, state, action, reward, new_state, code, **kw) -> None:
        """``memory[m].store_batch``: member m's transitions. (With a ``PopulationReplay`` the
        members store in lockstep, through the replay itself.)"""
        if self._pop_replay:
            raise TypeError("this population holds a PopulationReplay, whose members store in lockstep: use "
                            "memory.store_batch / memory.store_env_step for all members at once")
        self.memory[m].store_batch(state, action, reward, new_state, code, **kw)

    store_batch = remember

    def sample(self):
        """One batch per member from its own buffer, as ``learn`` takes them: stacked, or with a
        ``PopulationReplay`` as its two launches write them."""
        B = self.configs[0].batch_size
        if self._pop_replay:
            return self.memory.sample(B, as_bool=False)[:5]
        rows = [mem.sample(B, as_bool=False)[:5] for mem in self.memory]
        return tuple(torch.stack([r[k] for r in rows]) for k in range(5))

    @torch.no_grad()
    def learn(self, batch=None, noise=None, *, losses: bool = True):
        """``NativeSAC.learn`` for every member. ``batch`` = stacked (state [P, B, D], action
        [P, B, 1], reward [P, B], new_state, done); else each member's own buffer is sampled
        (None until every buffer holds B rows; a ``PopulationReplay`` given as ``replay=`` is
        sampled in two launches, with no stacking). ``noise`` = (eps1, eps2), each [P, B(, 1)].
        Returns a [P, 4] tensor of (value, actor, critic 1, critic 2) losses: a copy, or with
        ``losses=False`` the population's own buffer, which the next learn() rewrites."""
        P, B, D = self.P, self.configs[0].batch_size, self.params.obs_dim
        if batch is None:
            if self.memory is None:
                return None
            if self.memory.mem_cntr < B if self._pop_replay else any(mem.mem_cntr < B for mem in self.memory):
                return None
            batch = self.sample()
        state, action, reward, state_, done = batch
        state = self._f32(state, P * B * D, "state")
        state_ = self._f32(state_, P * B * D, "new_state")
        action = self._f32(action, P * B, "action")
        reward = torch.as_tensor(reward, device=self.device).to(torch.float64).contiguous()
        done = torch.as_tensor(done, device=self.device).to(torch.uint8).contiguous()
        if reward.numel() != P * B or reward.shape[0] != P or done.numel() != P * B or done.shape[0] != P:
            raise ValueError(f"reward and done must be [{P}, {B}], got {list(reward.shape)} and {list(done.shape)}")
        if noise is not None:
            e1, e2 = self._f32(noise[0], P * B, "noise[0]"), self._f32(noise[1], P * B, "noise[1]")
        elif self.noise is not None:
            e1, e2 = (t[0] for t in self.noise.draw([(LEARN1, self.adam_step, B), (LEARN2, self.adam_step, B)]))
        else:
            e1, e2 = torch.randn((P, B), device=self.device), torch.randn((P, B), device=self.device)
        step = self.adam_step + 1  # committed only once the call is accepted
        _lib.check(self._native().sacenv_sac_pop_learn(
            C.byref(self.params), P, self._hp, self.weights.data_ptr(), self.scratch.data_ptr(),
            state.data_ptr(), action.data_ptr(), reward.data_ptr(), state_.data_ptr(), done.data_ptr(),
            e1.data_ptr(), e2.data_ptr(), step, self.losses.data_ptr(), self._stream()))
        self.adam_step = step
        return self.losses.clone() if losses else self.losses

    # ---- members in and out

    def export_member(self, m: int) -> NativeSAC:
        """A stand-alone ``NativeSAC`` with member m's weights, Adam moments, step, noise seed and
        act count (a copy)."""
        agent = NativeSAC(self.device, self.configs[m], obs_dim=self.params.obs_dim,
                          max_action=self.params.max_action, with_memory=False, adam_eps=self.params.adam_eps,
                          noise_seed=None if self.noise_seeds is None else self.noise_seeds[m])
        agent.weights.copy_(self.weights[m, : agent.weights.numel()])
        agent.adam_step = self.adam_step
        agent.act_calls = self.act_calls
        return agent

    @classmethod
    def from_agents(cls, agents, *, with_memory: bool = False, buffer_seeds=None) -> "NativeSACPopulation":
        """The population whose member m is a copy of ``agents[m]`` (weights, Adam moments, step,
        noise seed). The agents must agree in everything the members share, in their step, and --
        seeded agents (all or none) -- in their act count."""
        agents = list(agents)
        if not agents:
            raise ValueError("a population needs at least one member")
        a0 = agents[0]
        for a in agents[1:]:
            for f in ("obs_dim", "batch", "max_action", "adam_beta1", "adam_beta2", "adam_eps"):
                if getattr(a.params, f) != getattr(a0.params, f):
                    raise ValueError(f"the agents differ in {f}")
            if a.adam_step != a0.adam_step:
                raise ValueError(f"the agents differ in their Adam step ({a.adam_step} != {a0.adam_step})")
            if a.device != a0.device:
                raise ValueError("the agents live on different devices")
            if (a.noise_seed is None) != (a0.noise_seed is None):
                raise ValueError("either every agent has a noise seed or none has")
            if a0.noise_seed is not None and a.act_calls != a0.act_calls:
                raise ValueError(f"the agents differ in their act count ({a.act_calls} != {a0.act_calls})")
        pop = cls(a0.device, [a.cfg for a in agents], obs_dim=a0.params.obs_dim, max_action=a0.params.max_action,
                  with_memory=with_memory, buffer_seeds=buffer_seeds, adam_eps=a0.params.adam_eps,
                  noise_seeds=None if a0.noise_seed is None else [a.noise_seed for a in agents], _build=False)
        for m, a in enumerate(agents):
            pop.weights[m, : a.weights.numel()].copy_(a.weights)
        pop.adam_step = a0.adam_step
        pop.act_calls = a0.act_calls
        return pop

    def state_dicts(self) -> list:
        return [mem.state_dicts() for mem in self.members]

    def save_models(self, experiment_dir: str, optimizer: bool = False) -> None:
        """Each member's checkpoints (the reference's files) under
        ``<experiment_dir>/member_<m>/checkpoints/``: one experiment directory per model, as
        ``-p`` leaves them."""
        for m, mem in enumerate(self.members):
            save_models(mem, os.path.join(experiment_dir, f"member_{m}"), optimizer)

    def load_models(self, experiment_dir: str, optimizer: bool = False) -> None:
        steps, acts = set(), set()
        for m, mem in enumerate(self.members):
            load_models(mem, os.path.join(experiment_dir, f"member_{m}"), optimizer)
            if optimizer:
                steps.add(mem.loaded_step)
                if self.noise_seeds is not None and mem.loaded_act_calls is not None:
                    acts.add(mem.loaded_act_calls)
        if len(steps) > 1:
            raise ValueError(f"the members' checkpoints differ in their Adam step: {sorted(steps)}")
        if len(acts) > 1:
            raise ValueError(f"the members' checkpoints differ in their act count: {sorted(acts)}")
        if steps:
            self.adam_step = steps.pop()
        if acts:
            self.act_calls = acts.pop()
        self.sync()


__all__ = ["HPRanges", "NativeSACPopulation", "PopulationMember", "sample_hpsets"]
