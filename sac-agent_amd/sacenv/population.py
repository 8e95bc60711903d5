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

import dataclasses
import os
import random
from dataclasses import dataclass

import torch

from . import _lib
from .agent import AgentConfig, load_models, save_models
from .sac_native import NativeSAC, SlabNets, _SacCore

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


class PopulationMember(SlabNets):
    """Member m: the five ``nn.Module``s on views of its slab, as ``NativeSAC`` has them; the step,
    the act count and the noise seed are the population's."""

    def __init__(self, pop, m: int, cfg: AgentConfig, init_seed, build: bool):
        self.population, self.index = pop, m
        super().__init__(pop.weights[m], pop.params, pop.layout, cfg, pop.device, init_seed, build)

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
        super().load_optimizer_state(state)
        self.loaded_step = int(state["step"])  # the population commits it (one step for all members)
        self.loaded_act_calls = int(state["act_calls"]) if "act_calls" in state else None

    def hpset(self) -> dict:
        """The four searched values under the reference's config keys (tuned_configs.yaml)."""
        c = self.cfg
        return {"learning_rate_alpha": c.lr_alpha, "learning_rate_beta": c.lr_beta, "gamma": c.gamma,
                "tvn_parameter_modulation_tau": c.tau}


class NativeSACPopulation(_SacCore):
    """P ``NativeSAC`` agents learning in lockstep, in one set of launches: ``_SacCore`` with
    ``lead = (P,)``. ``choose_action``: [P, n, obs_dim] -> [P, n, 1]; ``learn`` takes stacked
    batches (state [P, B, D], ...) or samples each member's own buffer -- P ``DeviceReplayBuffer``s,
    or a ``PopulationReplay`` given as ``replay=`` (two launches, no stacking) -- and returns
    [P, 4] losses. ``pool_rows=K`` (with ``replay=``): K of every member's B rows come from all
    members' rings (include/sacenv_population_share.h); a member still learns once its own ring
    holds B rows, and with K > 0 its weights depend on the other members' rows. With a
    ``PrioritizedPopulationReplay`` as ``replay=`` (sacenv/prioritized.py) a ``learn()`` that sampled
    the replay itself hands the batch's TD errors back to it afterwards; with
    ``importance_weights=True`` such a ``learn()`` also passes the sample's importance weights
    (``memory.last_weights``) as its ``weights=`` (include/sacenv_weighted_learn.h)."""

    _learn_weighted_name = "sacenv_sac_pop_learn_weighted"

    def __init__(self, device, configs, *, obs_dim: int = 11, max_action: float = 1.0, init_seeds=None,
                 buffer_seeds=None, with_memory: bool = True, adam_eps: float = 1e-8, replay=None,
                 noise_seeds=None, pool_rows: int = 0, importance_weights: bool = False, _build: bool = True):
        # the sample's importance weights in the critic loss: only a prioritized replay has them
        # (checked before a device is looked for)
        self.importance_weights = bool(importance_weights)
        if self.importance_weights:
            from .prioritized import PrioritizedPopulationReplay as _Prio
            if not isinstance(replay, _Prio):
                raise ValueError("importance_weights=True needs replay=PrioritizedPopulationReplay(...): "
                                 "no other replay computes them")
        cfgs = self.configs = _common_configs(configs)
        P = self.P = len(cfgs)
        cfg = cfgs[0]
        # rows of every member's batch that learn() draws from all members' rings
        # (PopulationReplay.sample(pool_rows=)): checked before anything is built or launched
        self.pool_rows = int(pool_rows)
        if not 0 <= self.pool_rows <= cfg.batch_size:
            raise ValueError(f"pool_rows must lie in [0, batch_size = {cfg.batch_size}], got {pool_rows}")
        if self.pool_rows and replay is None:
            raise ValueError("pool_rows needs the members' buffers in one arena: give replay=PopulationReplay(...)")
        if P > _lib.POPULATION_MAX_MEMBERS:
            raise ValueError(f"a population holds at most {_lib.POPULATION_MAX_MEMBERS} members, got {P}")
        for name, seeds in (("init_seeds", init_seeds), ("buffer_seeds", buffer_seeds),
                            ("noise_seeds", noise_seeds)):
            if seeds is not None and len(seeds) != P:
                raise ValueError(f"{name} must hold one seed per member")
        device = _lib.cuda_device(device, "NativeSACPopulation")
        if replay is not None:
            # one PopulationReplay for all members (sacenv/population_replay.py): checked before
            # anything is built or launched
            from .population_replay import PopulationReplay
            if not isinstance(replay, PopulationReplay):
                raise TypeError("replay must be a PopulationReplay")
            for what, have, want in (("members", replay.P, P), ("max_size", replay.mem_size, cfg.max_size),
                                     ("obs_dim", replay.params.obs_dim, obs_dim), ("n_actions", replay.n_actions, 1),
                                     ("device", replay.device, device)):
                if have != want:
                    raise ValueError(f"the replay's {what} ({have}) must be the population's ({want})")
        self._sync, self._act, self._learn = _lib.require(_lib.POPULATION_EXPORTS[1:], "sacenv_population.h")
        # one member's noise is what a NativeSAC(noise_seed=noise_seeds[m]) draws
        self.noise_seeds = None if noise_seeds is None else tuple(int(s) for s in noise_seeds)
        super().__init__((P,), cfg, device, obs_dim, 1, max_action, adam_eps, self.noise_seeds)
        self._hp = (_lib.SacMember * P)(*[
            _lib.SacMember(lr_actor=c.lr_alpha, lr_critic=c.lr_beta, gamma=c.gamma, tau=c.tau,
                           reward_scale=c.reward_scale) for c in cfgs])
        self._head, self._learn_head = (self._pp, P), (self._pp, P, self._hp)
        self.members = [PopulationMember(self, m, cfgs[m], None if init_seeds is None else init_seeds[m], _build)
                        for m in range(P)]
        if _build:
            self.sync()
        self.memory = None
        self._pop_replay = replay is not None
        # a PrioritizedPopulationReplay (sacenv/prioritized.py): learn() on its own sample hands the
        # rows' TD errors back to it; with any other replay nothing changes
        from .prioritized import PrioritizedPopulationReplay
        self._prioritized = isinstance(replay, PrioritizedPopulationReplay)
        if self._prioritized and self.pool_rows:
            raise ValueError("a prioritized replay does not pool: pool_rows must be 0")
        if replay is not None:
            self.memory = replay
        elif with_memory:
            from .replay import DeviceReplayBuffer
            self.memory = [DeviceReplayBuffer(cfg.max_size, (obs_dim,), 1, device=self.device,
                                              seed=m if buffer_seeds is None else buffer_seeds[m])
                           for m in range(P)]

    def __len__(self) -> int:
        return self.P

    def _sizes(self):
        PL = self.pop_layout = _lib.sac_pop_layout(self.params, self.P)   # (self.layout: inside a member's slab)
        return PL.member_floats, PL.total_scratch_bytes

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
        if self._pop_replay:
            return self.memory.sample(self._B, as_bool=False, pool_rows=self.pool_rows)[:5]
        rows = [mem.sample(self._B, as_bool=False)[:5] for mem in self.memory]
        return tuple(torch.stack([r[k] for r in rows]) for k in range(5))

    def _sample(self):
        """``sample()`` once every member's buffer holds B rows."""
        mem, B = self.memory, self._B
        if mem is None or (mem.mem_cntr < B if self._pop_replay else any(b.mem_cntr < B for b in mem)):
            return None
        return self.sample()

    def learn(self, batch=None, noise=None, *, weights=None, losses: bool = True):
        if self.importance_weights and batch is None and weights is None:
            batch = self._sample()                # the replay's own sample, with its weights
            if batch is None:
                return None
            out = super().learn(batch, noise, weights=self.memory.last_weights, losses=losses)
            self.memory.update_from_learn(self)
            return out
        out = super().learn(batch, noise, weights=weights, losses=losses)
        if self._prioritized and batch is None and out is not None:
            self.memory.update_from_learn(self)   # the batch was the replay's last sample
        return out

    learn.__doc__ = _SacCore.learn.__doc__

    # ---- members in and out

    def export_member(self, m: int) -> NativeSAC:
        """A stand-alone ``NativeSAC`` with member m's weights, Adam moments, step, noise seed and
        act count (a copy)."""
        p = self.params
        return NativeSAC.from_slab(self.device, self.configs[m], self.weights[m], obs_dim=p.obs_dim,
                                   max_action=p.max_action, adam_eps=p.adam_eps,
                                   noise_seed=self.members[m].noise_seed, adam_step=self.adam_step,
                                   act_calls=self.act_calls)

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
