"""The replay buffers of a population: P ``DeviceReplayBuffer``s in one arena, stored to and
sampled in one set of launches (include/sacenv_population_replay.h, sacenv_replay_pop.hip).

``NativeSACPopulation`` acts and learns for P agents in 1 + 4 launches; with one
``DeviceReplayBuffer`` per member its replay side costs a store launch, a draw launch and a
gather launch per member and five stack copies per iteration. ``PopulationReplay`` holds the P
buffers as the rows of one ``[P, member_bytes]`` arena, each laid out as a
``DeviceReplayBuffer``'s: a store is one launch, a sample two, for all members, and the sampled
batches come out as the ``[P, B, ...]`` tensors ``NativeSACPopulation.learn`` reads. Member m's
bytes and batches are those of a ``DeviceReplayBuffer`` with member m's seed given member m's
rows, bit for bit (tests/test_population_replay_gpu.py); ``export_member`` copies one out.

The members store in lockstep: n rows each per call, one count for all. There is no CPU path.

``sample(B, pool_rows=K)`` draws K of every member's B rows from all members' rings
(include/sacenv_population_share.h): the rings lie side by side in the arena, so the pooled draw
is an index computation and a gather across slabs, still two launches. With K > 0 a member's
batches depend on the other members' rows; with K = 0 nothing changes.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .replay import TERMINAL_GOAL, DeviceReplayBuffer, _cuda_device, _ReplayArena


class PopulationReplay(_ReplayArena):
    def __init__(self, members: int, max_size: int, input_shape, n_actions: int, *, device=None, seeds=None,
                 reward_f32: bool = True, terminal_mask: int = TERMINAL_GOAL):
        _lib.require(_lib.REPLAY_POP_EXPORTS, "sacenv_population_replay.h")
        device = _cuda_device(device, "PopulationReplay")   # (a CPU device is refused before the members are looked at)
        P = self.P = int(members)
        if not 1 <= P <= _lib.REPLAY_POP_MAX_MEMBERS:
            raise ValueError(f"a population replay holds 1 to {_lib.REPLAY_POP_MAX_MEMBERS} members, got {P}")
        self.seeds = list(range(P)) if seeds is None else [int(s) for s in seeds]
        if len(self.seeds) != P:
            raise ValueError("seeds must hold one seed per member")
        super().__init__((P,), max_size, input_shape, n_actions, device, reward_f32, terminal_mask)
        self.pop_layout = _lib.replay_pop_layout(self.params, P)   # (self.layout: inside a member's slab)
        self.member_bytes = int(self.pop_layout.member_bytes)
        self.mt_pos = self.mt_pos[:, 0]
        sd = (C.c_uint32 * P)(*[s & 0xFFFFFFFF for s in self.seeds])
        _lib.check(self.lib.sacenv_replay_pop_init(self._pp, P, self.arena.data_ptr(), sd, self.stream))

    def __len__(self) -> int:
        return self.P

    def store_batch(self, state, action, reward, new_state, code, final_state=None, last_term=None,
                    graph_safe: bool = False) -> None:
        """Append n transitions per member: ``DeviceReplayBuffer.store_batch`` with a leading
        member axis on every argument (state ``[P, n, D]``, ``last_term`` a contiguous u8
        ``[P, n]`` device tensor, in/out). One launch, or with ``graph_safe=True`` a store
        and an advance launch on the device counts."""
        n, ptrs = self._store_inputs(state, action, reward, new_state, code, final_state, last_term)
        _lib.check(self.lib.sacenv_replay_pop_store(self._pp, self.P, self.arena.data_ptr(),
                                                    -1 if graph_safe else self.mem_cntr, n, *ptrs, self.stream))
        self.mem_cntr += n

    def store_env_step(self, prev_obs, actions, env, reference_terminal: bool = True) -> None:
        """The transitions of one ``VecBoatEnv.step`` of P x n envs, member m owning envs
        [m n, (m + 1) n): the env's own reward, obs, term and final_obs are the ``[P][n]``
        inputs as they lie (no copy). ``reference_terminal``: as
        ``DeviceReplayBuffer.store_env_step``, one persistent byte per env."""
        P = self.P
        if env.num_envs % P:
            raise ValueError(f"the env's {env.num_envs} envs do not split over {P} members")
        n = env.num_envs // P
        D = self.params.obs_dim
        s = self._dev(prev_obs, torch.float32)
        a = self._dev(actions, torch.float32)
        if s.numel() != P * n * D or a.numel() != P * n * self.n_actions:
            raise ValueError("prev_obs and actions must hold one row per env")
        self.store_batch(s.view(P, n, *self.input_shape), a.view(P, n, -1), env.reward.view(P, n),
                         env.obs.view(P, n, *self.input_shape), env.term.view(P, n),
                         final_state=env.final_obs.view(P, n, *self.input_shape),
                         last_term=self._env_last_term(env) if reference_terminal else None)

    def _idx(self, idx) -> torch.Tensor:
        """``idx`` as a contiguous i64 ``[P, B]`` tensor on the device."""
        idx = torch.as_tensor(idx).to(device=self.device, dtype=torch.int64).contiguous()
        if idx.dim() != 2 or idx.shape[0] != self.P:
            raise ValueError(f"idx must be [{self.P}, B], got {list(idx.shape)}")
        return idx

    def _check_stored(self, B: int) -> None:
        """np.random.choice(0, B)'s refusal: nothing is drawn from an empty ring."""
        if self.mem_cntr == 0 and B > 0:
            raise ValueError("a must be greater than 0 unless no samples are taken")

    def sample(self, batch_size: int, as_bool: bool = True, pool_rows: int = 0):
        """``DeviceReplayBuffer.sample`` for every member in two launches: (states [P, B, D],
        actions [P, B, A], rewards f64 [P, B], states_, dones [P, B], idx [P, B]), member m's
        from its own stream. ``as_bool=False``: dones as the kernel writes them (u8 0/1).

        ``pool_rows=K`` > 0 (include/sacenv_population_share.h): the last K rows of every
        member's batch come from the whole arena -- member m draws ``choice(s, B - K)`` from its
        own ring, then ``choice(P s, K)`` over all members' rows, on its own stream -- and
        ``idx`` holds GLOBAL rows, owner x mem_size + row (what ``gather_pool`` takes). With 0
        the call is what it was: the members' ring rows, through the same entry point."""
        if pool_rows:
            return self.sample_pool(batch_size, pool_rows, as_bool)
        B = int(batch_size)
        self._check_stored(B)
        st, ac, rw, ns, tm, idx = self._outputs(B, idx=True)
        _lib.check(self.lib.sacenv_replay_pop_sample(
            self._pp, self.P, self.arena.data_ptr(), B, self.mem_cntr, idx.data_ptr(), st.data_ptr(), ac.data_ptr(),
            rw.data_ptr(), ns.data_ptr(), tm.data_ptr(), self.stream))
        return st, ac, rw, ns, (tm.bool() if as_bool else tm), idx

    def sample_pool(self, batch_size: int, pool_rows: int, as_bool: bool = True):
        """``sample`` through ``sacenv_replay_pop_sample_pool`` whatever ``pool_rows`` is (0 to
        ``batch_size``): ``idx`` holds global rows, owner x mem_size + row. With ``pool_rows=0``
        the batches, and the arena's bytes afterwards, are ``sample``'s, and ``idx`` is
        ``sample``'s plus m x mem_size."""
        B, K = int(batch_size), int(pool_rows)
        if not 0 <= K <= max(B, 0):
            raise ValueError(f"pool_rows must lie in [0, batch_size = {B}], got {K}")
        self._check_stored(B)
        fn, = _lib.require(_lib.REPLAY_SHARE_EXPORTS[:1], "sacenv_population_share.h", self.lib)
        st, ac, rw, ns, tm, idx = self._outputs(B, idx=True)
        _lib.check(fn(self._pp, self.P, self.arena.data_ptr(), B, K, self.mem_cntr, idx.data_ptr(), st.data_ptr(),
                      ac.data_ptr(), rw.data_ptr(), ns.data_ptr(), tm.data_ptr(), self.stream))
        return st, ac, rw, ns, (tm.bool() if as_bool else tm), idx

    def _gather(self, fn, idx, as_bool: bool):
        idx = self._idx(idx)
        B = idx.shape[1]
        st, ac, rw, ns, tm, _ = self._outputs(B)
        _lib.check(fn(self._pp, self.P, self.arena.data_ptr(), B, idx.data_ptr(), st.data_ptr(), ac.data_ptr(),
                      rw.data_ptr(), ns.data_ptr(), tm.data_ptr(), self.stream))
        return st, ac, rw, ns, (tm.bool() if as_bool else tm)

    def gather_pool(self, idx: torch.Tensor, as_bool: bool = True):
        """The rows at the given global indices ``[P, B]`` (owner x mem_size + row, as a pooled
        ``sample`` returns them), for every member, each from its owner's slab (one launch); an
        index outside ``[0, P x mem_size)`` gives zeros."""
        fn, = _lib.require(_lib.REPLAY_SHARE_EXPORTS[1:], "sacenv_population_share.h", self.lib)
        return self._gather(fn, idx, as_bool)

    def gather(self, idx: torch.Tensor, as_bool: bool = True):
        """The rows at the given ring indices ``[P, B]``, for every member (one launch); an
        index outside the ring gives zeros."""
        return self._gather(self.lib.sacenv_replay_pop_gather, idx, as_bool)

    def export_member(self, m: int) -> DeviceReplayBuffer:
        """A stand-alone ``DeviceReplayBuffer`` with a copy of member m's arena and count."""
        rb = DeviceReplayBuffer(self.mem_size, self.input_shape, self.n_actions, device=self.device,
                                seed=self.seeds[m], reward_f32=bool(self.params.reward_f32),
                                terminal_mask=int(self.params.terminal_mask))
        rb.arena.copy_(self.arena[m])
        rb.mem_cntr = self.mem_cntr
        return rb


__all__ = ["PopulationReplay"]
