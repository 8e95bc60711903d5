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
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib
from .replay import TERMINAL_GOAL, DeviceReplayBuffer


class PopulationReplay:
    def __init__(self, members: int, max_size: int, input_shape, n_actions: int, *, device=None, seeds=None,
                 reward_f32: bool = True, terminal_mask: int = TERMINAL_GOAL):
        self.lib = _lib.load()
        if not hasattr(self.lib, "sacenv_replay_pop_store"):
            raise _lib.SacenvError("this libsacenv.so was built before sacenv_population_replay.h")
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("PopulationReplay runs on a GPU (HIP); no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        P = self.P = int(members)
        if not 1 <= P <= _lib.REPLAY_POP_MAX_MEMBERS:
            raise ValueError(f"a population replay holds 1 to {_lib.REPLAY_POP_MAX_MEMBERS} members, got {P}")
        self.seeds = list(range(P)) if seeds is None else [int(s) for s in seeds]
        if len(self.seeds) != P:
            raise ValueError("seeds must hold one seed per member")
        shape = (int(input_shape),) if np.isscalar(input_shape) else tuple(int(d) for d in input_shape)
        self.input_shape = shape
        self.mem_size = int(max_size)
        self.n_actions = int(n_actions)
        p = _lib.ReplayParams()
        p.mem_size, p.obs_dim, p.act_dim = self.mem_size, int(np.prod(shape)), self.n_actions
        p.reward_f32, p.terminal_mask = int(bool(reward_f32)), int(terminal_mask)
        self.params = p
        self._pp = C.byref(p)
        self.layout = L = _lib.replay_layout(p)              # inside a member's slab
        self.pop_layout = PL = _lib.replay_pop_layout(p, P)
        self.member_bytes = int(PL.member_bytes)
        self.arena = torch.zeros((P, self.member_bytes), dtype=torch.uint8, device=self.device)
        M, A = self.mem_size, self.n_actions

        def view(off, dtype, *shp):  # [P, *shp]: member m's field, strided over the arena's rows
            esz = torch.empty((), dtype=dtype).element_size()
            return self.arena[:, off: off + int(np.prod(shp)) * esz].view(dtype).unflatten(1, shp)

        self.state_memory = view(L.state, torch.float32, M, *shape)
        self.new_state_memory = view(L.new_state, torch.float32, M, *shape)
        self.action_memory = view(L.action, torch.float32, M, A)
        self.reward_memory = view(L.reward, torch.float64, M)
        self.terminal_memory = view(L.terminal, torch.uint8, M)
        self._cntr = view(L.mem_cntr, torch.int64, 1)
        self.mt_key = view(L.mt_key, torch.int32, _lib.MT_N)
        self.mt_pos = view(L.mt_pos, torch.int32, 1)[:, 0]
        self.mem_cntr = 0                        # host mirror: every member's count
        # env -> u8 [P x n] info['termination'] codes (DeviceReplayBuffer._last_term)
        self._last_term = weakref.WeakKeyDictionary()
        sd = (C.c_uint32 * P)(*[s & 0xFFFFFFFF for s in self.seeds])
        _lib.check(self.lib.sacenv_replay_pop_init(self._pp, P, self.arena.data_ptr(), sd, self.stream))

    def __len__(self) -> int:
        return self.P

    @property
    def stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _dev(self, x, dtype):
        t = torch.as_tensor(x, device=self.device)
        return t.to(dtype).contiguous() if t.dtype != dtype else t.contiguous()

    def store_batch(self, state, action, reward, new_state, code, final_state=None, last_term=None,
                    graph_safe: bool = False) -> None:
        """Append n transitions per member: ``DeviceReplayBuffer.store_batch`` with a leading
        member axis on every argument (state ``[P, n, D]``, ``last_term`` a contiguous u8
        ``[P, n]`` device tensor, in/out). One launch, or with ``graph_safe=True`` a store
        and an advance launch on the device counts."""
        P = self.P
        s = self._dev(state, torch.float32)
        if s.dim() < 3 or s.shape[0] != P:
            raise ValueError(f"state must be [{P}, n, ...] (one block of rows per member), got {list(s.shape)}")
        n = s.shape[1]
        a = self._dev(action, torch.float32)
        r = self._dev(reward, torch.float32 if self.params.reward_f32 else torch.float64)
        ns = self._dev(new_state, torch.float32)
        c = self._dev(code, torch.uint8)
        fs = None if final_state is None else self._dev(final_state, torch.float32)
        # every tensor is contiguous with the state's leading [P, n], so member m's rows are
        # its m-th block of n (counts as DeviceReplayBuffer.store_batch checks them, times P)
        rows = P * n
        if (s.numel() != rows * self.params.obs_dim or ns.shape != s.shape or a.numel() != rows * self.n_actions
                or r.numel() != rows or c.numel() != rows or (fs is not None and fs.shape != s.shape)
                or (n and not (a.dim() and r.dim() and c.dim() and a.shape[0] == r.shape[0] == c.shape[0] == P))):
            raise ValueError(f"transition shapes do not match the buffer and its {P} members")
        lt = None
        if last_term is not None:
            lt = last_term
            if (not isinstance(lt, torch.Tensor) or lt.dtype != torch.uint8 or lt.device != self.device
                    or lt.numel() != P * n or not lt.is_contiguous()):
                raise ValueError("last_term must be a contiguous u8 device tensor with one byte per member and row")
        _lib.check(self.lib.sacenv_replay_pop_store(
            self._pp, P, self.arena.data_ptr(), -1 if graph_safe else self.mem_cntr, n, s.data_ptr(), a.data_ptr(),
            r.data_ptr(), ns.data_ptr(), None if fs is None else fs.data_ptr(), c.data_ptr(),
            None if lt is None else lt.data_ptr(), self.stream))
        self._keep = (s, a, r, ns, c, fs)
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
        last = None
        if reference_terminal:
            last = self._last_term.get(env)
            if last is None or last.numel() != env.num_envs:
                last = torch.zeros(env.num_envs, dtype=torch.uint8, device=self.device)
                self._last_term[env] = last
        D = self.params.obs_dim
        s = self._dev(prev_obs, torch.float32)
        a = self._dev(actions, torch.float32)
        if s.numel() != P * n * D or a.numel() != P * n * self.n_actions:
            raise ValueError("prev_obs and actions must hold one row per env")
        self.store_batch(s.view(P, n, *self.input_shape), a.view(P, n, -1), env.reward.view(P, n),
                         env.obs.view(P, n, *self.input_shape), env.term.view(P, n),
                         final_state=env.final_obs.view(P, n, *self.input_shape), last_term=last)

    def _outputs(self, B: int):
        P, dev = self.P, self.device
        st = torch.empty((P, B, *self.input_shape), dtype=torch.float32, device=dev)
        ns = torch.empty_like(st)
        ac = torch.empty((P, B, self.n_actions), dtype=torch.float32, device=dev)
        rw = torch.empty((P, B), dtype=torch.float64, device=dev)
        tm = torch.empty((P, B), dtype=torch.uint8, device=dev)
        return st, ac, rw, ns, tm

    def sample(self, batch_size: int, as_bool: bool = True):
        """``DeviceReplayBuffer.sample`` for every member in two launches: (states [P, B, D],
        actions [P, B, A], rewards f64 [P, B], states_, dones [P, B], idx [P, B]), member m's
        from its own stream. ``as_bool=False``: dones as the kernel writes them (u8 0/1)."""
        B = int(batch_size)
        if self.mem_cntr == 0 and B > 0:
            raise ValueError("a must be greater than 0 unless no samples are taken")
        idx = torch.empty((self.P, B), dtype=torch.int64, device=self.device)
        st, ac, rw, ns, tm = self._outputs(B)
        _lib.check(self.lib.sacenv_replay_pop_sample(
            self._pp, self.P, self.arena.data_ptr(), B, self.mem_cntr, idx.data_ptr(), st.data_ptr(), ac.data_ptr(),
            rw.data_ptr(), ns.data_ptr(), tm.data_ptr(), self.stream))
        return st, ac, rw, ns, (tm.bool() if as_bool else tm), idx

    def gather(self, idx: torch.Tensor, as_bool: bool = True):
        """The rows at the given ring indices ``[P, B]``, for every member (one launch); an
        index outside the ring gives zeros."""
        idx = torch.as_tensor(idx).to(device=self.device, dtype=torch.int64).contiguous()
        if idx.dim() != 2 or idx.shape[0] != self.P:
            raise ValueError(f"idx must be [{self.P}, B], got {list(idx.shape)}")
        B = idx.shape[1]
        st, ac, rw, ns, tm = self._outputs(B)
        _lib.check(self.lib.sacenv_replay_pop_gather(
            self._pp, self.P, self.arena.data_ptr(), B, idx.data_ptr(), st.data_ptr(), ac.data_ptr(), rw.data_ptr(),
            ns.data_ptr(), tm.data_ptr(), self.stream))
        return st, ac, rw, ns, (tm.bool() if as_bool else tm)

    def export_member(self, m: int) -> DeviceReplayBuffer:
        """A stand-alone ``DeviceReplayBuffer`` with a copy of member m's arena and count."""
        rb = DeviceReplayBuffer(self.mem_size, self.input_shape, self.n_actions, device=self.device,
                                seed=self.seeds[m], reward_f32=bool(self.params.reward_f32),
                                terminal_mask=int(self.params.terminal_mask))
        rb.arena.copy_(self.arena[m])
        rb.mem_cntr = self.mem_cntr
        return rb


__all__ = ["PopulationReplay"]
