"""Proportional prioritized replay for a population: a ``PopulationReplay`` whose members each keep
a 64-ary sum tree over their ring rows' priorities on the device, and sample row i with
probability p_i / sum(p) (include/sacenv_prioritized_replay.h, sacenv_replay_prio.h; Schaul et al.,
"Prioritized Experience Replay", 2016).

The priorities live in a buffer of their own (``prio``, ``[P, member_bytes]``); the replay arena is
byte for byte a plain ``PopulationReplay``'s. A store marks the rows it writes with the largest
priority seen so far, a sample is a draw on the trees and the population gather, and after a learn
``update_from_learn`` turns the per-row squared TD errors the learn kernels leave in their scratch
into new priorities. The importance weights a sample computes (``last_weights``) are applied in
the critic loss with ``importance_weights=True`` (``NativeSACPopulation``; ``--importance-weights``
in examples/train_population.py; include/sacenv_weighted_learn.h), and not without it; their
exponent is ``beta``, or with ``beta_final`` / ``beta_anneal`` runs from ``beta`` to ``beta_final``
over ``beta_anneal`` samples, derived on the device from the sample's number. Priorities are u32 fixed point
(65 536 = 1.0) and node sums u64, so the tree and every drawn index are reproducible bit for bit
(tests/prio_oracle.py). Whether prioritizing speeds learning up has not been measured.

There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .population_replay import PopulationReplay

_HEADER = "sacenv_prioritized_replay.h"


class PrioritizedPopulationReplay(PopulationReplay):
    """``PopulationReplay`` sampled in proportion to priorities. ``alpha``: the exponent of the TD
    error in a priority (0: uniform over the stored rows); ``beta``: the exponent of the importance
    weights; ``eps``: added to the TD error, so that no stored row's priority is zero;
    ``prio_seeds``: one Philox seed per member for the draws (default: the members' ``seeds``)."""

    def __init__(self, members: int, max_size: int, input_shape, n_actions: int, *, alpha: float = 0.6,
                 beta: float = 0.4, eps: float = 1e-3, prio_seeds=None, beta_final: float | None = None,
                 beta_anneal: int = 0, **kw):
        fns = _lib.require(_lib.REPLAY_PRIO_EXPORTS, _HEADER)
        (_, self._init, self._mark, self._set, self._update_td, self._learn_rows, self._sample) = fns
        for name, v in (("alpha", alpha), ("beta", beta), ("eps", eps)):
            if not (math.isfinite(v) and v >= 0):
                raise ValueError(f"{name} must be finite and >= 0, got {v}")
        self.alpha, self.beta, self.eps = float(alpha), float(beta), float(eps)
        # the weights' exponent annealed from beta to beta_final over beta_anneal samples, on the
        # device (include/sacenv_weighted_learn.h); without beta_final nothing changes
        self.beta_final, self.beta_anneal, self._sample_annealed = None, 0, None
        if beta_final is not None:
            if not (math.isfinite(beta_final) and beta_final >= 0):
                raise ValueError(f"beta_final must be finite and >= 0, got {beta_final}")
            if int(beta_anneal) < 1:
                raise ValueError(f"beta_final needs beta_anneal >= 1 (the samples the exponent takes to reach "
                                 f"it), got {beta_anneal}")
            self.beta_final, self.beta_anneal = float(beta_final), int(beta_anneal)
            self._sample_annealed = _lib.weighted_learn_fn("sacenv_replay_prio_sample_annealed")
        elif beta_anneal:
            raise ValueError("beta_anneal needs beta_final")
        super().__init__(members, max_size, input_shape, n_actions, **kw)
        P = self.P
        self.prio_seeds = list(self.seeds) if prio_seeds is None else [int(s) for s in prio_seeds]
        if len(self.prio_seeds) != P:
            raise ValueError("prio_seeds must hold one seed per member")
        self._prio_seeds = (C.c_uint64 * P)(*[s & 0xFFFFFFFFFFFFFFFF for s in self.prio_seeds])
        self.prio_layout = L = _lib.replay_prio_layout(self.params, P)
        self.prio = torch.empty((P, int(L.member_bytes)), dtype=torch.uint8, device=self.device)
        _lib.check(self._init(self._pp, P, self.prio.data_ptr(), self.stream))
        self.sample_calls = 0          # the samples numbered by the host (the device counts its own: graph_safe)
        self.last_idx = self.last_leaf = self.last_weights = None
        self._rows = self._rows_of = None

    # ---- stores: mark, then store (with the device counts the mark must read them first)

    def store_batch(self, state, action, reward, new_state, code, final_state=None, last_term=None,
                    graph_safe: bool = False) -> None:
        """``PopulationReplay.store_batch``, after the rows it will write are marked with the
        largest priority so far (two to three launches more)."""
        n, ptrs = self._store_inputs(state, action, reward, new_state, code, final_state, last_term)
        cntr = -1 if graph_safe else self.mem_cntr
        _lib.check(self._mark(self._pp, self.P, self.arena.data_ptr(), self.prio.data_ptr(), cntr, n, self.stream))
        _lib.check(self.lib.sacenv_replay_pop_store(self._pp, self.P, self.arena.data_ptr(), cntr, n, *ptrs,
                                                    self.stream))
        self.mem_cntr += n

    # (store_env_step goes through store_batch)

    # ---- samples

    def sample(self, batch_size: int, as_bool: bool = True, pool_rows: int = 0, graph_safe: bool = False):
        """``PopulationReplay.sample``'s 6-tuple, every member's rows drawn from its own ring in
        proportion to their priorities; ``idx`` holds ring rows. Keeps ``last_idx``, ``last_leaf``
        (the drawn rows' priorities, u32 as i32 bits) and ``last_weights`` (f32, (min leaf /
        leaf)^beta). The draws are a function of the priorities, the member's seed and the sample's
        number: ``sample_calls``, or with ``graph_safe`` the state's own count of such samples
        (one launch more). A replay stays with one of the two."""
        if pool_rows:
            raise ValueError("a prioritized sample draws from the member's own ring: pool_rows must be 0")
        B = int(batch_size)
        self._check_stored(B)
        st, ac, rw, ns, tm, idx = self._outputs(B, idx=True)
        leaf = torch.empty(self.P, B, dtype=torch.int32, device=self.device)
        w = torch.empty(self.P, B, dtype=torch.float32, device=self.device)
        if self._sample_annealed is None:
            _lib.check(self._sample(self._pp, self.P, self.arena.data_ptr(), self.prio.data_ptr(), B,
                                    -1 if graph_safe else self.sample_calls, self._prio_seeds, idx.data_ptr(),
                                    leaf.data_ptr(), w.data_ptr(), self.beta, st.data_ptr(), ac.data_ptr(),
                                    rw.data_ptr(), ns.data_ptr(), tm.data_ptr(), self.stream))
        else:   # beta_at(the sample's number), computed on the device
            _lib.check(self._sample_annealed(
                self._pp, self.P, self.arena.data_ptr(), self.prio.data_ptr(), B,
                -1 if graph_safe else self.sample_calls, self._prio_seeds, idx.data_ptr(), leaf.data_ptr(),
                w.data_ptr(), self.beta, self.beta_final, self.beta_anneal, st.data_ptr(), ac.data_ptr(),
                rw.data_ptr(), ns.data_ptr(), tm.data_ptr(), self.stream))
        if B > 0 and not graph_safe:
            self.sample_calls += 1
        self.last_idx, self.last_leaf, self.last_weights = idx, leaf, w
        return st, ac, rw, ns, (tm.bool() if as_bool else tm), idx

    def beta_at(self, k: int) -> float:
        """The weights' exponent of sample number ``k`` (``sample_calls``, or with ``graph_safe``
        ``header(m)["calls"]``, before the sample): ``beta`` without ``beta_final``, else in f64
        ``beta + (beta_final - beta) * (min(k, beta_anneal) / beta_anneal)``, as the device forms it."""
        if self.beta_final is None:
            return self.beta
        n = self.beta_anneal
        return self.beta + (self.beta_final - self.beta) * (min(int(k), n) / n)

    def sample_pool(self, batch_size: int, pool_rows: int, as_bool: bool = True):
        raise ValueError("a prioritized replay does not pool: pool_rows must be 0")

    # ---- priorities

    def set_priorities(self, idx, leaf) -> None:
        """Explicit priorities: u32 fixed point (65 536 = 1.0) ``[P, B]`` for the ring rows ``idx``
        ``[P, B]``; clamped to [1, 2^31 - 1], rows outside the ring skipped, of equal rows the last
        wins."""
        idx = self._idx(idx)
        leaf = torch.as_tensor(leaf).to(device=self.device, dtype=torch.int64)
        if leaf.shape != idx.shape:
            raise ValueError("leaf must have idx's shape")
        lo = leaf.clamp(0, 0xFFFFFFFF).to(torch.int32).contiguous()   # (the low 32 bits: u32 as the kernel reads it)
        _lib.check(self._set(self._pp, self.P, self.prio.data_ptr(), idx.shape[1], idx.data_ptr(), lo.data_ptr(),
                             self.stream))

    def update_priorities(self, idx, td_sq1, td_sq2=None, member_stride: int | None = None) -> None:
        """Priorities from squared TD errors: f32 ``[P, B]`` tensors (or, with ``member_stride`` in
        floats, views whose member m starts m strides after member 0), as
        ``sacenv_replay_prio_update_td`` states."""
        idx = self._idx(idx)
        B = idx.shape[1]
        if member_stride is None:
            td_sq1 = torch.as_tensor(td_sq1, device=self.device).to(torch.float32).contiguous()
            if td_sq1.shape != idx.shape:
                raise ValueError("td_sq1 must have idx's shape")
            if td_sq2 is not None:
                td_sq2 = torch.as_tensor(td_sq2, device=self.device).to(torch.float32).contiguous()
                if td_sq2.shape != idx.shape:
                    raise ValueError("td_sq2 must have idx's shape")
            member_stride = B
        _lib.check(self._update_td(self._pp, self.P, self.prio.data_ptr(), B, idx.data_ptr(), td_sq1.data_ptr(),
                                   None if td_sq2 is None else td_sq2.data_ptr(), int(member_stride), self.alpha,
                                   self.eps, self.stream))

    def learn_rows(self, pop):
        """(td_sq1, td_sq2, member_stride): the ``[B]``-row views into ``pop``'s learn scratch where
        its last learn left (q - q_hat)^2 of critic 1 and 2 for member 0, and the floats between two
        members."""
        o1, o2 = C.c_int64(), C.c_int64()
        _lib.check(self._learn_rows(pop._pp, C.byref(o1), C.byref(o2)))
        stride = int(pop.pop_layout.scratch_bytes) // 4
        B = pop._B
        return pop.scratch[o1.value: o1.value + B], pop.scratch[o2.value: o2.value + B], stride

    def update_from_learn(self, pop) -> None:
        """After ``pop.learn()`` on the batch this replay sampled last: that batch's rows take the
        priorities of their TD errors (one call, three launches; the scratch is read in place)."""
        if self.last_idx is None:
            raise RuntimeError("update_from_learn follows a sample")
        if pop.P != self.P or pop._B != self.last_idx.shape[1]:
            raise ValueError("the population's members and batch must be the last sample's")
        if self._rows_of is not pop:   # (the views of this population's scratch, looked up once)
            self._rows, self._rows_of = self.learn_rows(pop), pop
        rows = self._rows
        self.update_priorities(self.last_idx, rows[0], rows[1], member_stride=rows[2])

    # ---- inspection

    def levels(self, m: int) -> list:
        """Member m's tree as numpy copies: [leaves u32 [M], level 1 u64, ...]."""
        L, slab = self.prio_layout, self.prio[m].cpu().numpy()
        out = []
        for k in range(L.levels):
            dt, n, off = (np.uint32 if k == 0 else np.uint64), int(L.count[k]), int(L.offset[k])
            out.append(slab[off: off + n * np.dtype(dt).itemsize].view(dt).copy())
        return out

    def header(self, m: int) -> dict:
        h = self.prio[m, :24].cpu().numpy()
        return {"total": int(h[0:8].view(np.uint64)[0]), "max_leaf": int(h[8:12].view(np.uint32)[0]),
                "calls": int(h[16:24].view(np.int64)[0])}

    def total(self, m: int) -> int:
        return self.header(m)["total"]


__all__ = ["PrioritizedPopulationReplay"]
