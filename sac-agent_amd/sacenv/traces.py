"""BestEpisodes: each member's best episode, step by step, kept on the device.

The reference writes every episode's rows to ``episodes/episode_<k>_data.csv``
(postprocessing/recorder.py) and its replayer and renderer pick out the episodes that set a new
best (postprocessing/replayer.py:45-65). ``EpisodeLog`` keeps an episode's score and drops its
steps; ``MemberScoreboard`` keeps the best score per member. This class keeps what belongs to
that score -- the rows of the episode that set it -- without knowing beforehand which env will
host it: a working store on the device holds the recent steps of EVERY env, and when an episode
ends with a score above its member's best its rows are copied into that member's buffer
(``sacenv_traces_update``, include/sacenv_traces.h). No host round trip until ``table`` / ``best``.

    traces = BestEpisodes(env, members=P, envs_per_member=N)
    for _ in range(iters):
        env.step(actions)
        traces.update(actions)                       # the env's record and final_obs
    records, final = env.rollout(actions_k, final_obs=final)
    traces.update(actions_k, records, final)         # or a rollout's K steps (call_steps >= K)
    print(traces.table())
    traces.save_csv("runs/search")                   # member_<m>/episodes/episode_0_data.csv

The persistent ``segment_async`` launch rewrites its record in place, so its steps cannot be
kept afterwards; run them through ``rollout``. ``--keep-best`` of examples/train_population.py
keeps the models the reference would have on disk; this keeps the episodes it would render.
"""
from __future__ import annotations

import csv
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from .recorder import COLUMNS, INFO_KEYS, N_RPM, _fmt
from .vec_env import VecBoatEnv

HEADER_DTYPE = np.dtype({
    "names": ["end_step", "score", "env", "length", "term", "rows", "first_row", "replaced"],
    "formats": ["<i8", "<f8", "<i4", "<i4", "<u4", "<i4", "<i4", "<i8"],
    "offsets": [0, 8, 16, 20, 24, 28, 32, 40], "itemsize": _lib.TRACE_HEADER_BYTES})
# one row: obs f32 x 11 | action f32 | reward f32 | three zero words
ROW_DTYPE = np.dtype({"names": ["obs", "action", "reward"], "formats": [("<f4", (_lib.OBS_DIM,)), "<f4", "<f4"],
                      "offsets": [0, 4 * _lib.OBS_DIM, 4 * _lib.OBS_DIM + 4], "itemsize": _lib.TRACE_ROW_BYTES})


class BestEpisodes:
    """The best episode of each of ``members`` members, member m owning envs
    ``[m * envs_per_member, (m + 1) * envs_per_member)`` of ``env`` (a ``VecBoatEnv`` with
    autoreset; envs past the last member belong to nobody).

    Parameters
    ----------
    max_steps : R; at most R + 1 rows of an episode are kept, the last ones of a longer episode.
        Default: the env's ``max_episode_steps``; required when that is 0.
    call_steps : the largest number of steps one ``update`` passes (a rollout's K).
    step0 : global number of the next step passed to ``update``.
    max_bytes : refuse a working store larger than this (it holds 52 B per env for each of
        ``max_steps + call_steps`` steps).

    The carry starts from the env's running ``ep_reward`` and ``index``, as ``EpisodeLog``'s does
    (the keeper has its own, so the two are independent and no call order between them matters):
    an episode in flight at attachment is reported with its full score and length, and
    ``first_row > 0`` says how many of its leading rows were not seen. Attach between steps.
    """

    def __init__(self, env, members: int, envs_per_member: int, max_steps: int | None = None,
                 call_steps: int = 1, step0: int = 0, *, max_bytes: int = 4 << 30):
        if not isinstance(env, VecBoatEnv):
            raise ValueError("BestEpisodes keeps the episodes of a VecBoatEnv (no toy envs)")
        if not env.autoreset:
            raise ValueError("BestEpisodes needs an env with autoreset: an episode's reset obs is read from "
                             "the record of the step that ended the one before")
        self.lib = _lib.load()
        self._bytes, self._init, self._update = _lib.require(_lib.TRACES_EXPORTS, "sacenv_traces.h", self.lib)
        if max_steps is None:
            max_steps = int(env.params.max_episode_steps)
            if max_steps == 0:
                raise ValueError("max_steps is required for an env without max_episode_steps")
        self.env, self.device = env, env.device
        self.num_envs, self.n_pad = int(env.num_envs), int(env.n_pad)
        self.P, self.N, self.R, self.call_steps = int(members), int(envs_per_member), int(max_steps), int(call_steps)
        if not 1 <= self.P <= _lib.TRACES_MAX_MEMBERS or self.N < 1 or self.P * self.N > self.num_envs:
            raise ValueError(f"{self.P} members x {self.N} envs do not fit {self.num_envs} envs "
                             f"(1..{_lib.TRACES_MAX_MEMBERS} members)")
        if self.P > 1 and self.N % 64:
            raise ValueError("envs_per_member must be a multiple of 64 with more than one member (no wave "
                             "straddles two members)")
        if not 1 <= self.R <= _lib.TRACES_MAX_STEPS or not 1 <= self.call_steps <= _lib.TRACES_MAX_STEPS:
            raise ValueError(f"max_steps and call_steps must be 1..{_lib.TRACES_MAX_STEPS}")
        self.term_names = _lib.TERM_NAMES
        self.params = _lib.Traces(n_envs=self.num_envs, n_pad=self.n_pad, members=self.P, envs_per_member=self.N,
                                  env_base=int(env.env_id_offset), max_steps=self.R, call_steps=self.call_steps,
                                  step0=int(step0))
        mb, sb = C.c_int64(), C.c_int64()
        _lib.check(self._bytes(C.byref(self.params), C.byref(mb), C.byref(sb)))
        if sb.value > int(max_bytes):
            raise ValueError(f"the working store of {self.num_envs} envs x ({self.R} + {self.call_steps}) steps "
                             f"takes {sb.value} bytes, more than max_bytes = {int(max_bytes)}")
        self.member_bytes = mb.value // self.P
        self.members = torch.empty(mb.value, dtype=torch.uint8, device=self.device)
        self.store = torch.empty(sb.value, dtype=torch.uint8, device=self.device)
        NP = self.n_pad
        self.steps = _lib.TraceSteps(n_steps=1, step=int(step0), rec_stride=0, obs_off=_lib.REC_OBS * NP,
                                     reward_off=_lib.REC_REWARD * NP, done_off=_lib.REC_DONE * NP,
                                     term_off=_lib.REC_TERM * NP, final_stride=0)
        score, length = env.ep_reward.contiguous(), env.index.contiguous()
        _lib.check(self._init(C.byref(self.params), env.obs.data_ptr(), score.data_ptr(), length.data_ptr(),
                              self.members.data_ptr(), self.store.data_ptr(), env.stream))
        self._keep = (score, length)

    @property
    def step0(self) -> int:
        """Global number of the next step ``update`` expects."""
        return int(self.steps.step)

    @property
    def nbytes(self) -> int:
        """Device bytes held: the members' buffers and the working store."""
        return int(self.members.numel() + self.store.numel())

    def update(self, actions: torch.Tensor, records: torch.Tensor | None = None,
               final_obs: torch.Tensor | None = None, n_steps: int | None = None) -> None:
        """Append the next steps and keep each member's new best; only enqueues work on the env's
        stream (two launches).

        ``records=None``: the env's own ``record`` and ``final_obs``, one step, after a ``step`` /
        ``step_async`` with ``actions`` (f32, ``num_envs`` values). Otherwise ``records`` is a
        ``[K, >= record_bytes * n_pad]`` uint8 device tensor and ``final_obs`` a ``[K, n_pad, 11]``
        f32 one, as ``VecBoatEnv.rollout`` fills them, and ``actions`` the rollout's ``[K, num_envs]``
        (rows of ``records`` and ``final_obs`` may be strided; ``n_steps`` takes only the first rows).

        EVERY step of the env must be passed exactly once, in order, as for ``EpisodeLog.update``.
        """
        nb = _lib.RECORD_BYTES * self.n_pad
        if records is None:
            if final_obs is not None:
                raise ValueError("final_obs goes with records")
            if n_steps not in (None, 1):
                raise ValueError("the env's own record holds one step")
            records, final_obs, K, stride, fstride = self.env.record, self.env.final_obs_bytes, 1, 0, 0
        else:
            if (not isinstance(records, torch.Tensor) or records.dtype != torch.uint8
                    or records.device != self.device or records.dim() != 2 or records.shape[0] < 1
                    or records.shape[1] < nb or records.stride(1) != 1):
                raise ValueError(f"records must be a uint8 [K, >= {nb}] tensor on {self.device} with "
                                 "contiguous rows")
            K = int(records.shape[0]) if n_steps is None else int(n_steps)
            if not 1 <= K <= records.shape[0]:
                raise ValueError(f"n_steps must be 1..{records.shape[0]}")
            if (not isinstance(final_obs, torch.Tensor) or final_obs.dtype != torch.float32
                    or final_obs.device != self.device or final_obs.dim() != 3 or final_obs.shape[0] < K
                    or tuple(final_obs.shape[1:]) != (self.n_pad, _lib.OBS_DIM)
                    or final_obs.stride(1) != _lib.OBS_DIM or final_obs.stride(2) != 1):
                raise ValueError(f"final_obs is required with records: a float32 [>= {K}, {self.n_pad}, "
                                 f"{_lib.OBS_DIM}] tensor on {self.device} with contiguous rows")
            stride = int(records.stride(0)) if K > 1 else 0
            fstride = 4 * int(final_obs.stride(0)) if K > 1 else 0
        if K > self.call_steps:
            raise ValueError(f"n_steps = {K} is more than call_steps = {self.call_steps}")
        if (not isinstance(actions, torch.Tensor) or actions.dtype != torch.float32 or actions.device != self.device
                or not actions.is_contiguous() or actions.numel() != K * self.num_envs):
            raise ValueError(f"actions must be a contiguous float32 tensor of {K} x {self.num_envs} values "
                             f"on {self.device}")
        s = self.steps
        s.n_steps, s.rec_stride, s.final_stride = K, stride, fstride
        _lib.check(self._update(C.byref(self.params), C.byref(s), records.data_ptr(), actions.data_ptr(),
                                final_obs.data_ptr(), self.members.data_ptr(), self.store.data_ptr(),
                                self.env.stream))
        self._keep = (actions, records, final_obs)
        s.step += K

    # ---- the host's view (each synchronises)

    def raw(self) -> bytes:
        """The members' buffers' bytes, after everything enqueued so far."""
        torch.cuda.current_stream(self.device).synchronize()
        return self.members.cpu().numpy().tobytes()

    def headers(self) -> np.ndarray:
        """The members' headers as a structured array (``HEADER_DTYPE``): one read-back."""
        torch.cuda.current_stream(self.device).synchronize()
        h = self.members.view(self.P, self.member_bytes)[:, : _lib.TRACE_HEADER_BYTES].cpu().numpy()
        return np.ascontiguousarray(h).reshape(-1).view(HEADER_DTYPE)

    def _term_name(self, term: int) -> str:
        return self.term_names[term] if term < len(self.term_names) else str(term)

    def _fields(self, m: int, h) -> dict:
        return {"member": m, "score": float(h["score"]), "env": int(h["env"]), "end_step": int(h["end_step"]),
                "length": int(h["length"]), "term": self._term_name(int(h["term"])), "rows": int(h["rows"]),
                "first_row": int(h["first_row"]), "replaced": int(h["replaced"])}

    def table(self) -> list:
        """One dict per member: score, env, end_step, length, the termination's name, rows,
        first_row and replaced of its best episode; score, env, end_step and term are None for a
        member without one."""
        out = []
        for m, h in enumerate(self.headers()):
            row = self._fields(m, h)
            if row["rows"] == 0:
                row.update(score=None, env=None, end_step=None, term=None)
            out.append(row)
        return out

    def best(self, m: int):
        """Member m's best episode: the header's fields and ``obs`` [rows, 11], ``action`` [rows],
        ``reward`` [rows] (f32; row i is row ``first_row + i`` of the episode: row 0 the reset obs
        with action 0 and reward 0, the last one the terminal obs). None if it has none yet."""
        if not 0 <= m < self.P:
            raise IndexError(f"member {m} of {self.P}")
        torch.cuda.current_stream(self.device).synchronize()
        raw = self.members[m * self.member_bytes: (m + 1) * self.member_bytes].cpu().numpy()
        h = raw[: _lib.TRACE_HEADER_BYTES].view(HEADER_DTYPE)[0]
        if int(h["rows"]) == 0:
            return None
        rows = raw[_lib.TRACE_HEADER_BYTES:].view(ROW_DTYPE)[: int(h["rows"])]
        out = self._fields(m, h)
        out.update(obs=rows["obs"].copy(), action=rows["action"].copy(), reward=rows["reward"].copy())
        return out

    def save_csv(self, experiment_dir: str) -> list:
        """Each member's best episode in the reference's format (postprocessing/recorder.py), for
        its replayer and renderer: ``<dir>/member_<m>/episodes/episode_0_data.csv`` with
        ``recorder.COLUMNS``, ';'-separated, and ``info.csv`` beside it with the termination's name
        and the score. The reference writes the state BEFORE each step, so rows 0 .. length - 1
        are written and the terminal row is not; of a truncated episode (``first_row > 0``) the
        rows from ``first_row`` on. Returns the members written.

        The values are denormalised from the f32 obs with the bounds of ``Boat.return_state``
        (boat_env.py:308-323): they are f32-accurate, not the recorder's f64."""
        cfg = self.env.cfg
        gl, tw = float(cfg.goal_line), float(cfg.track_width)
        written = []
        for m in range(self.P):
            b = self.best(m)
            if b is None:
                continue
            d = os.path.join(experiment_dir, f"member_{m}", "episodes")
            os.makedirs(d, exist_ok=True)
            o = b["obs"].astype(np.float64)
            n = min(b["rows"], b["length"] - b["first_row"])      # without the terminal row
            with open(os.path.join(d, "episode_0_data.csv"), "w", newline="") as f:
                w = csv.writer(f, delimiter=";")
                w.writerow(COLUMNS)
                for i in range(n):
                    w.writerow([_fmt(o[i, 0] * gl), _fmt(o[i, 3] * (2 * tw) - tw), _fmt(o[i, 1] * 5), _fmt(o[i, 4] * 2),
                                _fmt(o[i, 6] * (2 * math.pi)), str(np.float32(b["action"][i])),
                                _fmt(b["reward"][i]), _fmt(o[i, 9] * (2 * math.pi / 3) - math.pi / 3), str(N_RPM)])
            with open(os.path.join(d, "info.csv"), "w", newline="") as f:
                w = csv.writer(f, delimiter=";")
                w.writerow(INFO_KEYS)
                w.writerow([b["term"]] + [str(int(b["term"] == k)) for k in INFO_KEYS[1:6]] + [_fmt(b["score"])])
            written.append(m)
        return written


__all__ = ["BestEpisodes", "HEADER_DTYPE", "ROW_DTYPE"]
