"""The episode traces in plain numpy (include/sacenv_traces.h).

``TraceOracle`` takes the steps as arrays -- what the step launches write (obs, reward, done,
term, final_obs) and the actions -- and the state at attachment, walks them env by env, applies
the rule per member over its endings in (end_step, env) order and returns every member's header
and rows exactly as the header defines them. ``synthetic_steps`` makes step arrays with chosen
endings and ``pack_records`` lays a range of them out as the packed boat records
(obs f32 [n_pad][11] | reward f32 [n_pad] | done u8 [n_pad] | term u8 [n_pad]).
"""
from __future__ import annotations

import struct

import numpy as np

OBS = 11
HEADER_BYTES = ROW_BYTES = 64
RECORD_BYTES = 50
HEADER_FORMAT = "<qdiiIiiiq16x"      # SacenvTraceHeader
assert struct.calcsize(HEADER_FORMAT) == HEADER_BYTES
EMPTY = struct.pack(HEADER_FORMAT, -1, float("-inf"), -1, 0, 0, 0, 0, 0, 0)


def member_bytes(max_steps: int) -> int:
    return HEADER_BYTES + ROW_BYTES * (max_steps + 1)


def store_bytes(n_pad: int, max_steps: int, call_steps: int) -> int:
    """The working store's size: the per-wave candidates, the per-(step, wave) maxima, the carry
    and max_steps + call_steps slots of 52 B per env."""
    waves = n_pad // 64
    return 32 * waves + (8 * call_steps * waves + 15) // 16 * 16 + 12 * n_pad + 52 * n_pad * (max_steps + call_steps)


def pack_row(obs, action, reward) -> bytes:
    return (np.asarray(obs, "<f4").tobytes() + struct.pack("<ff", np.float32(action), np.float32(reward))
            + bytes(12))


class TraceOracle:
    """``members`` members of ``envs_per_member`` envs each over ``n_envs`` envs, at most
    ``max_steps`` + 1 rows kept. Attachment: ``obs0`` [n_envs, 11] every env's obs before the
    first step, ``carry_score`` f64 / ``carry_length`` i32 [n_envs] the episodes in flight."""

    def __init__(self, n_envs, members, envs_per_member, max_steps, *, env_base=0, step0=0, obs0=None,
                 carry_score=None, carry_length=None):
        self.n, self.P, self.N, self.R = int(n_envs), int(members), int(envs_per_member), int(max_steps)
        self.env_base, self.step0 = int(env_base), int(step0)
        self.obs0 = np.zeros((self.n, OBS), np.float32) if obs0 is None else np.asarray(obs0, np.float32)
        self.c_score = np.zeros(self.n) if carry_score is None else np.asarray(carry_score, np.float64)
        self.c_len = np.zeros(self.n, np.int64) if carry_length is None else np.asarray(carry_length, np.int64)
        self.obs, self.reward, self.done, self.term, self.final, self.action = [], [], [], [], [], []

    def feed(self, obs, reward, done, term, final_obs, actions) -> None:
        """Append K steps: obs [K, n, 11], reward / done / term / actions [K, n], final_obs [K, n, 11]."""
        for dst, src in ((self.obs, obs), (self.reward, reward), (self.done, done), (self.term, term),
                         (self.final, final_obs), (self.action, actions)):
            dst.extend(np.asarray(src)[:, : self.n])

    def endings(self) -> list:
        """Every finished episode as (end_step, env index, score, length, term), walked env by env:
        each f32 reward widened to f64 and added in step order from +0.0 (from the carry for the
        episode in flight at attachment); sorted by (end_step, env)."""
        out = []
        for e in range(self.n):
            score, length = float(self.c_score[e]), int(self.c_len[e])
            for k in range(len(self.done)):
                with np.errstate(all="ignore"):
                    score = float(np.float64(score) + np.float64(self.reward[k][e]))
                length += 1
                if self.done[k][e]:
                    out.append((self.step0 + k, e, score, length, int(self.term[k][e])))
                    score, length = 0.0, 0
        return sorted(out, key=lambda x: (x[0], x[1]))

    def rows_of(self, t: int, e: int, L: int):
        """(first_row, [packed rows first_row .. L]) of the episode of env e that ended at global
        step t with length L. Row j lives at global step t - L + j; it is there if it is among
        the last max_steps + 1 and the keeper saw it: row 0 needs the obs of step t - L (the slot
        before step0 holds the obs at attachment), every other row its own step's action and
        reward too."""
        rows, first = [], L
        for j in range(L, -1, -1):
            u = t - L + j
            seen = u >= self.step0 - 1 if j == 0 else u >= self.step0
            if not seen or j < L - self.R:
                break
            k = u - self.step0
            if j == L:
                row = pack_row(self.final[k][e], self.action[k][e], self.reward[k][e])
            elif j == 0:
                row = pack_row(self.obs0[e] if k < 0 else self.obs[k][e], 0.0, 0.0)
            else:
                row = pack_row(self.obs[k][e], self.action[k][e], self.reward[k][e])
            rows.append(row)
            first = j
        return first, rows[::-1]

    def members(self) -> list:
        """Per member (header bytes, [row bytes]): the rule `if score > best: best = score, keep
        that episode` over the member's endings in (end_step, env) order. A NaN never wins, an
        empty member takes the first score that is not NaN, and `replaced` counts the steps at
        which the best changed."""
        state = [dict(best=float("-inf"), kept=None, steps=set()) for _ in range(self.P)]
        for t, e, score, L, term in self.endings():
            m = e // self.N
            if m >= self.P:
                continue
            s = state[m]
            if score == score and (s["kept"] is None or score > s["best"]):
                s["best"], s["kept"] = score, (t, e, score, L, term)
                s["steps"].add(t)
        out = []
        for s in state:
            if s["kept"] is None:
                out.append((EMPTY, []))
                continue
            t, e, score, L, term = s["kept"]
            first, rows = self.rows_of(t, e, L)
            out.append((struct.pack(HEADER_FORMAT, t, score, self.env_base + e, L, term, len(rows), first, 0,
                                    len(s["steps"])), rows))
        return out


def pack(members: list, max_steps: int) -> bytes:
    """The member buffer's bytes: per member the header, its rows, zeros up to max_steps + 1 rows."""
    return b"".join(h + b"".join(rows) + bytes(ROW_BYTES * (max_steps + 1 - len(rows))) for h, rows in members)


def split(raw: bytes, members: int, max_steps: int) -> list:
    """A member buffer's bytes as ``TraceOracle.members`` returns them: per member the header and
    the first ``rows`` rows."""
    mb, out = member_bytes(max_steps), []
    for m in range(members):
        part = raw[m * mb: (m + 1) * mb]
        rows = struct.unpack_from("<i", part, 28)[0]
        out.append((part[:HEADER_BYTES], [part[HEADER_BYTES + ROW_BYTES * i: HEADER_BYTES + ROW_BYTES * (i + 1)]
                                          for i in range(max(rows, 0))]))
    return out


def describe(member) -> str:
    header, rows = member
    return f"{struct.unpack(HEADER_FORMAT, header)} + {len(rows)} rows"


def synthetic_steps(T: int, n_envs: int, seed: int = 0, p_end: float = 0.15, done=None, reward=None) -> dict:
    """T steps of n_envs envs: random obs, final_obs and actions (every value different, so a row
    taken from the wrong step or env shows), rewards of a few bits (sums are exact, ties can be
    made) unless given, endings with probability ``p_end`` unless ``done`` [T, n_envs] is given,
    term codes 1..6 where done and 0 elsewhere."""
    rng = np.random.default_rng(seed)
    d = (rng.random((T, n_envs)) < p_end) if done is None else np.asarray(done, bool)
    r = rng.integers(-8, 9, (T, n_envs)).astype(np.float32) / 4 if reward is None else np.asarray(reward, np.float32)
    return {"obs": rng.random((T, n_envs, OBS), np.float32), "reward": r, "done": d.astype(np.uint8),
            "term": np.where(d, rng.integers(1, 7, (T, n_envs)), 0).astype(np.uint8),
            "final_obs": rng.random((T, n_envs, OBS), np.float32) + 2,
            "actions": rng.uniform(-1, 1, (T, n_envs)).astype(np.float32)}


def pack_records(steps: dict, k0: int, K: int, n_pad: int, pad_byte: int = 0xFF) -> np.ndarray:
    """Steps k0 .. k0 + K - 1 as packed records, u8 [K, 50 n_pad]; the columns of envs >= n_envs
    are filled with ``pad_byte`` (0xFF: their done bytes say done)."""
    n = steps["done"].shape[1]
    rec = np.full((K, RECORD_BYTES * n_pad), pad_byte, np.uint8)
    for k in range(K):
        rec[k, : 4 * OBS * n] = steps["obs"][k0 + k].reshape(-1).view(np.uint8)
        rec[k, 44 * n_pad: 44 * n_pad + 4 * n] = steps["reward"][k0 + k].view(np.uint8)
        rec[k, 48 * n_pad: 48 * n_pad + n] = steps["done"][k0 + k]
        rec[k, 49 * n_pad: 49 * n_pad + n] = steps["term"][k0 + k]
    return rec


def pad_final(steps: dict, k0: int, K: int, n_pad: int) -> np.ndarray:
    """final_obs of steps k0 .. k0 + K - 1 as f32 [K, n_pad, 11]."""
    n = steps["done"].shape[1]
    out = np.full((K, n_pad, OBS), -7.0, np.float32)
    out[:, :n] = steps["final_obs"][k0: k0 + K]
    return out
