"""Counter-based policy noise (include/sacenv_noise.h): the standard normal draws of
``choose_action`` and ``learn`` as a pure function of (member's seed, stream, call, element).

torch's ``randn`` takes every draw from the process's one device stream, so the noise member m
of a population sees depends on how many members there are, on the other members' shapes and
on everything else that drew before. ``PolicyNoise`` holds one 64-bit seed per member and
computes element i of call c of stream s from them alone (Philox4x64-10 and Box-Muller in f64;
the header has the contract, tests/noise_oracle.py restates it): member m's rows are what a
``PolicyNoise([seed_m])`` gives, whatever the other members are. One launch serves every member
and up to four draws. There is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

ACT, LEARN1, LEARN2 = _lib.NOISE_ACT, _lib.NOISE_LEARN1, _lib.NOISE_LEARN2
_U64 = (1 << 64) - 1


class PolicyNoise:
    """``seeds``: one integer in [0, 2^64) per member (an int alone is one member)."""

    ACT, LEARN1, LEARN2 = ACT, LEARN1, LEARN2

    def __init__(self, seeds, device):
        seeds = [seeds] if isinstance(seeds, int) else list(seeds)
        P = self.P = len(seeds)
        if not 1 <= P <= _lib.NOISE_MAX_MEMBERS:
            raise ValueError(f"PolicyNoise takes 1..{_lib.NOISE_MAX_MEMBERS} seeds, got {P}")
        for s in seeds:
            if int(s) != s or not 0 <= int(s) <= _U64:
                raise ValueError(f"a noise seed is an integer in [0, 2^64), got {s!r}")
        self.seeds = tuple(int(s) for s in seeds)
        self.device = _lib.cuda_device(device, "PolicyNoise")
        self._normal, = _lib.require(_lib.NOISE_EXPORTS, "sacenv_noise.h")
        self._seeds = (C.c_uint64 * P)(*self.seeds)

    def draw(self, requests) -> list:
        """Up to four draws in one launch and one allocation. ``requests``: tuples
        ``(stream, call, n)`` or ``(stream, call, n, calls)``; returns one f32
        ``[calls, P, n]`` tensor per request (row k is call ``call + k``)."""
        reqs = [tuple(r) + (1,) * (4 - len(r)) for r in requests]
        if not 1 <= len(reqs) <= _lib.NOISE_MAX_STREAMS:
            raise ValueError(f"one launch serves 1..{_lib.NOISE_MAX_STREAMS} draws, got {len(reqs)}")
        P, sizes = self.P, []
        for stream, call, n, calls in reqs:
            if not (0 <= int(stream) <= _U64 and 0 <= int(call) and int(call) + int(calls) - 1 <= _U64):
                raise ValueError("stream and call are unsigned 64-bit counts")
            if int(n) < 0 or int(calls) < 1 or int(calls) * P * int(n) >= 1 << 31:
                raise ValueError(f"a draw is calls >= 1 rows of n >= 0 values, under 2^31 in all; got {calls} x {P} x {n}")
            sizes.append(int(calls) * P * int(n))
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=self.device)
        desc = (_lib.NoiseDraw * len(reqs))()
        out, off = [], 0
        for d, (stream, call, n, calls), size in zip(desc, reqs, sizes):
            t = flat[off: off + size].view(int(calls), P, int(n))
            d.stream, d.first_call, d.calls, d.n = int(stream), int(call), int(calls), int(n)
            d.out = t.data_ptr() if size else None
            out.append(t)
            off += size
        _lib.check(self._normal(P, self._seeds, len(reqs), desc, _lib.stream_handle(self.device)))
        return out

    def normal(self, stream: int, call: int, n: int, calls: int = 1) -> torch.Tensor:
        """f32 ``[calls, P, n]``: calls ``call .. call + calls - 1`` of ``stream``, n values per member."""
        return self.draw([(stream, call, n, calls)])[0]


__all__ = ["PolicyNoise", "ACT", "LEARN1", "LEARN2"]
