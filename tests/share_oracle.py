"""The pooled sample in plain numpy (include/sacenv_population_share.h).

``draw`` restates the index draw of ``sacenv_replay_pop_sample_pool`` on numpy's own legacy
generator: member m's ``RandomState`` makes two consecutive ``choice`` calls, ``choice(s, B - K)``
for its own ring and ``choice(P * s, K)`` for the pool, and every index comes out as a global row,
owner x M + row. ``gather`` restates the gather on the members' rows as numpy arrays. Nothing here
knows the device's masked-rejection loop: the reference is numpy itself.
"""
from __future__ import annotations

import numpy as np


def draw(rngs, P: int, M: int, count: int, B: int, K: int, poisoned=()) -> np.ndarray:
    """idx i64 [P][B] of one pooled sample with ``count`` rows stored per member; ``rngs[m]`` is
    member m's ``np.random.RandomState`` and is advanced as the device advances member m's
    stream. A member in ``poisoned`` draws nothing: -1, and its generator stays where it is."""
    if not 0 <= K <= B:
        raise ValueError("pool_rows must lie in [0, batch]")
    if count <= 0:
        raise ValueError("a must be greater than 0 unless no samples are taken")
    s = min(int(count), int(M))
    idx = np.empty((P, B), np.int64)
    for m in range(P):
        if m in poisoned:
            idx[m] = -1
            continue
        own = rngs[m].choice(s, B - K).astype(np.int64)
        g = rngs[m].choice(P * s, K).astype(np.int64)
        idx[m, : B - K] = m * M + own
        idx[m, B - K:] = (g // s) * M + g % s
    return idx


def gather(fields, idx, M: int) -> list:
    """The rows at the global indices ``idx [P][B]``: for every array ``[P, M, ...]`` of
    ``fields`` the ``[P, B, ...]`` batch, row ``idx % M`` of member ``idx // M``; an index outside
    ``[0, P x M)`` gives zeros."""
    idx = np.asarray(idx, np.int64)
    out = []
    for f in fields:
        f = np.asarray(f)
        P = f.shape[0]
        flat = f.reshape(P * M, *f.shape[2:])
        inside = (idx >= 0) & (idx < P * M)
        rows = flat[np.where(inside, idx, 0)]
        rows[~inside] = 0
        out.append(rows)
    return out
