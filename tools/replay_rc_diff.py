"""Compare the return codes of two builds of libsacenv.so over the replay entry points.

    python tools/replay_rc_diff.py PARENT.so HEAD.so

Every sacenv_replay_* and sacenv_replay_pop_* entry point (and sacenv_copy_standin) is
called in both libraries with the same arguments: one call with every argument good,
then every argument in turn at each of its other values (bad, boundary, null,
misaligned), then every pair of arguments at their other values -- two faults at once,
which is what pins the ORDER of the checks. sacenv_replay_stage_side runs that grid four
times: with all three roles, and with the draws alone, the pack alone and the unpack alone
(the other roles switched off), so that each role's checks meet one and two faults of their
own. Device pointers are made-up addresses: no
entry point reads them on the host, and without a GPU a valid call fails at its launch
with the same HIP code in both libraries. Prints the calls compared and every mismatch;
exits non-zero on any. A host-side refactor must leave every code as it was.
"""
import ctypes as C
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sac-agent_amd"))
from sacenv import _lib  # noqa: E402

BASE = 0x7F0000000000


def ptr(i):
    """argument i's device pointer: 256-B aligned, null, 4-B aligned only, 64-B aligned only, odd"""
    a = BASE + 0x100000 * (i + 1)
    return [a, None, a + 4, a + 64, a + 2]


def rparams(M=1000, D=11, A=1, f32=1):
    p = _lib.ReplayParams()
    p.mem_size, p.obs_dim, p.act_dim, p.reward_f32, p.terminal_mask = M, D, A, f32, 2
    return p


def sparams(period=128, offset=0, n=64, n_pad=64, seg=16, exp=6):
    sp = _lib.StagedParams()
    sp.period, sp.offset, sp.n, sp.n_pad, sp.seg, sp.experiment = period, offset, n, n_pad, seg, exp
    return sp


KEEP = []   # the structs the calls point to


def ref(x):
    KEEP.append(x)
    return C.byref(x)


RP = [ref(rparams()), None, ref(rparams(M=0)), ref(rparams(M=1 << 31)), ref(rparams(M=(1 << 31) - 1)),
      ref(rparams(D=0)), ref(rparams(A=0)), ref(rparams(M=4)), ref(rparams(D=5, A=2, f32=0))]
# (the staged entry points want the boat's rows and mem_size <= seg x period)
SRP = [ref(rparams(M=2048)), None, ref(rparams(M=2049)), ref(rparams(M=0)), ref(rparams(D=5)), ref(rparams(M=2048, A=2)),
       ref(rparams(M=1)), ref(rparams(M=100))]
SP = [ref(sparams()), None, ref(sparams(offset=64)), ref(sparams(offset=65)), ref(sparams(offset=-1)),
      ref(sparams(n=0)), ref(sparams(n_pad=32)), ref(sparams(n_pad=96)), ref(sparams(seg=0)), ref(sparams(period=0)),
      ref(sparams(period=1 << 31, seg=1)), ref(sparams(period=64)), ref(sparams(period=96))]
N = [8, 0, -1, 1, 1001, 1 << 29, 1 << 32]
BATCH = [32, 0, -1, 1, (1 << 31) - 1, 1 << 27]
NB = [16, 0, -1, 1, 17, (1 << 31) - 1]
G = [3, 0, -1, 1, 1 << 40, 1 << 62]
STORED = [10, 0, -1, 1, 1 << 40]
CNTR = [5, 0, -1, -2, 1 << 40]
MEMBERS = [2, 0, -1, 1, 64, 65]
CAP = [100, 0, -1, 1, 512, 513, 1 << 31]
SEEDS = (C.c_uint32 * 64)(*range(64))
I64A, I64B = C.c_int64(), C.c_int64()
OUT = lambda x: [C.byref(x), None]   # noqa: E731  (a host output)


def stores(extra):
    """(p, arena, *extra, n, state, action, reward, new_state, final_state, code[, last_term], stream)"""
    return [RP, ptr(0), *extra, N, ptr(1), ptr(2), ptr(3), ptr(4), ptr(5), ptr(6)]


ENTRIES = {
    "sacenv_replay_layout": [RP, OUT(_lib.ReplayLayout())],
    "sacenv_replay_init": [RP, ptr(0), [7, 0, 0xFFFFFFFF], [None]],
    "sacenv_replay_store": stores([]) + [[None]],
    "sacenv_replay_store_env": stores([]) + [ptr(7), [None]],
    "sacenv_replay_store_env_at": stores([CNTR]) + [ptr(7), [None]],
    "sacenv_replay_store_shard": [RP, ptr(0), N, [0, -1, 8, 120, 121], [128, 0, -1, 8, 7], *stores([])[3:], ptr(7),
                                  [None]],
    "sacenv_replay_sample": [RP, ptr(0), BATCH, STORED, ptr(1), ptr(2), ptr(3), ptr(4), ptr(5), ptr(6), [None]],
    "sacenv_replay_sample_shard": [RP, ptr(0), BATCH, STORED, [0, -1, 64, 65], [64, 0, -1, 128, 129], [128, 0, -1, 64],
                                   ptr(1), ptr(2), ptr(3), ptr(4), ptr(5), ptr(6), [None]],
    "sacenv_replay_gather": [RP, ptr(0), BATCH, ptr(1), ptr(2), ptr(3), ptr(4), ptr(5), ptr(6), [None]],
    "sacenv_replay_stage_scratch_bytes": [RP, BATCH[:4], NB[:5], OUT(I64A)],
    "sacenv_replay_stage_draw": [SRP, ptr(0), SP, G, BATCH, NB, ptr(1), ptr(2), [1 << 30, 0, -1, 1 << 10], [None]],
    "sacenv_replay_stage_mark": [SRP, SP, G, ptr(0), ptr(1), BATCH, NB, ptr(2), [None]],
    "sacenv_replay_sample_staged": [SRP, SP, G, ptr(0), ptr(1), ptr(2), BATCH, NB, ptr(3), [None]],
    "sacenv_replay_stage_draw_ctr": [SRP, SP, G, BATCH, NB, [9, 0], ptr(0), ptr(1), ptr(2), ptr(3), [None]],
    "sacenv_replay_stage_chunk": [SRP, SP, BATCH[:4] + [1 << 27], NB, OUT(I64A), OUT(I64B)],
    "sacenv_replay_stage_pack": [SRP, SP, G, ptr(0), ptr(1), ptr(2), BATCH, NB, CAP, ptr(3), ptr(4), [1, 0], [None]],
    "sacenv_replay_stage_unpack": [[2, 0, -1, 1, 1 << 30], [4096 * 100, 0, -1, 4 * (4 + 100 * 25), 4 * (4 + 100 * 25) - 4,
                                                           4 * (4 + 100 * 25) + 2], CAP, BATCH, NB + [1 << 22],
                                   ptr(0), ptr(1), ptr(2), [None]],
    "sacenv_copy_standin": [ptr(0), ptr(1), [4096, 0, -1, 8, 16], [4, 0, 1, 4096, 4097], [5.0, 0.0, -1.0, 1e5, 2e5,
                                                                                         float("nan")], [None]],
    "sacenv_replay_pop_layout": [RP, MEMBERS, OUT(_lib.ReplayPopLayout())],
    "sacenv_replay_pop_init": [RP, MEMBERS, ptr(0), [SEEDS, None], [None]],
    "sacenv_replay_pop_store": [RP, MEMBERS, ptr(0), CNTR, N, ptr(1), ptr(2), ptr(3), ptr(4), ptr(5), ptr(6), ptr(7),
                                [None]],
    "sacenv_replay_pop_sample": [RP, MEMBERS, ptr(0), BATCH, STORED, ptr(1), ptr(2), ptr(3), ptr(4), ptr(5), ptr(6),
                                 [None]],
    "sacenv_replay_pop_gather": [RP, MEMBERS, ptr(0), BATCH, ptr(1), ptr(2), ptr(3), ptr(4), ptr(5), ptr(6), [None]],
}

# sacenv_replay_stage_side: (p, sp, batch, n_batches) and the fields of its SacenvStageSide
SIDE_FIELDS = {"draw_g": [5, -1, 0, 1 << 62], "seed": [9], "draw_idx": ptr(0), "marks_prev": ptr(1), "marks_cur": ptr(2),
               "draw_tiles": ptr(3), "pack_g": [3, -1, 0, 1 << 62], "stage_cur": ptr(4), "stage_prev": ptr(5),
               "pack_idx": ptr(6) + [ptr(0)[0]], "pack_tiles": ptr(7) + [ptr(3)[0]], "cap": CAP,
               "chunk": ptr(8), "gathered": ptr(9) + [ptr(8)[0] + 256], "chunk_bytes": ENTRIES["sacenv_replay_stage_unpack"][1],
               "words": ptr(10), "status_word": ptr(11), "world": [2, 0, -1, 1, 1 << 30]}
SIDE = [SRP, SP, BATCH, NB, *SIDE_FIELDS.values()]
_F = {k: 4 + i for i, k in enumerate(SIDE_FIELDS)}   # a field's place among the arguments
SIDE_BASES = {"": (), " (draws alone)": ((_F["pack_g"], -1), (_F["gathered"], None)),
              " (pack alone)": ((_F["draw_g"], -1), (_F["gathered"], None)),
              " (unpack alone)": ((_F["draw_g"], -1), (_F["pack_g"], -1))}


def side_call(lib, p, sp, batch, nb, *fields):
    w = _lib.StageSide()
    for k, v in zip(SIDE_FIELDS, fields):
        setattr(w, k, v)
    return lib.sacenv_replay_stage_side(p, sp, batch, nb, C.byref(w), None)


def grid(cands, base=()):
    """all good; each argument at each other value; each pair of arguments at their other values.
    ``base``: (argument, value) pairs that replace the good value of those arguments throughout."""
    good = [c[0] for c in cands]
    for i, v in base:
        good[i] = v
    yield tuple(good)
    alts = [[(i, v) for v in c[1:] if v != good[i]] for i, c in enumerate(cands)]
    for a in alts:
        for i, v in a:
            yield tuple(v if k == i else g for k, g in enumerate(good))
    for a, b in itertools.combinations(alts, 2):
        for (i, v), (j, u) in itertools.product(a, b):
            yield tuple(v if k == i else u if k == j else g for k, g in enumerate(good))


def main(parent, head):
    libs = [_lib.load(parent), _lib.load(head)]
    calls = {n: (lambda lib, *a, n=n: getattr(lib, n)(*a), c, ()) for n, c in ENTRIES.items()}
    for tag, base in SIDE_BASES.items():
        calls["sacenv_replay_stage_side" + tag] = (side_call, SIDE, base)
    exported = [n for n in (*_lib.EXPORTS, *_lib.REPLAY_POP_EXPORTS) if n.startswith("sacenv_replay_")]
    assert set(exported) <= set(calls), sorted(set(exported) - set(calls))
    total = bad = 0
    for name, (fn, cands, base) in calls.items():
        n = launched = 0
        for args in grid(cands, base):
            ra, rb = fn(libs[0], *args), fn(libs[1], *args)
            n += 1
            launched += ra > 0
            if ra != rb:
                bad += 1
                print(f"MISMATCH {name}{args}: parent {ra}, head {rb}")
        print(f"{name}: {n} calls, {launched} of them reached a launch")
        total += n
    print(f"{total} calls compared over {len(calls) - len(SIDE_BASES) + 1} entry points, {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
