/*
 * sacenv_selection.h — population selection: the losers of a hyper-parameter search copy
 * the winners' weights and take perturbed copies of their four values, on the device.
 *
 * The search (main.py -p N) draws each member's actor and critic learning rate, gamma and
 * tau once and trains every member to the end. The scoreboard (sacenv_scoreboard.h) keeps
 * each member's look-back mean on the device, and the population (sacenv_population.h)
 * keeps each member's whole training state -- nets, target net, Adam moments and the
 * kernels' fragment-order copies -- in one [P, member_floats] slab. The entry points here
 * are truncation selection on those two, the exploit and explore steps of population-based
 * training (Jaderberg et al., "Population based training of neural networks", 2017): the
 * worst q ready members each become a copy of one of the best q, with each of the four
 * values multiplied by one of two factors and clipped to its range.
 *
 * Conventions as in sacenv_scoreboard.h: device pointers, `s` is host memory read during
 * the call, `stream` a hipStream_t, every call only enqueues kernels (stream-ordered,
 * graph-capturable, nothing read back, no atomics: the bytes are the same from run to
 * run), every error is found on the host before anything is launched; return 0, an
 * SACENV_E_* code or a hipError_t. sacenv.h is untouched: SACENV_ABI_VERSION does not
 * count these.
 *
 * What stays put. The board is only read: it is the record of what the envs did, and a
 * replaced member keeps its score history (`since` below keeps a fresh copy from being
 * judged at once on its old scores; with min_episodes >= lookback the look-back window
 * holds post-copy scores only by the time the member is ready again). The loser's replay
 * buffer is not copied either: SAC is off-policy, the loser's own rows stay valid.
 */
#ifndef SACENV_SELECTION_H
#define SACENV_SELECTION_H

#include "sacenv_population.h"
#include "sacenv_scoreboard.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SACENV_SELECTION_VERSION 1
#define SACENV_SELECT_MAX_MEMBERS 64          /* one wave decides: a lane per member */
#define SACENV_SELECT_HEADER_BYTES 32
#define SACENV_SELECT_MEMBER_BYTES 64
#define SACENV_SELECT_KEY1 0x73656C656374ull  /* second Philox key word ("select"); the replay
                                                 sampler's is 0, the noise's SACENV_NOISE_KEY1 */
/* the copy launch: a workgroup of COPY_THREADS lanes moves COPY_THREADS x COPY_UNROLL 16-B
 * vectors per pass; a member's slab is cut into at most COPY_CHUNKS workgroups */
#define SACENV_SELECT_COPY_THREADS 256
#define SACENV_SELECT_COPY_UNROLL 4
#define SACENV_SELECT_COPY_CHUNKS 256

typedef struct SacenvSelect {        /* host memory */
  int32_t members;                   /* P, 2 .. SACENV_SELECT_MAX_MEMBERS */
  int32_t quantile;                  /* q, 1 <= q and 2 q <= P */
  int32_t lookback;                  /* the board's (1 .. SACENV_BOARD_MAX_LOOKBACK) */
  int32_t reserved;                  /* 0 */
  int64_t min_episodes;              /* >= 1: episodes a member must finish after a replacement */
  int64_t member_floats;             /* stride of one member's slab in weights: a multiple of 4, > 0 */
  uint64_t seed;
  double factor[2];                  /* finite, > 0 (0.8 and 1.2 are the usual pair) */
  double lo[4], hi[4];               /* finite, lo[k] <= hi[k]: the clip ranges of lr_actor, lr_critic,
                                        gamma and tau, in that order */
} SacenvSelect;

/* The selection state (device, caller-owned, 16-B aligned, sacenv_select_bytes() bytes):
 *   header (32 B)
 *     int64 round            sacenv_select_step calls so far
 *     int64 replaced_total   replacements over all calls
 *     int64 0, 0
 *   members x SacenvSelectMember (64 B each)
 */
typedef struct SacenvSelectMember {
  int64_t since;        /* the board's `episodes` of this member at its last replacement; 0 at init */
  int64_t replaced;     /* how many times this member was overwritten */
  int32_t source_now;   /* the winner it was copied from in the LAST call, else -1 */
  int32_t rank_now;     /* in the last call: 0 = best among the ready members; -1 if not ready */
  int32_t parent;       /* the last source ever; -1 if none */
  int32_t reserved;     /* 0 */
  double hp[4];         /* the member's current lr_actor, lr_critic, gamma, tau */
} SacenvSelectMember;

/* 32 + 64 members. Errors: SACENV_E_NULL, SACENV_E_SIZE, SACENV_E_RANGE (as sacenv_select_step's,
 * for `s` alone). */
int sacenv_select_bytes(const SacenvSelect *s, int64_t *bytes);

/* One launch: the empty state (round 0, nobody replaced, since 0, source_now, rank_now and
 * parent -1) with hp[m] = hp0[m]'s lr_actor, lr_critic, gamma, tau. hp0: host memory,
 * [members], read during the call (the values ride in the kernel's arguments).
 * Errors: those of `s`, SACENV_E_NULL, SACENV_E_RANGE (state not 16-B aligned; one of the
 * 4 x members values not finite). */
int sacenv_select_init(const SacenvSelect *s, const SacenvSacMember *hp0, void *state, void *stream);

/* One round of selection. With r = the header's `round` before the call:
 *
 *  1. Member m is READY iff board.episodes[m] - since[m] >= min_episodes and board.avg[m]
 *     is not NaN. R = the number of ready members.
 *  2. rank[m] of a ready m = the number of ready j with avg[j] > avg[m], or with avg[j] ==
 *     avg[m] and j < m: descending by avg, equal values (-0.0 == +0.0) by the lower index;
 *     +inf and -inf are ordinary values. rank_now[m] = rank[m], -1 for a member not ready.
 *  3. If R < 2 q nobody is replaced. Else the WINNERS are the members of rank < q and the
 *     LOSERS those of rank >= R - q; with 2 q <= R no member is both.
 *  4. For loser l: w[0..3] = Philox4x64-10 of counter (l, r, 0, 0) under key (seed,
 *     SACENV_SELECT_KEY1); j = ((w[0] >> 32) * q) >> 32 (a multiply-shift, no rejection: the
 *     bias is below q 2^-32); the source is the member of rank j.
 *  5. For k = 0..3: f = factor[(w[1] >> k) & 1], v = hp[source][k] * f (one f64 multiply),
 *     then `if (v < lo[k]) v = lo[k]; if (v > hi[k]) v = hi[k];` and hp[l][k] = v. The
 *     source's values are those from before the call: winners are never written.
 *  6. since[l] = board.episodes[l], replaced[l] += 1, parent[l] = source_now[l] = source;
 *     everyone else gets source_now = -1. Header: round += 1, replaced_total += losers.
 *  7. The loser's slab becomes its source's: all member_floats floats of weights +
 *     source * member_floats to weights + l * member_floats -- nets, target net, Adam
 *     moments and the kernels' fragment-order copies, so no sacenv_sac_pop_sync is needed.
 *
 * Two launches. The first is the decision: one wave, lane m for member m, ranks with a
 * 64-step compare loop over wave-shared values and writes the state. The second is the
 * copy, grid (chunks, members): the workgroups of a member whose source_now is < 0 exit at
 * once, the others move the slab with 16-B loads and stores. Sources are only read and
 * destinations only written, and by 3 no member is both.
 *
 * The hyper-parameters of sacenv_sac_pop_learn ride in its arguments, from host memory: the
 * caller reads the state back (hp of the members with source_now >= 0) and passes the new
 * values on, and captures again any graph that holds a learn with the old ones.
 *
 * Errors: SACENV_E_NULL (s, board, state or weights NULL), SACENV_E_SIZE (members, quantile,
 * lookback or min_episodes out of range, member_floats < 1 or no multiple of 4),
 * SACENV_E_RANGE (board, state or weights not 16-B aligned; a factor not finite or <= 0; a
 * range bound not finite, or lo[k] > hi[k]). */
int sacenv_select_step(const SacenvSelect *s, const void *board, void *state, float *weights, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SACENV_SELECTION_H */
