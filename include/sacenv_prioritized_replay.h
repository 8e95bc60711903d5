/*
 * sacenv_prioritized_replay.h — proportional prioritized replay for a population: one
 * 64-ary sum tree per member, kept and sampled on the device.
 *
 * A population replay (sacenv_population_replay.h) samples member m's ring uniformly.
 * The calls here sample ring row i of member m with probability p_i / sum(p)
 * (Schaul, Quan, Antonoglou, Silver, "Prioritized Experience Replay", 2016, the
 * proportional variant), p_i following the row's last TD error. The replay arena is
 * untouched: its bytes stay those sacenv_population_replay.h describes. The priorities
 * live in a buffer of their own, and a sample is a draw on that buffer followed by the
 * population gather (sacenv_replay_pop_gather) on the arena.
 *
 * Integers throughout. A priority is a u32 in 16.16 fixed point (65 536 = 1.0), a node
 * sum a u64, a stratum and an offset integer arithmetic on Philox words: sums are
 * associative, any reduction order gives the same bytes, and the tree and every drawn
 * index can be restated bit for bit (tests/prio_oracle.py).
 *
 * The priority state (device, caller-owned, 256-B aligned): members slabs of
 * SacenvReplayPrioLayout.member_bytes each, member m's at state + m * member_bytes.
 * With M = p->mem_size, one slab is
 *
 *   header, 256 B        u64 total     sum of the member's leaves
 *                        u32 max_leaf  the largest leaf ever written; 65 536 at init
 *                        u32 0
 *                        i64 calls     device-counted samples (call == -1) so far
 *   level 0              u32 leaf[M]   at offset[0]
 *   level k >= 1         u64 [count[k]], count[k] = ceil(count[k-1] / 64), at offset[k]:
 *                        node i is the sum of entries [64 i, min(64 i + 64, count[k-1]))
 *                        of level k - 1
 *
 * Levels go on until one holds <= 64 entries (the top level; `total` is its sum), so M
 * <= 64 has leaves only and M = 1 000 000 has four levels (1 000 000, 15 625, 245, 4).
 * Every offset is a multiple of 256; bytes between the levels are zero. A leaf is 0
 * exactly for a ring row never stored; a stored row's leaf lies in [1, 2^31 - 1].
 *
 * Conventions as in sacenv_population_replay.h: device pointers unless noted, `p` and
 * `seeds` host memory read during the call, `stream` a hipStream_t, every call only
 * enqueues kernels (stream-ordered, graph-capturable, nothing read back), return 0, an
 * SACENV_E_* code or a hipError_t. There are no atomics: the same inputs give the same
 * bytes. sacenv.h, sacenv_population_replay.h and sacenv_population_share.h are
 * untouched: none of their version numbers counts these.
 *
 * Errors, all found on the host before anything is launched, in this order for every
 * call: SACENV_E_NULL for a NULL `p`; SACENV_E_SIZE for `p` refused by
 * sacenv_replay_layout's rules or members < 1 or > SACENV_REPLAY_POP_MAX_MEMBERS; then
 * the call's sizes and ranges in the order of its arguments (SACENV_E_SIZE for n < 0,
 * batch < 0 or member_stride < 0; SACENV_E_RANGE for cntr < -1, call < -1, alpha or eps
 * not finite or < 0, beta not finite or < 0); a call of no rows (n == 0, batch == 0)
 * then returns 0 without a launch; then SACENV_E_NULL for a NULL pointer where one is
 * not allowed; then SACENV_E_SIZE for a state or an arena that is not 256-B aligned, or
 * (the sample) a member's element count of one call >= 2^32.
 */
#ifndef SACENV_PRIORITIZED_REPLAY_H
#define SACENV_PRIORITIZED_REPLAY_H

#include "sacenv_population_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SACENV_REPLAY_PRIO_VERSION 1
#define SACENV_REPLAY_PRIO_MAX_LEVELS 6          /* mem_size < 2^31: 2^31, 2^25, 2^19, 2^13, 2^7, 2 */
#define SACENV_REPLAY_PRIO_HEADER_BYTES 256
#define SACENV_REPLAY_PRIO_ONE 65536u            /* priority 1.0 */
#define SACENV_REPLAY_PRIO_MAX_LEAF 0x7FFFFFFFu  /* 2^31 - 1 */
#define SACENV_REPLAY_PRIO_KEY1 0x7072696Full    /* second Philox key word ("prio"); the replay sampler's
                                                    is 0, the noise's SACENV_NOISE_KEY1, the selection's
                                                    SACENV_SELECT_KEY1 */

typedef struct SacenvReplayPrioLayout {
  int64_t member_bytes;                           /* one member's slab, a multiple of 256 */
  int64_t total_bytes;                            /* members x member_bytes */
  int32_t levels, pad;                            /* 1 .. SACENV_REPLAY_PRIO_MAX_LEVELS, 0 */
  int64_t count[SACENV_REPLAY_PRIO_MAX_LEVELS];   /* entries of level k; 0 above the top level */
  int64_t offset[SACENV_REPLAY_PRIO_MAX_LEVELS];  /* byte offset of level k in a slab */
} SacenvReplayPrioLayout;

int sacenv_replay_prio_layout(const SacenvReplayParams *p, int32_t members, SacenvReplayPrioLayout *out);

/* One launch: the empty state of every member (all leaves and nodes 0, total 0, max_leaf
 * SACENV_REPLAY_PRIO_ONE, calls 0). */
int sacenv_replay_prio_init(const SacenvReplayParams *p, int32_t members, void *state, void *stream);

/* The ring rows that sacenv_replay_pop_store(p, members, arena, cntr, n, ...) writes get
 * leaf = max_leaf (a new row is sampled at least once soon): rows (c0 + first + j) % M for
 * j in [0, min(n, M)), first = max(n - M, 0), the store's own rule, ring wrap included.
 * cntr >= 0: c0 = cntr, the rows every member held before the store, from the host (the
 * arena is not read and may be NULL). cntr == -1: c0 is member m's device count in the
 * arena, so THIS CALL MUST BE ENQUEUED BEFORE THE STORE IT DESCRIBES (the store advances
 * the count). Then the tree is repaired. At most three launches: the leaves, the level-1
 * nodes over the written rows, and levels >= 2 with the total, per member. */
int sacenv_replay_prio_mark_stored(const SacenvReplayParams *p, int32_t members, const void *arena, void *state,
                                   int64_t cntr, int64_t n, void *stream);

/* Explicit leaves: leaf[m][i], clamped to [1, SACENV_REPLAY_PRIO_MAX_LEAF], is written to
 * ring row idx[m][i] of member m. idx i64 [members][batch], leaf u32 [members][batch]. An
 * idx outside [0, M) is skipped. Where one member's batch names a row more than once, the
 * HIGHEST batch position wins (decided in LDS before anything is written, not by a racing
 * store). max_leaf becomes the maximum of its old value and the leaves written (the
 * winners, after the clamp). Then the tree is repaired: three launches, as above, the
 * level-1 nodes being those of the written rows. */
int sacenv_replay_prio_set(const SacenvReplayParams *p, int32_t members, void *state, int32_t batch,
                           const int64_t *idx, const uint32_t *leaf, void *stream);

/* Leaves from squared TD errors, then as sacenv_replay_prio_set. In f64,
 *   a = 0.5 (sqrt(sq1) + sqrt(sq2)) + eps     (td_sq2 == NULL: a = sqrt(sq1) + eps)
 *   leaf = clamp(floor(pow(a, alpha) x 65536), 1, SACENV_REPLAY_PRIO_MAX_LEAF)
 * A NaN `a` (a NaN or negative td_sq) gives 1 whatever alpha is, +inf the cap. td_sq1 /
 * td_sq2: f32, member m's [batch] values at td_sq + m * member_stride (member_stride in floats): views of the learn scratch of
 * sacenv_sac_pop_learn, where the learn leaves (q - q_hat)^2 of both critics per batch row
 * until the next learn (sacenv_replay_prio_learn_rows). */
int sacenv_replay_prio_update_td(const SacenvReplayParams *p, int32_t members, void *state, int32_t batch,
                                 const int64_t *idx, const float *td_sq1, const float *td_sq2,
                                 int64_t member_stride, double alpha, double eps, void *stream);

/* Where a learn leaves its per-row squared TD errors: the offsets, in floats from the start
 * of one agent's (member's) learn scratch, of the [batch] rows of critic 1 and critic 2, for
 * the batch of `sp`. A population's member m starts SacenvSacPopLayout.scratch_bytes / 4 x m
 * floats into the scratch. Errors: SACENV_E_NULL, SACENV_E_SIZE (`sp` refused by
 * sacenv_sac_layout's rules). */
int sacenv_replay_prio_learn_rows(const SacenvSacParams *sp, int64_t *td_sq1_off, int64_t *td_sq2_off);

/* A prioritized batch for every member: a draw launch on the state, then the population
 * gather launch on the arena (sacenv_replay_pop_gather). Member m draws from its own ring
 * only. idx i64 [members][batch]: the drawn ring rows, local to the member; leaf_out u32
 * [members][batch]: their leaves; both required. state / new_state / action / reward /
 * terminal as sacenv_replay_pop_sample's, any of which may be NULL. seeds: host memory,
 * u64 [members].
 *
 * The draw. For member m, slot j of B = batch, T = total_m, (q, r) = divmod(T, B):
 *   lo_j = q j + (r j) / B,  hi_j = q (j + 1) + (r (j + 1)) / B      (= floor(T j / B),
 *                                                  floor(T (j + 1) / B): no 128-bit product)
 *   w    = word 0 of Philox4x64-10 at counter (j, call, m, 0), key (seeds[m],
 *          SACENV_REPLAY_PRIO_KEY1)
 *   t    = lo_j + mulhi64(w, hi_j - lo_j)
 * then from the top level down: at each node the first child whose inclusive prefix sum
 * exceeds t is taken and its exclusive prefix is subtracted from t; the child of level 0 is
 * the row. mulhi64(w, width) is uniform on [0, width) up to a bias below width / 2^64 per
 * value (width <= 2^62: below 2^-2, in units of one part in 2^64 of the stratum -- far
 * under one leaf unit), as the selection's multiply-shift is. t < T always, so a row with
 * leaf 0 is never drawn; an empty stratum (T < B, hi_j == lo_j) draws t = lo_j. With T == 0
 * (nothing marked) every idx is -1 and every leaf_out 0, and the gather writes zero bits.
 *
 * call >= 0: the sample's number, from the host. call == -1: the state's `calls`, and one
 * more launch adds 1 to it afterwards (the store's convention for its count).
 *
 * weights (f32 [members][batch], may be NULL): (min_k leaf_k / leaf_j)^beta over member
 * m's batch, computed in f64 and rounded once: the importance weight (s p_j / T)^-beta
 * divided by the batch's largest, in which the stored rows s and T cancel. (0 where leaf_j
 * is 0.) Weights take the same launch as the count's advance: with weights == NULL and
 * call >= 0 the sample is two launches, else three. */
int sacenv_replay_prio_sample(const SacenvReplayParams *p, int32_t members, void *arena, void *state,
                              int32_t batch, int64_t call, const uint64_t *seeds, int64_t *idx,
                              uint32_t *leaf_out, float *weights, double beta, float *st, float *action,
                              double *reward, float *new_state, uint8_t *terminal, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SACENV_PRIORITIZED_REPLAY_H */
