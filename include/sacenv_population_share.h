/*
 * sacenv_population_share.h — a population's replay buffers as one pool: part of
 * each member's batch drawn from all members' rings.
 *
 * A population replay (sacenv_population_replay.h) holds P rings as the slabs of
 * one arena, [P] x member_bytes, and member m samples its own ring. A stored row
 * is (obs, action, reward, obs', terminal) as the env wrote it -- a member's
 * reward_scale and gamma are applied in the learn, not at the store -- so every
 * row is training data for every member. The calls here draw `pool_rows` of the
 * `batch` rows of each member from the whole arena, in the two launches a
 * population sample takes. Nothing is copied or laid out again: a pooled draw is
 * an index computation and a gather across slabs.
 *
 * Semantics. B = batch, K = pool_rows, 0 <= K <= B, M = p->mem_size, P = members,
 * s = min(cntr_m, M) with cntr_m member m's own device count (the members store in
 * lockstep, so s is the same for all). Member m consumes its own MT19937 stream --
 * the key and position sacenv_replay_pop_sample uses -- as two consecutive legacy
 * numpy calls, in this order:
 *
 *   1. own = RandomState_m.choice(s, B - K)       ring rows of member m
 *   2. g   = RandomState_m.choice(P * s, K)       flat pool indices:
 *                                                 owner = g / s, row = g % s
 *
 * Both draws follow the rule of the one-buffer sample: masked rejection on 32-bit
 * words with rng = range - 1, the accepted words fill the output in order, the
 * stream stops after the last accepted word; a draw of size 0 consumes no words;
 * rng == 0 (s == 1 in the own draw; P == 1 and s == 1 in the pool draw) gives
 * zeros and consumes no words. The key is written back only if the draw passed a
 * 624-word block boundary.
 *
 * Outputs. idx i64 [P][B]; every entry is a GLOBAL row, owner x M + row: entries
 * [0, B - K) are the own rows (owner = m), entries [B - K, B) the pool rows. state
 * / new_state f32 [P][B][obs_dim], action f32 [P][B][act_dim], reward f64 [P][B],
 * terminal u8 [P][B] hold the rows at those global indices, taken from the owner's
 * slab; any of the five may be NULL (not written). A poisoned stream (position <
 * 0) draws nothing: its idx is -1, its rows are zero bits and the poison is kept,
 * as in sacenv_replay_pop_sample. A gather index outside [0, P x M) gives zero
 * bits. There are no atomics: the same inputs give the same bytes.
 *
 * Consequences. With K > 0 member m's batches depend on the other members' rows:
 * a member re-run alone reproduces its weights bit for bit only for K = 0. With K
 * = 0 the sample is sacenv_replay_pop_sample with idx offset by m x M: the gathered
 * bytes and the arena bytes afterwards are identical. members == 1 is legal: the
 * pool is the member's own ring, and the draw is still the two choice calls.
 *
 * Conventions as in sacenv_population_replay.h: device pointers, `stream` a
 * hipStream_t, every call only enqueues kernels (the sample a draw and a gather
 * launch, the gather one launch; stream-ordered, graph-capturable), return 0, an
 * SACENV_E_* code or a hipError_t. sacenv.h and sacenv_population_replay.h are
 * untouched: neither SACENV_ABI_VERSION nor SACENV_REPLAY_POP_VERSION counts these.
 *
 * Errors, all found on the host before anything is launched, in this order: the
 * family's rules as sacenv_population_replay.h states them -- SACENV_E_NULL for a
 * NULL `p`, SACENV_E_SIZE for `p` refused by sacenv_replay_layout's rules or
 * members < 1 or > SACENV_REPLAY_POP_MAX_MEMBERS, SACENV_E_SIZE for batch < 0,
 * SACENV_E_SIZE for stored <= 0 (the sample), SACENV_E_NULL for a NULL arena or
 * idx, SACENV_E_SIZE for an arena that is not 256-B aligned or a member's element
 * count of one call >= 2^32 -- then SACENV_E_SIZE for pool_rows < 0 or pool_rows >
 * batch (the sample), then SACENV_E_SIZE for members x mem_size > 2^32 (numpy would
 * leave the 32-bit word path there, and a global row is a 32-bit number in the
 * gather). batch == 0 then returns 0 without a launch.
 */
#ifndef SACENV_POPULATION_SHARE_H
#define SACENV_POPULATION_SHARE_H

#include "sacenv_population_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SACENV_REPLAY_SHARE_VERSION 1

/* The pooled sample of every member in two launches (a draw and a gather). `stored`
 * is the host's count, read only for the error above. */
int sacenv_replay_pop_sample_pool(const SacenvReplayParams *p, int32_t members, void *arena,
                                  int32_t batch, int32_t pool_rows, int64_t stored, int64_t *idx,
                                  float *state, float *action, double *reward, float *new_state,
                                  uint8_t *terminal, void *stream);

/* The rows at the global indices idx [members][batch], for every member, in one
 * launch: row idx % mem_size of slab idx / mem_size; an index outside [0, members x
 * mem_size) gives zero bits. */
int sacenv_replay_pop_gather_pool(const SacenvReplayParams *p, int32_t members, void *arena,
                                  int32_t batch, const int64_t *idx, float *state, float *action,
                                  double *reward, float *new_state, uint8_t *terminal, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SACENV_POPULATION_SHARE_H */
