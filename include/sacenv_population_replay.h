/*
 * sacenv_population_replay.h — the replay buffers of a population: store and
 * sample for P members in one set of launches.
 *
 * A population (sacenv_population.h) learns from P buffers, one per member
 * (agent/buffer.py:3-35 each, on its own np.random stream). Here the P buffers
 * are the slabs of one arena ([P] x member_bytes, each laid out as
 * sacenv_replay_layout lays out one buffer) and the kernels of
 * sacenv_replay_store_env / sacenv_replay_sample / sacenv_replay_gather run
 * with a second grid dimension over the members: one store launch, and a draw and
 * a gather launch per sample, for the whole population. The sampled batches come
 * out as [members][batch][...], the tensors sacenv_sac_pop_learn reads.
 *
 * Contract: member m's member_bytes at arena + m * member_bytes are, after any
 * sequence of these calls, the bytes a sacenv_replay_* arena holds after the same
 * calls with member m's rows and seed (the same device code on the same values),
 * and member m's outputs are that arena's outputs.
 *
 * The members store in lockstep: n rows each per call, one count for all. With
 * members == 1 the launches are the one-buffer entry points' own.
 *
 * Conventions as in sacenv.h: device pointers unless noted, `stream` a
 * hipStream_t, every call only enqueues kernels (stream-ordered, graph-
 * capturable), return 0, an SACENV_E_* code or a hipError_t. sacenv.h is
 * untouched: SACENV_ABI_VERSION does not count these.
 *
 * Errors, all found on the host before anything is launched: SACENV_E_NULL (a
 * NULL pointer where one is not allowed), SACENV_E_SIZE (members < 1 or >
 * SACENV_REPLAY_POP_MAX_MEMBERS, `p` refused by sacenv_replay_layout's rules, n < 0
 * or batch < 0, stored <= 0 for a sample, a member's element count of one call >=
 * 2^32, an arena that is not 256-B aligned), SACENV_E_RANGE (cntr < -1). The member
 * count is checked before the rows; n == 0 and batch == 0 return 0 without a launch.
 */
#ifndef SACENV_POPULATION_REPLAY_H
#define SACENV_POPULATION_REPLAY_H

#include "sacenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SACENV_REPLAY_POP_VERSION 1
#define SACENV_REPLAY_POP_MAX_MEMBERS 64   /* one u32 seed per member rides in the init kernel's arguments */

typedef struct SacenvReplayPopLayout {
  int64_t member_bytes;      /* = SacenvReplayLayout.total_bytes (a multiple of 256) */
  int64_t total_bytes;       /* members x member_bytes */
  int32_t max_members, pad;  /* SACENV_REPLAY_POP_MAX_MEMBERS, 0 */
} SacenvReplayPopLayout;

int sacenv_replay_pop_layout(const SacenvReplayParams *p, int32_t members, SacenvReplayPopLayout *out);

/* sacenv_replay_init for every member in one launch. seeds: host memory,
 * [members], read during the call. */
int sacenv_replay_pop_init(const SacenvReplayParams *p, int32_t members, void *arena,
                           const uint32_t *seeds, void *stream);

/* n rows for every member. state / new_state / final_state f32
 * [members][n][obs_dim], action f32 [members][n][act_dim], reward f32 or f64
 * (p->reward_f32) [members][n], code u8 [members][n], last_term u8 [members][n]
 * in/out; final_state and last_term may be NULL (sacenv_replay_store_env's rules).
 * cntr >= 0: the rows every member held before this call, from the host: one
 * launch (sacenv_replay_store_env_at's rule). cntr == -1: the device counts, a
 * store and an advance launch (graph-safe, sacenv_replay_store_env). */
int sacenv_replay_pop_store(const SacenvReplayParams *p, int32_t members, void *arena, int64_t cntr,
                            int64_t n, const float *state, const float *action, const void *reward,
                            const float *new_state, const float *final_state, const uint8_t *code,
                            uint8_t *last_term, void *stream);

/* sacenv_replay_sample for every member in two launches: member m draws `batch`
 * indices from its own stream at its device count and gathers its rows. idx i64
 * [members][batch] (required); state / new_state f32 [members][batch][obs_dim],
 * action f32 [members][batch][act_dim], reward f64, terminal u8 [members][batch],
 * any of which may be NULL (not written). `stored` is the host's count, read only
 * for the error above. */
int sacenv_replay_pop_sample(const SacenvReplayParams *p, int32_t members, void *arena, int32_t batch,
                             int64_t stored, int64_t *idx, float *state, float *action, double *reward,
                             float *new_state, uint8_t *terminal, void *stream);

/* sacenv_replay_gather for every member in one launch: the rows at idx
 * [members][batch]; an index outside the ring gives zero bits. */
int sacenv_replay_pop_gather(const SacenvReplayParams *p, int32_t members, void *arena, int32_t batch,
                             const int64_t *idx, float *state, float *action, double *reward,
                             float *new_state, uint8_t *terminal, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SACENV_POPULATION_REPLAY_H */
