/*
 * sacenv_population.h — a population of SAC agents: act and learn for P
 * members in one set of launches.
 *
 * The reference's hyper-parameter search (main.py -p N, main.py:215-235) trains N
 * agents that differ in four numbers -- the actor and critic learning rates,
 * gamma and tau, drawn by utils/hyperparameter_tuner.py:20-43 -- as OS processes,
 * three at a time. Here the P agents share one weights buffer ([P] slabs, each
 * laid out as sacenv_sac_layout lays out one agent) and the kernels of
 * sacenv_sac_learn / sacenv_sac_act run with a second grid dimension over the
 * members: 4 learn launches and 1 act launch for the whole population. Member m
 * computes exactly what sacenv_sac_learn / sacenv_sac_act compute for one agent
 * with member m's hyper-parameters on member m's slab: the same device code on the
 * same f32 scalars, in the same order, so the results are equal bit for bit.
 *
 * Conventions as in sacenv.h: device pointers unless noted, `stream` a
 * hipStream_t, every call only enqueues kernels (stream-ordered, graph-
 * capturable), return 0, an SACENV_E_* code or a hipError_t. sacenv.h is
 * untouched: SACENV_ABI_VERSION does not count these.
 */
#ifndef SACENV_POPULATION_H
#define SACENV_POPULATION_H

#include "sacenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SACENV_POPULATION_VERSION 1
#define SACENV_SAC_POP_MAX_MEMBERS 64   /* six f32 per member ride in the kernel arguments (< 4 KB) */

/* What one member's learn() has of its own (host memory, 40 B). */
typedef struct SacenvSacMember {
  double lr_actor, lr_critic, gamma, tau, reward_scale;
} SacenvSacMember;

typedef struct SacenvSacPopLayout {
  int64_t member_floats;   /* weights stride: SacenvSacLayout.total_floats rounded up to 4 floats */
  int64_t scratch_bytes;   /* per member: SacenvSacLayout.scratch_bytes rounded up to 16 */
  int64_t total_floats, total_scratch_bytes;   /* members x the strides */
  int32_t max_members, pad;                    /* SACENV_SAC_POP_MAX_MEMBERS, 0 */
} SacenvSacPopLayout;

/* `p` carries what the members share: obs_dim, n_actions, hidden, batch,
 * max_action and Adam's betas and eps; its lr_*, gamma, tau and reward_scale are
 * not read by sacenv_sac_pop_learn. Member m's weights are the member_floats
 * floats at weights + m * member_floats (inside: sacenv_sac_layout's offsets), its
 * scratch the scratch_bytes bytes at scratch + m * scratch_bytes.
 *
 * Errors, all found on the host before anything is launched: SACENV_E_NULL (a
 * NULL pointer; log_prob and losses may be NULL), SACENV_E_SIZE (members < 1 or
 * > SACENV_SAC_POP_MAX_MEMBERS, `p` refused by sacenv_sac_layout's rules -- the
 * act entry point ignores p->batch, as sacenv_sac_act does --, n < 0, weights or
 * scratch not 16-B aligned), SACENV_E_RANGE (adam_step < 1). */
int sacenv_sac_pop_layout(const SacenvSacParams *p, int32_t members, SacenvSacPopLayout *out);

/* sacenv_sac_sync for every member (after a host write to the weights). */
int sacenv_sac_pop_sync(const SacenvSacParams *p, int32_t members, float *weights, void *stream);

/* sacenv_sac_act for every member in one launch: member m acts on its own n rows.
 * obs f32 [members][n][obs_dim], eps / action / log_prob f32 [members][n].
 * n == 0 returns 0 without a launch. */
int sacenv_sac_pop_act(const SacenvSacParams *p, int32_t members, const float *weights,
                       const float *obs, int32_t n, const float *eps, float *action,
                       float *log_prob, void *stream);

/* sacenv_sac_learn for every member in four launches (the members learn in
 * lockstep: one adam_step). hp: host memory, [members], read during the call.
 * state / new_state f32 [members][batch][obs_dim]; action, eps1, eps2 f32, reward
 * f64, done u8, each [members][batch]; losses f32 [members][4] (value, actor,
 * critic 1, critic 2) or NULL. With members == 1 the launches are sacenv_sac_learn's own,
 * with hp[0]'s values. */
int sacenv_sac_pop_learn(const SacenvSacParams *p, int32_t members, const SacenvSacMember *hp,
                         float *weights, void *scratch, const float *state, const float *action,
                         const double *reward, const float *new_state, const uint8_t *done,
                         const float *eps1, const float *eps2, int32_t adam_step, float *losses,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SACENV_POPULATION_H */
