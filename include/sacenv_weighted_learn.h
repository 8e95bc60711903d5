/*
 * sacenv_weighted_learn.h — importance weights of a prioritized sample, applied in the
 * critic loss, and their exponent annealed on the device.
 *
 * A prioritized replay (sacenv_prioritized_replay.h) draws row i with probability
 * p_i / sum(p) and computes the correction weights w = (min leaf / leaf)^beta of every
 * batch (Schaul, Quan, Antonoglou, Silver, "Prioritized Experience Replay", 2016, §3.4).
 * The two learn calls here take those weights, per batch row, into the critics' TD loss;
 * the sample here computes them with an exponent that runs from beta0 to beta1 over a
 * number of samples, derived from the sample's own number, so that a captured graph
 * anneals with no host in the loop.
 *
 * Arithmetic of the weighted learn. With row_weights == NULL every launch and every byte
 * is that of sacenv_sac_learn / sacenv_sac_pop_learn. With row_weights != NULL, w_r the
 * weight of batch row r, d = q - q_hat the row's TD error of one critic, B the batch:
 *
 *   what                                         unweighted        weighted
 *   per-row gradient of the critic's head        g = d * (1 / B)   g = (w_r * d) * (1 / B)
 *   per-row squared TD error in the scratch      d * d             d * d   (unchanged, raw)
 *   per-thread partial sums of the critic losses s += v[r]         s += w_r * v[r]
 *   losses[2], losses[3]                         0.5 mean(d^2)     0.5 mean(w d^2): the sum
 *                                                                  divided by B, not by sum(w)
 *
 * The rows that sacenv_replay_prio_learn_rows names stay raw because the priority update
 * reads them. The value loss, the actor loss and their gradients are untouched. Weights
 * are taken as they are: finite and >= 0 expected, not checked. The scratch layout, its
 * size and every offset in it are those of the unweighted calls.
 *
 * Conventions as in sacenv_population.h: device pointers unless noted, `stream` a
 * hipStream_t, every call only enqueues kernels (stream-ordered, graph-capturable), errors
 * found on the host before anything is launched, return 0, an SACENV_E_* code or a
 * hipError_t. sacenv.h, sacenv_population.h and sacenv_prioritized_replay.h are untouched:
 * none of their version numbers counts these.
 */
#ifndef SACENV_WEIGHTED_LEARN_H
#define SACENV_WEIGHTED_LEARN_H

#include "sacenv_population.h"
#include "sacenv_prioritized_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SACENV_WEIGHTED_LEARN_VERSION 1

/* sacenv_sac_learn with a weight per batch row: row_weights f32 [batch], or NULL for
 * sacenv_sac_learn's own launches and bytes. Errors as sacenv_sac_learn's, in its order. */
int sacenv_sac_learn_weighted(const SacenvSacParams *p, float *weights, void *scratch, const float *state,
                              const float *action, const double *reward, const float *new_state,
                              const uint8_t *done, const float *eps1, const float *eps2, int32_t adam_step,
                              float *losses, const float *row_weights, void *stream);

/* sacenv_sac_pop_learn with a weight per member and batch row: row_weights f32
 * [members][batch] (member m reads row_weights + m * batch), or NULL for
 * sacenv_sac_pop_learn's own launches and bytes. With members == 1 the launches are the one
 * agent's, as there. Errors as sacenv_sac_pop_learn's, in its order. */
int sacenv_sac_pop_learn_weighted(const SacenvSacParams *p, int32_t members, const SacenvSacMember *hp,
                                  float *weights, void *scratch, const float *state, const float *action,
                                  const double *reward, const float *new_state, const uint8_t *done,
                                  const float *eps1, const float *eps2, int32_t adam_step, float *losses,
                                  const float *row_weights, void *stream);

/* sacenv_replay_prio_sample with the weights' exponent annealed: in f64,
 *   beta_k = beta0 + (beta1 - beta0) * (min(k, anneal_calls) / anneal_calls)
 * (the quotient first, then the product, then the sum: three roundings in this order), k being
 * the sample's number: `call` when call >= 0, else the state's `calls` BEFORE this
 * sample's advance. The draw, idx, leaf_out and the number of launches (two or three) are
 * the plain sample's; beta0 == beta1 gives the plain sample's bytes.
 * Errors, in this order: those of the plain sample up to `call` (SACENV_E_RANGE for call <
 * -1); SACENV_E_RANGE for beta0 or beta1 not finite or < 0; SACENV_E_RANGE for anneal_calls
 * < 1; the rest as the plain sample. */
int sacenv_replay_prio_sample_annealed(const SacenvReplayParams *p, int32_t members, void *arena, void *state,
                                       int32_t batch, int64_t call, const uint64_t *seeds, int64_t *idx,
                                       uint32_t *leaf_out, float *weights, double beta0, double beta1,
                                       int64_t anneal_calls, float *st, float *action, double *reward,
                                       float *new_state, uint8_t *terminal, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SACENV_WEIGHTED_LEARN_H */
