/*
 * sacenv_noise.h — counter-based policy noise: the standard normal draws of
 * choose_action and learn for every member of a population, in one launch.
 *
 * The agents draw one normal per acting row (agent/continuous_agent.py:57-61,
 * the actor's sample_normal) and two per batch row of a learn
 * (continuous_agent.py:113,127). Drawn from one process-wide stream, the noise a
 * member sees depends on how many members there are and on everything else that
 * used the stream. Here every draw is a pure function of (the member's seed, the
 * stream that names the use, the call, the element), as the staged replay's
 * draws are (sacenv_replay_stage_draw_ctr): member m of a population computes
 * what a stand-alone agent with member m's seed computes, bit for bit.
 *
 * The contract. Element i >= 0 of call c of stream s under seed S:
 *   w[0..3] = Philox4x64-10 of counter (i div 4, c, s, 0), key (S, SACENV_NOISE_KEY1)
 *             (the replay sampler's blocks have key (seed, 0));
 *   p  = (i mod 4) div 2;
 *   u1 = ((w[2p] >> 11) + 1) * 2^-53   in (0, 1],
 *   u2 = (w[2p+1] >> 11) * 2^-53       in [0, 1)       (both exact in f64);
 *   r  = sqrt(-2 log(u1));
 *   z  = r * cospi(2 u2) for even i, r * sinpi(2 u2) for odd i   (all in f64, the
 *        product a plain multiply);
 *   the value is (float)z.
 * No value is infinite or NaN: |z| <= sqrt(106 ln 2) < 8.58. tests/noise_oracle.py
 * restates this in numpy and in mpmath.
 *
 * Streams: 0 the act draw, 1 and 2 the first and second noise of a learn; any
 * 64-bit value is a stream of its own.
 *
 * Conventions as in sacenv.h: `stream` (the last argument) a hipStream_t, the
 * call only enqueues one kernel (stream-ordered, graph-capturable; the seeds and
 * the descriptors are read during the call and ride in the kernel's arguments:
 * no copy, no device-side state), return 0, an SACENV_E_* code or a hipError_t.
 * sacenv.h is untouched: SACENV_ABI_VERSION does not count this.
 *
 * Errors, all found on the host before anything is launched, in this order:
 * SACENV_E_SIZE (members < 1 or > SACENV_NOISE_MAX_MEMBERS, n_draws < 1 or >
 * SACENV_NOISE_MAX_STREAMS), SACENV_E_NULL (seeds or draws NULL), then per draw
 * SACENV_E_SIZE (calls < 1, n < 0, calls x members x n >= 2^31), SACENV_E_NULL
 * (out NULL with n > 0), SACENV_E_SIZE (out not 4-B aligned). A draw with n == 0
 * writes nothing; a call whose draws are all empty launches nothing and returns 0.
 */
#ifndef SACENV_NOISE_H
#define SACENV_NOISE_H

#include "sacenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SACENV_NOISE_VERSION 1
#define SACENV_NOISE_MAX_MEMBERS 64   /* one u64 seed per member rides in the kernel's arguments */
#define SACENV_NOISE_MAX_STREAMS 4    /* draws of one call */
#define SACENV_NOISE_KEY1 0x6E6F697365ull   /* second Philox key word ("noise") */
#define SACENV_NOISE_ACT 0
#define SACENV_NOISE_LEARN1 1
#define SACENV_NOISE_LEARN2 2

typedef struct SacenvNoiseDraw {       /* host memory */
  uint64_t stream, first_call;         /* rows are calls first_call, first_call + 1, ... */
  int32_t calls, n;                    /* calls >= 1 rows of n >= 0 values per member */
  float *out;                          /* device, f32 [calls][members][n] */
} SacenvNoiseDraw;

/* The n_draws draws for every member in one launch: draws[d].out[k][m][i] =
 * element i of call draws[d].first_call + k of stream draws[d].stream under
 * seeds[m]. seeds: host memory, [members]; draws: host memory, [n_draws]. */
int sacenv_noise_normal(int32_t members, const uint64_t *seeds, int32_t n_draws,
                        const SacenvNoiseDraw *draws, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SACENV_NOISE_H */
