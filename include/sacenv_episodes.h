/*
 * sacenv_episodes.h — the episode log: score, length and end of every finished
 * episode, scanned on the device from the step records (no host round trip).
 *
 * The reference's training loop is built around finished episodes (main.py:70-114:
 * `score += reward` per step, `score_history.append(score)`, the best score and
 * the look-back average, how the episode ended). The vectorised envs of sacenv.h
 * restart inside the step launch, so an episode's score is gone one ending later
 * (layout.final_ep_reward keeps each env's LAST one only). This entry point reads
 * the packed per-step records those launches already write -- the records of
 * sacenv_boat_rollout, the arena's record after one step, a toy arena's record --
 * and appends one entry per finished episode to a device log, in chronological
 * order. No step kernel takes part: the scan runs beside them.
 *
 * Conventions as in sacenv.h: device pointers, `s` is host memory read during
 * the call, `stream` a hipStream_t, every call only enqueues kernels (stream-
 * ordered, graph-capturable, nothing read back), return 0, an SACENV_E_* code or
 * a hipError_t. sacenv.h is untouched: SACENV_ABI_VERSION does not count these.
 */
#ifndef SACENV_EPISODES_H
#define SACENV_EPISODES_H

#include "sacenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SACENV_EPISODES_VERSION 1
#define SACENV_EPISODE_ENTRY_BYTES 32   /* one log entry; the log's header has the same size */

/* K consecutive steps' records and where their columns are. Step k's record
 * starts at records + k * rec_stride; inside it, reward is f32 [n_pad] at
 * reward_off, done u8 [n_pad] at done_off, term u8 [n_pad] at term_off:
 *   boat record (SACENV_RECORD_BYTES x n_pad): SACENV_REC_REWARD / _DONE / _TERM x n_pad
 *   toy record (14 n_pad):                      8 n_pad, 12 n_pad, 13 n_pad
 * Columns of envs >= n_envs are never read (a rollout leaves them uninitialised). */
typedef struct SacenvEpisodeScan {
  int32_t n_envs, n_pad;        /* n_pad a multiple of 64, n_envs <= n_pad */
  int32_t n_steps;              /* K >= 1 */
  int32_t env_base;             /* added to the env index (a rank's first global env) */
  int64_t rec_stride;           /* bytes between consecutive steps' records (0 only with K == 1) */
  int64_t reward_off, done_off, term_off;   /* byte offsets of the columns inside one record */
  int64_t step0;                /* global step number of records row 0 */
  int64_t cap;                  /* entries the log can hold */
} SacenvEpisodeScan;

/* One finished episode (SACENV_EPISODE_ENTRY_BYTES, 16-B aligned):
 *   int64  end_step   step0 + k of the step whose done byte was set
 *   double score      the episode's rewards, each record's f32 widened to f64 and added
 *                     in step order from +0.0 (main.py:74,82)
 *   int32  env        env_base + the env's index in the arena
 *   int32  length     steps of the episode
 *   uint32 term       the step's term byte (SACENV_TERM_* / toy codes)
 *   uint32 reserved   0
 *
 * log:   a 32-B header -- int64 total: entries found since the host last zeroed it,
 *        those that did not fit included; the other 24 bytes are not touched --
 *        followed by cap entries. A call appends at `total` and advances it on the
 *        device; entries whose position is >= cap are written nowhere and still
 *        counted, so total > cap says the log overflowed. Entries are ascending by
 *        (end_step, env) within a call, and calls append in the order issued; the
 *        positions come from counts and a prefix sum, never from atomics, so the
 *        log's bytes are the same from run to run.
 * carry: f64 [n_pad] score so far, then i32 [n_pad] steps so far, of each env's
 *        episode in flight (8-B aligned; zero = at an episode's first step). Read
 *        and written by every call: pass every step exactly once, in order.
 * scratch: 16-B aligned device buffer of sacenv_episodes_scratch_bytes() bytes for
 *        this n_steps and n_pad (16 B per step and 64 envs); no contents kept. */
int sacenv_episodes_scratch_bytes(const SacenvEpisodeScan *s, int64_t *bytes);

/* Scan n_steps records: three launches (count the endings per step and 64 envs;
 * exclusive scan of the counts in step-major order, which also advances the log's
 * total; walk the steps again with the carry in registers and write the entries).
 * Errors, all found on the host before anything is launched: SACENV_E_NULL (a NULL
 * pointer), SACENV_E_SIZE (n_envs, n_pad, n_steps, env_base or cap out of range,
 * n_pad no multiple of 64, n_steps x n_pad / 64 >= 2^31, scratch too small),
 * SACENV_E_RANGE (a negative offset or stride, reward_off, records or -- with
 * n_steps > 1 -- rec_stride not 4-B aligned, rec_stride == 0 with n_steps > 1,
 * carry not 8-B or log / scratch not 16-B aligned). */
int sacenv_episodes_update(const SacenvEpisodeScan *s, const void *records, void *carry,
                           void *log, void *scratch, int64_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SACENV_EPISODES_H */
