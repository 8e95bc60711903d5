/*
 * sacenv_traces.h — episode traces: each member's best episode, step by step, kept on
 * the device from the step records.
 *
 * The reference writes every episode's rows to episodes/episode_<k>_data.csv
 * (postprocessing/recorder.py) and its replayer picks out the episodes that set a new
 * best (postprocessing/replayer.py:45-65). The episode log (sacenv_episodes.h) keeps an
 * episode's score and drops its steps; the scoreboard (sacenv_scoreboard.h) keeps the
 * best score per member. The entry points here keep what belongs to that score: the rows
 * of the episode that set it. They hold the recent steps of every env in a working store
 * and, when an episode ends with a score above its member's best, copy its rows into that
 * member's buffer.
 *
 * Conventions as in sacenv_episodes.h: device pointers, the descriptors are host memory
 * read during the call, `stream` a hipStream_t, every call only enqueues kernels (stream-
 * ordered, graph-capturable, nothing read back), every error is found on the host before
 * anything is launched; return 0, an SACENV_E_* code or a hipError_t. sacenv.h is
 * untouched: SACENV_ABI_VERSION does not count these.
 */
#ifndef SACENV_TRACES_H
#define SACENV_TRACES_H

#include "sacenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SACENV_TRACES_VERSION 1
#define SACENV_TRACES_MAX_MEMBERS 64
#define SACENV_TRACES_MAX_STEPS 1048576   /* the largest max_steps and call_steps */
#define SACENV_TRACE_HEADER_BYTES 64
#define SACENV_TRACE_ROW_BYTES 64
#define SACENV_TRACE_STEP_BYTES 52        /* the store's bytes per env and step */

typedef struct SacenvTraces {
  int32_t n_envs, n_pad;     /* n_pad a multiple of 64, n_envs <= n_pad */
  int32_t members;           /* P, 1 .. SACENV_TRACES_MAX_MEMBERS */
  int32_t envs_per_member;   /* the env at arena index e belongs to member e / envs_per_member; envs at or
                                past members x envs_per_member belong to nobody. With members > 1 a multiple
                                of 64: no wave straddles two members */
  int32_t env_base;          /* added to the env index in a header (a rank's first global env) */
  int32_t max_steps;         /* R >= 1: at most R + 1 rows of an episode are kept */
  int32_t call_steps;        /* Kmax >= 1: the largest n_steps an update passes */
  int32_t reserved;
  int64_t step0;             /* global number (>= 0) of the first step passed after sacenv_traces_init */
} SacenvTraces;

/* K consecutive steps, one update call. Step k's record starts at records + k * rec_stride;
 * inside it obs is f32 [n_pad][11] at obs_off, reward f32 [n_pad] at reward_off, done u8
 * [n_pad] at done_off and term u8 [n_pad] at term_off (the boat record of sacenv.h:
 * SACENV_REC_OBS / _REWARD / _DONE / _TERM x n_pad). Columns of envs >= n_envs are never
 * read. */
typedef struct SacenvTraceSteps {
  int32_t n_steps;           /* K, 1 .. call_steps */
  int32_t reserved;
  int64_t step;              /* global number of records row 0: step0 for the first call, then the
                                previous call's step + n_steps. Pass every step exactly once, in order */
  int64_t rec_stride;        /* bytes between consecutive steps' records (0 only with K == 1) */
  int64_t obs_off, reward_off, done_off, term_off;
  int64_t final_stride;      /* bytes between consecutive steps' final_obs (0 only with K == 1) */
} SacenvTraceSteps;

/* The member buffer (device, caller-owned, 16-B aligned): per member a SacenvTraceHeader
 * followed by max_steps + 1 rows of SACENV_TRACE_ROW_BYTES. */
typedef struct SacenvTraceHeader {
  int64_t end_step;          /* global step whose done byte ended the kept episode; -1 when empty */
  double score;              /* its score, exactly sacenv_episodes.h's: each record's f32 reward widened
                                to f64 and added in step order from +0.0; -inf when empty */
  int32_t env;               /* env_base + the env's arena index; -1 when empty */
  int32_t length;            /* L, steps of the episode */
  uint32_t term;             /* the ending step's term byte */
  int32_t rows;              /* rows kept: rows first_row .. length of the episode; 0 when empty */
  int32_t first_row;         /* leading rows that are missing */
  int32_t reserved0;
  int64_t replaced;          /* steps at which a new best was kept (see the rule) */
  int64_t reserved[2];       /* 0 */
} SacenvTraceHeader;

/* A row: obs f32 x 11 | action f32 | reward f32 | three zero words. Of an episode that ended
 * at global step t with length L:
 *   row 0           the episode's reset obs -- the record's obs at step t - L, the previous
 *                   episode's done step; for the episode in flight at sacenv_traces_init with
 *                   no step taken, init's obs -- with action 0 and reward 0 (BoatEnv.__init__'s
 *                   values, which the reference's first CSV row carries)
 *   row j, 0<j<L    the record's obs after the episode's j-th step (global step t - L + j),
 *                   with that step's action and reward
 *   row L           final_obs at step t, with the last step's action and reward
 * Kept are rows first_row .. L, first_row = max(L - R, c > 0 ? c + 1 : 0) with c the steps
 * the episode had taken before sacenv_traces_init (the carry's length): the last R + 1 rows,
 * and of an episode that began before the keeper was attached those whose step it saw.
 * Rows past `rows` are zero (a new best clears what a longer one before it left), so the
 * whole buffer, not only what a reader looks at, is the same however the steps are split
 * into calls.
 *
 * The rule, per member, over the endings of its envs in (end_step, env) order:
 *     if score > best: best = score, and keep that episode
 * which is the scoreboard's `best` (main.py:103), so the two agree bit for bit. A NaN score
 * never wins; a tie with the stored best replaces nothing; an empty member takes the first
 * score that is not NaN (-inf included: the stored score cannot tell, `rows` can). Of one
 * step's endings only the first greatest can be the one that stays, so the rule is applied
 * per step: `replaced` counts the steps at which the best changed, whatever way the steps
 * are split into calls. No atomics decide anything: the same inputs give the same bytes.
 *
 * The working store (device, 16-B aligned) is opaque; only its size is public. It holds
 * the last max_steps + call_steps steps of every env (SACENV_TRACE_STEP_BYTES per env and
 * step: the record's obs block, the action column and the reward column as the step wrote
 * them), the carry (f64 score, i32 length per env, as in sacenv_episodes.h but the keeper's
 * own) and the walk's per-wave results. */
int sacenv_traces_bytes(const SacenvTraces *t, int64_t *member_bytes, int64_t *store_bytes);

/* The empty state. obs: f32 [n_envs][11], every env's current obs (NULL: zeros); it fills
 * the slot before step0. carry_score f64 [n_envs] / carry_length i32 [n_envs]: each env's
 * episode in flight (NULL: zeros, every env at an episode's first step). One launch. */
int sacenv_traces_init(const SacenvTraces *t, const float *obs, const double *carry_score,
                       const int32_t *carry_length, void *member_buf, void *store, void *stream);

/* Append s->n_steps steps and keep each member's new best, if any. actions: f32 [K][n_envs];
 * final_obs: f32 [n_pad][11] per step, final_stride bytes apart, read only at the kept
 * episode's own (end step, env), where the step's done byte is set. Two launches: one wave
 * per 64 envs walks the steps with the carry in registers and copies every step into the
 * store; one workgroup per member picks the winner and, if it beats the stored score, copies
 * its rows out and writes the header last. Members without a winner touch nothing.
 *
 * Errors: SACENV_E_NULL (a NULL pointer), SACENV_E_SIZE (n_envs, n_pad, members,
 * envs_per_member, env_base, max_steps, call_steps or step0 out of range; n_pad no multiple
 * of 64; members > 1 with envs_per_member no multiple of 64; members x envs_per_member >
 * n_envs; n_steps < 1 or > call_steps), SACENV_E_RANGE (a negative offset or stride; step <
 * step0; records, actions, final_obs, obs_off, reward_off or -- with n_steps > 1 --
 * rec_stride or final_stride not 4-B aligned, or 0 with n_steps > 1; member_buf or store not
 * 16-B aligned). */
int sacenv_traces_update(const SacenvTraces *t, const SacenvTraceSteps *s, const void *records,
                         const float *actions, const void *final_obs, void *member_buf, void *store,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SACENV_TRACES_H */
