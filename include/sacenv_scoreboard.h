/*
 * sacenv_scoreboard.h — the population scoreboard: per-member scores, the look-back
 * average and the reference's save rule, kept on the device from the episode log.
 *
 * The reference keeps per model (main.py:99-108) a score history, the best score, the
 * mean of the last `avg_lookback` scores, and saves the model whenever an episode's score
 * beats that mean. A hyper-parameter search of P members on one env (member m owns envs
 * [env_base + m * envs_per_member, + envs_per_member)) shares one episode log
 * (sacenv_episodes.h). The entry points here consume the log's new entries per member,
 * apply exactly those lines and, optionally, copy the weights slab of every member the
 * rule selects into a snapshot buffer: the models the reference would have on disk.
 *
 * Conventions as in sacenv_episodes.h: device pointers, `b` is host memory read during
 * the call, `stream` a hipStream_t, every call only enqueues kernels (stream-ordered,
 * graph-capturable, nothing read back), every error is found on the host before anything
 * is launched; return 0, an SACENV_E_* code or a hipError_t. sacenv.h is untouched:
 * SACENV_ABI_VERSION does not count these.
 */
#ifndef SACENV_SCOREBOARD_H
#define SACENV_SCOREBOARD_H

#include "sacenv_episodes.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SACENV_SCOREBOARD_VERSION 1
#define SACENV_BOARD_MAX_MEMBERS 64
#define SACENV_BOARD_MAX_LOOKBACK 128   /* numpy sums up to 128 values in one unrolled block */
#define SACENV_BOARD_HEADER_BYTES 32
#define SACENV_BOARD_MEMBER_BYTES 128

typedef struct SacenvBoard {
  int32_t members;          /* P, 1 .. SACENV_BOARD_MAX_MEMBERS */
  int32_t envs_per_member;  /* >= 1 */
  int32_t env_base;         /* member 0's first env, as the log's entries number them (>= 0) */
  int32_t lookback;         /* L, 1 .. SACENV_BOARD_MAX_LOOKBACK (avg_lookback; the reference's default is 50) */
  int64_t cap;              /* entries the log can hold (SacenvEpisodeScan.cap) */
  int64_t member_floats;    /* stride of one member's slab in weights / snapshot, a multiple of 4;
                               0 = no snapshot */
} SacenvBoard;

/* The board (device, caller-owned, 16-B aligned, sacenv_board_bytes() bytes):
 *   header (32 B)
 *     int64 cursor   entries of the log seen since the log was last emptied (those past
 *                    cap included: it follows the log's total)
 *     int64 missed   entries that overflowed the log and were never seen, over all calls
 *     int64 calls    sacenv_board_update calls
 *     int64 0
 *   members x SacenvBoardMember (128 B each)
 *   members x lookback doubles: member m's last scores, episode i in slot i % lookback
 */
typedef struct SacenvBoardMember {
  int64_t episodes;         /* finished episodes seen */
  int64_t saves;            /* of them, those whose score beat the look-back mean */
  int64_t last_save_step;   /* end_step of the last such episode, -1 if none */
  int64_t last_end_step;    /* end_step of the last episode, -1 if none */
  double last;              /* the last episode's score (main.py's `Score`) */
  double best;              /* `Best Score`, -inf if none */
  double avg;               /* `Average Score`: the look-back mean after the last episode */
  uint32_t saved_now;       /* 1 if an episode among the LAST call's entries saved, else 0 */
  uint32_t reserved;
  uint64_t terms[8];        /* endings per term code; codes >= 7 are counted in slot 7 */
} SacenvBoardMember;

/* 32 + 128 members + 8 members lookback. Errors: SACENV_E_NULL, SACENV_E_SIZE. */
int sacenv_board_bytes(const SacenvBoard *b, int64_t *bytes);

/* One launch: the empty state (zero counters, -1 steps, best = -inf, zeroed rings). */
int sacenv_board_init(const SacenvBoard *b, void *board, void *stream);

/* Consume the log's new entries. With total = the log's header clamped to >= cursor, the
 * new entries are [min(cursor, cap), min(total, cap)): never one past cap, whatever the
 * header holds. missed grows by max(total, cap) - max(cursor, cap), cursor becomes total.
 * An entry belongs to member (env - env_base) / envs_per_member if that is in
 * [0, members) and is ignored otherwise. Per member, its entries in log order go through
 * main.py:99-108:
 *     history.append(score); avg = np.mean(history[-L:])
 *     if score > best: best = score           (a NaN score never becomes best)
 *     if score > avg:  saves += 1; last_save_step = end_step; saved_now = 1
 *     last = score; last_end_step = end_step; episodes += 1; terms[min(term, 7)] += 1
 * The mean is numpy's, bit for bit (its summation order for up to 128 values: a running
 * sum from -0.0 below 8 values, else eight accumulators over the multiple-of-eight part,
 * combined pairwise, the remainder added in order; that sum added to +0.0, so the mean of
 * negative zeros is +0.0 as np.mean's is; one IEEE divide), so `score > avg` is
 * the reference's decision, ties included. A mean that is NaN (a NaN score in the window,
 * or +inf and -inf) is stored as the quiet NaN 0x7FF8000000000000: IEEE 754 leaves a
 * generated NaN's sign to the hardware, and no score beats a NaN of either sign.
 *
 * Two launches. The first is one workgroup per member; no atomics, so the board's bytes
 * are the same from run to run. The second commits the header and, if weights, snapshot
 * and member_floats are all non-zero, copies weights + m * member_floats to snapshot +
 * m * member_floats (member_floats floats, 16-B loads and stores) for every member with
 * saved_now set; other members' slabs are not touched. The granularity is the CALL: the
 * snapshot holds the weights as they are when this call runs on the stream, not as they
 * were at the saving episode's step. Call it once per iteration, after the learn launches,
 * to snapshot where main.py:106-108 saves.
 *
 * Errors: SACENV_E_NULL (b, log or board NULL), SACENV_E_SIZE (members, lookback,
 * envs_per_member, env_base or cap out of range, member_floats negative or no multiple of
 * 4), SACENV_E_RANGE (log, board, weights or snapshot not 16-B aligned; exactly one of
 * weights / snapshot NULL with member_floats non-zero). */
int sacenv_board_update(const SacenvBoard *b, const void *log, void *board, const float *weights,
                        float *snapshot, void *stream);

/* cursor = 0: enqueue after the host has emptied the log (zeroed its total). */
int sacenv_board_rewind(const SacenvBoard *b, void *board, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SACENV_SCOREBOARD_H */
