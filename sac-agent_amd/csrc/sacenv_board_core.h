// sacenv_board_core.h — what the scoreboard kernels (sacenv_board.hip) share: the board's
// layout and numpy's mean of up to 128 doubles. Plain C++ outside hipcc, so the mean can be
// compiled for the host and held against numpy there (tests/test_scoreboard_cpu.py).
#ifndef SACENV_BOARD_CORE_H
#define SACENV_BOARD_CORE_H

#include <stdint.h>

#include "sacenv_scoreboard.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SACENV_BOARD_HD __host__ __device__ __forceinline__
#else
#define SACENV_BOARD_HD inline
#endif

namespace sacenv_board {

constexpr int kMaxL = SACENV_BOARD_MAX_LOOKBACK;
constexpr int kHeaderWords = SACENV_BOARD_HEADER_BYTES / 8;   // the board as 8-B words
constexpr int kMemberWords = SACENV_BOARD_MEMBER_BYTES / 8;

static_assert(sizeof(SacenvBoardMember) == SACENV_BOARD_MEMBER_BYTES, "the member record is 128 B");
static_assert(sizeof(SacenvBoard) == 32, "SacenvBoard is 32 B");

SACENV_BOARD_HD int64_t board_bytes(int64_t members, int64_t lookback) {
  return SACENV_BOARD_HEADER_BYTES + members * (SACENV_BOARD_MEMBER_BYTES + 8 * lookback);
}

// np.mean of p[0 .. n), 1 <= n <= 128, in numpy's own order (one block of its pairwise sum,
// added to add.reduce's +0.0 start), needs -ffp-contract=off:
//   n < 8   a running sum from -0.0
//   else    eight accumulators from the first eight values, each taking every eighth value
//           of the multiple-of-eight part; ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)); the last
//           n mod 8 values added in order
// then 0.0 + that sum (it shows in one case only: a sum of -0.0 becomes +0.0, as np.mean of
// negative zeros is) and one correctly rounded divide by n.
SACENV_BOARD_HD double mean_np(const double* p, const int n) {
  double res;
  if (n < 8) {
    res = -0.0;
    for (int i = 0; i < n; ++i) res = res + p[i];
  } else {
    double r0 = p[0], r1 = p[1], r2 = p[2], r3 = p[3], r4 = p[4], r5 = p[5], r6 = p[6], r7 = p[7];
    const int whole = n - n % 8;
    int i = 8;
    for (; i < whole; i += 8) {
      r0 = r0 + p[i];
      r1 = r1 + p[i + 1];
      r2 = r2 + p[i + 2];
      r3 = r3 + p[i + 3];
      r4 = r4 + p[i + 4];
      r5 = r5 + p[i + 5];
      r6 = r6 + p[i + 6];
      r7 = r7 + p[i + 7];
    }
    res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res = res + p[i];
  }
  res = 0.0 + res;
  return res / (double)n;
}

}  // namespace sacenv_board

#endif  // SACENV_BOARD_CORE_H
