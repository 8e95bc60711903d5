// sacenv_board.hip — gfx950 population scoreboard (include/sacenv_scoreboard.h): main.py:99-108
// per member, from the episode log (include/sacenv_episodes.h), of which it needs the size of
// the header and of an entry and nothing else.
//
//   k_board_update  one workgroup of 1 024 lanes per member. It walks the log's new entries
//                   2 048 at a time (two per lane, the next round's loads issued before this
//                   round is worked on), keeps its own by ballot + mbcnt + the waves' counts
//                   in log order, and appends their scores to a window in LDS that starts
//                   with the member's last 128 scores. Entry r is then judged by lane r: its
//                   look-back mean is read from the window alone -- the decision for an
//                   episode depends on the scores before it, never on earlier decisions --
//                   so a round's entries are judged side by side. Each lane keeps its own
//                   saves, best, last save and term counts; they are reduced once, at the
//                   end, with the entry's index as the tie-break (the order of the
//                   reduction cannot show). All P workgroups read all new entries (32 B
//                   each, out of L2).
//   k_board_finish  thread 0 commits the header (cursor, missed, calls), which the update
//                   launch's workgroups all read; with a snapshot, workgroups (chunk, m)
//                   copy member m's slab if its saved_now is set and exit otherwise.
// No atomics: the board's bytes are the same from run to run.

#include "sacenv_board_core.h"
#include "sacenv_scoreboard.h"
#include "sacenv_wave_core.h"

namespace {

using namespace sacenv_board;

constexpr int kBoardThreads = 1024;
constexpr int kBoardWaves = kBoardThreads / kWave;
constexpr int kBoardPer = 2;                              // entries per lane and round
constexpr int kBoardRound = kBoardPer * kBoardThreads;
constexpr int kCopyThreads = 256;
constexpr int kCopyChunks = 64;                           // at most this many workgroups per member's slab

struct Board {
  const char* log;
  char* board;
  int64_t cap;
  int32_t members, epm, env_base, lookback;
};

// the log's new entries [lo, hi) and its total as the board takes it (>= the cursor)
__device__ __forceinline__ void board_window(const Board& a, int64_t& lo, int64_t& hi, int64_t& cursor,
                                             int64_t& total) {
  cursor = *reinterpret_cast<const int64_t*>(a.board);
  if (cursor < 0) cursor = 0;
  total = *reinterpret_cast<const int64_t*>(a.log);
  if (total < cursor) total = cursor;
  lo = cursor < a.cap ? cursor : a.cap;
  hi = total < a.cap ? total : a.cap;
}

__device__ __forceinline__ SacenvBoardMember* board_member(const Board& a, const int m) {
  return reinterpret_cast<SacenvBoardMember*>(a.board + SACENV_BOARD_HEADER_BYTES) + m;
}

__global__ __launch_bounds__(kBoardThreads) void k_board_update(const Board a) {
  __shared__ double hist[kMaxL + kBoardRound];   // [0, 128): the scores before this round, the latest at 127
  __shared__ int64_t ends[kBoardRound];
  __shared__ uint8_t terms[kBoardRound];
  __shared__ uint32_t wcnt[kBoardPer][kBoardWaves];
  __shared__ double last_score, last_avg;
  __shared__ int64_t last_end;
  __shared__ uint32_t w_saves[kBoardWaves], w_terms[kBoardWaves][8];
  __shared__ double w_best[kBoardWaves];
  __shared__ int64_t w_best_at[kBoardWaves], w_save_at[kBoardWaves], w_save_step[kBoardWaves];

  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  const int m = blockIdx.x, L = a.lookback;
  SacenvBoardMember* __restrict__ rec = board_member(a, m);
  double* __restrict__ ring =
      reinterpret_cast<double*>(a.board + SACENV_BOARD_HEADER_BYTES + (int64_t)SACENV_BOARD_MEMBER_BYTES * a.members) +
      (int64_t)m * L;
  int64_t lo, hi, cursor, total;
  board_window(a, lo, hi, cursor, total);
  const int64_t E = rec->episodes;
  if (t < kMaxL && t < (E < L ? E : L)) hist[kMaxL - 1 - t] = ring[(E - 1 - t) % L];
  const int64_t env_lo = (int64_t)a.env_base + (int64_t)m * a.epm, env_hi = env_lo + a.epm;
  const uint4* __restrict__ entries = reinterpret_cast<const uint4*>(a.log + SACENV_EPISODE_ENTRY_BYTES);

  uint32_t saves = 0, tc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double best = -__builtin_inf();
  int64_t best_at = INT64_MAX, save_at = -1, save_step = -1;
  int64_t k = 0;   // the member's entries before this round (the same in every lane)

  if (lo < hi) {
    uint4 c0[kBoardPer], c1[kBoardPer];
#pragma unroll
    for (int u = 0; u < kBoardPer; ++u) {   // unconditional loads at a clamped index, as in k_ep_count
      const int64_t i = lo + u * kBoardThreads + t;
      const int64_t ic = i < hi ? i : hi - 1;
      c0[u] = entries[2 * ic];
      c1[u] = entries[2 * ic + 1];
    }
    for (int64_t base = lo; base < hi; base += kBoardRound) {
      uint4 n0[kBoardPer], n1[kBoardPer];
#pragma unroll
      for (int u = 0; u < kBoardPer; ++u) {
        const int64_t i = base + kBoardRound + u * kBoardThreads + t;
        const int64_t ic = i < hi ? i : hi - 1;
        n0[u] = entries[2 * ic];
        n1[u] = entries[2 * ic + 1];
      }
      bool mine[kBoardPer];
      uint32_t rank[kBoardPer];
#pragma unroll
      for (int u = 0; u < kBoardPer; ++u) {
        const int64_t i = base + u * kBoardThreads + t;
        const int64_t env = (int32_t)c1[u].x;
        mine[u] = i < hi && env >= env_lo && env < env_hi;
        const uint64_t mask = __ballot(mine[u]);
        rank[u] = ballot_rank(mask);
        if (lane == 0) wcnt[u][wv] = (uint32_t)__popcll(mask);
      }
      __syncthreads();
      uint32_t c = 0;   // the member's entries of this round; pos: this lane's among them, in log order
#pragma unroll
      for (int u = 0; u < kBoardPer; ++u) {
        uint32_t pos = c + rank[u];
#pragma unroll
        for (int j = 0; j < kBoardWaves; ++j) {
          const uint32_t v = wcnt[u][j];
          pos += j < wv ? v : 0u;
          c += v;
        }
        if (mine[u]) {
          hist[kMaxL + pos] = __longlong_as_double((long long)(((uint64_t)c0[u].w << 32) | c0[u].z));
          ends[pos] = (int64_t)(((uint64_t)c0[u].y << 32) | c0[u].x);
          terms[pos] = (uint8_t)(c1[u].z < 7u ? c1[u].z : 7u);
        }
      }
      __syncthreads();
      for (uint32_t r = t; r < c; r += kBoardThreads) {
        const int64_t g = E + k + r;                       // the episode's number in the member's history
        const int n = (int)(g + 1 < L ? g + 1 : L);
        const double s = hist[kMaxL + r];
        double avg = mean_np(&hist[kMaxL + r - (n - 1)], n);
        if (avg != avg) avg = __longlong_as_double(0x7ff8000000000000ll);   // one NaN, whatever made it
        const int64_t end = ends[r];
        const uint32_t tk = terms[r];
        if (s > best) {
          best = s;
          best_at = g;
        }
        if (s > avg) {
          ++saves;
          save_at = g;
          save_step = end;
        }
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) tc[j] += tk == j ? 1u : 0u;
        if (r == c - 1) {
          last_score = s;
          last_avg = avg;
          last_end = end;
        }
      }
      double keep = 0.0;
      if (c != 0 && t < kMaxL) keep = hist[c + t];
      __syncthreads();
      if (c != 0 && t < kMaxL) hist[t] = keep;
      k += c;
#pragma unroll
      for (int u = 0; u < kBoardPer; ++u) {
        c0[u] = n0[u];
        c1[u] = n1[u];
      }
    }
  }
  __syncthreads();
  if (t < kMaxL && t < (k < L ? k : L)) ring[(E + k - 1 - t) % L] = hist[kMaxL - 1 - t];

  // the lanes' tallies: sums, the best score (the earlier episode on equal values, as the
  // loop of main.py:103 keeps it) and the latest save
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    saves += __shfl_xor(saves, o);
#pragma unroll
    for (int j = 0; j < 8; ++j) tc[j] += __shfl_xor(tc[j], o);
    const double ob = __shfl_xor(best, o);
    const int64_t oa = __shfl_xor((long long)best_at, o);
    if (ob > best || (ob == best && oa < best_at)) {
      best = ob;
      best_at = oa;
    }
    const int64_t sa = __shfl_xor((long long)save_at, o);
    const int64_t ss = __shfl_xor((long long)save_step, o);
    if (sa > save_at) {
      save_at = sa;
      save_step = ss;
    }
  }
  if (lane == 0) {
    w_saves[wv] = saves;
#pragma unroll
    for (int j = 0; j < 8; ++j) w_terms[wv][j] = tc[j];
    w_best[wv] = best;
    w_best_at[wv] = best_at;
    w_save_at[wv] = save_at;
    w_save_step[wv] = save_step;
  }
  __syncthreads();
  if (t < 8) {
    uint64_t sum = 0;
    for (int j = 0; j < kBoardWaves; ++j) sum += w_terms[j][t];
    if (sum != 0) rec->terms[t] += sum;
  }
  if (t == 0) {
    uint32_t S = 0;
    for (int j = 0; j < kBoardWaves; ++j) {
      S += w_saves[j];
      if (w_best[j] > best || (w_best[j] == best && w_best_at[j] < best_at)) {
        best = w_best[j];
        best_at = w_best_at[j];
      }
      if (w_save_at[j] > save_at) {
        save_at = w_save_at[j];
        save_step = w_save_step[j];
      }
    }
    rec->saved_now = S != 0 ? 1u : 0u;
    if (k != 0) {
      rec->episodes = E + k;
      rec->last = last_score;
      rec->avg = last_avg;
      rec->last_end_step = last_end;
      if (best > rec->best) rec->best = best;
      if (S != 0) {
        rec->saves += S;
        rec->last_save_step = save_step;
      }
    }
  }
}

__global__ __launch_bounds__(kCopyThreads) void k_board_finish(const Board a, const float4* __restrict__ weights,
                                                               float4* __restrict__ snapshot, const int64_t vecs) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    int64_t lo, hi, cursor, total;
    board_window(a, lo, hi, cursor, total);
    int64_t* hdr = reinterpret_cast<int64_t*>(a.board);
    hdr[0] = total;
    hdr[1] += (total > a.cap ? total : a.cap) - (cursor > a.cap ? cursor : a.cap);
    hdr[2] += 1;
  }
  if (snapshot == nullptr) return;
  const int m = blockIdx.y;
  if (board_member(a, m)->saved_now == 0u) return;
  slab_copy<kCopyThreads>(weights + (int64_t)m * vecs, snapshot + (int64_t)m * vecs, vecs);
}

// the empty board, as 8-B words
__global__ __launch_bounds__(256) void k_board_init(uint64_t* __restrict__ board, const int64_t words,
                                                    const int64_t members) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += stride) {
    uint64_t v = 0;
    if (w >= kHeaderWords && w < kHeaderWords + kMemberWords * members) {
      const int f = (int)((w - kHeaderWords) % kMemberWords);
      if (f == 2 || f == 3) v = ~0ull;                                                   // last_save_step, last_end_step = -1
      if (f == 5) v = (uint64_t)__double_as_longlong(-__builtin_inf());                  // best
    }
    board[w] = v;
  }
}

__global__ void k_board_rewind(int64_t* __restrict__ board) { board[0] = 0; }

int check_board(const SacenvBoard* b) {
  if (b == nullptr) return SACENV_E_NULL;
  if (b->members < 1 || b->members > SACENV_BOARD_MAX_MEMBERS || b->lookback < 1 ||
      b->lookback > SACENV_BOARD_MAX_LOOKBACK || b->envs_per_member < 1 || b->env_base < 0 || b->cap < 0 ||
      b->member_floats < 0 || b->member_floats % 4 != 0)
    return SACENV_E_SIZE;
  return SACENV_OK;
}

}  // namespace

extern "C" {

int sacenv_board_bytes(const SacenvBoard* b, int64_t* bytes) {
  const int rc = check_board(b);
  if (rc) return rc;
  if (bytes == nullptr) return SACENV_E_NULL;
  *bytes = board_bytes(b->members, b->lookback);
  return SACENV_OK;
}

int sacenv_board_init(const SacenvBoard* b, void* board, void* stream) {
  const int rc = check_board(b);
  if (rc) return rc;
  if (board == nullptr) return SACENV_E_NULL;
  if ((uintptr_t)board % 16 != 0) return SACENV_E_RANGE;
  const int64_t words = board_bytes(b->members, b->lookback) / 8;
  hipLaunchKernelGGL(k_board_init, dim3((uint32_t)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     static_cast<uint64_t*>(board), words, (int64_t)b->members);
  return status();
}

int sacenv_board_update(const SacenvBoard* b, const void* log, void* board, const float* weights, float* snapshot,
                        void* stream) {
  const int rc = check_board(b);
  if (rc) return rc;
  if (log == nullptr || board == nullptr) return SACENV_E_NULL;
  if ((uintptr_t)log % 16 != 0 || (uintptr_t)board % 16 != 0 || (uintptr_t)weights % 16 != 0 ||
      (uintptr_t)snapshot % 16 != 0)
    return SACENV_E_RANGE;
  if (b->member_floats != 0 && (weights == nullptr) != (snapshot == nullptr)) return SACENV_E_RANGE;
  const bool copy = b->member_floats != 0 && weights != nullptr && snapshot != nullptr;
  const Board a = {static_cast<const char*>(log), static_cast<char*>(board), b->cap, b->members,
                   b->envs_per_member, b->env_base, b->lookback};
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_board_update, dim3((uint32_t)b->members), dim3(kBoardThreads), 0, st, a);
  const int64_t vecs = copy ? b->member_floats / 4 : 0;
  const int64_t chunks = vecs < 1 ? 1 : slab_chunks(vecs, kCopyThreads, kCopyChunks);   // (the commit always runs)
  hipLaunchKernelGGL(k_board_finish, copy ? dim3((uint32_t)chunks, (uint32_t)b->members) : dim3(1), dim3(kCopyThreads), 0,
                     st, a, copy ? reinterpret_cast<const float4*>(weights) : nullptr,
                     copy ? reinterpret_cast<float4*>(snapshot) : nullptr, vecs);
  return status();
}

int sacenv_board_rewind(const SacenvBoard* b, void* board, void* stream) {
  const int rc = check_board(b);
  if (rc) return rc;
  if (board == nullptr) return SACENV_E_NULL;
  if ((uintptr_t)board % 16 != 0) return SACENV_E_RANGE;
  hipLaunchKernelGGL(k_board_rewind, dim3(1), dim3(1), 0, (hipStream_t)stream, static_cast<int64_t*>(board));
  return status();
}

}  // extern "C"
