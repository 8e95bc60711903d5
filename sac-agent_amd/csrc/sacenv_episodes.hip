// sacenv_episodes.hip — gfx950 episode log (include/sacenv_episodes.h).
//
// main.py:70-114 keeps a score per episode (`score += reward`, :82) and a history
// of them (:99). The step launches restart an env inside the step and keep only its
// last ending, so the per-episode scores are rebuilt here from the step records
// they already write: K steps' (reward, done, term) columns and a per-env carry go
// in, one 32-B entry per finished episode comes out, ascending by (end_step, env).
//
// Three launches, one lane per env, one wave per 64 envs:
//   k_ep_count  per (step, wave): ballot of the done bytes, its popcount
//   k_ep_scan   exclusive scan of the counts in step-major order (step k's waves
//               before step k + 1's); its last workgroup also moves the log's
//               device-resident total on by the number found
//   k_ep_emit   walks the K steps again with the carry in registers; an ending
//               lane's position is the log's old total + its (step, wave)'s scanned
//               count + its rank in the ballot (mbcnt), and it stores its entry
//               there with two 16-B stores
// No atomics give a position: the log's bytes are the same run to run.
//
// The population scoreboard (include/sacenv_scoreboard.h) reads that log: see the second
// half of this file.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sacenv_board_core.h"
#include "sacenv_episodes.h"
#include "sacenv_scoreboard.h"

namespace {

constexpr int kWave = 64;
constexpr int kCountSteps = 32;     // steps per wave of the count launch
constexpr int kUnroll = 8;          // count launch: steps whose loads are in flight together
constexpr int kEmitUnroll = 16;     // the same of the emit launch (three loads per step)
constexpr int kScanThreads = 1024;
constexpr int kScanWaves = kScanThreads / kWave;
constexpr int kScanTile = 2 * kScanThreads;  // counts per pass of a scan workgroup (two per lane)
constexpr int kScanBlocks = 128;    // at most this many scan workgroups
constexpr int kHeaderBytes = SACENV_EPISODE_ENTRY_BYTES;

// what the kernels need of SacenvEpisodeScan, the columns as pointers to env 0 of step 0
struct Scan {
  const char* reward;
  const uint8_t* done;
  const uint8_t* term;
  int64_t stride;
  int64_t step0;
  int64_t cap;
  int32_t n_envs, n_waves, n_steps, env_base;
};

// scratch: [0, 16) the log's total before this call (i64, set by k_ep_scan) | u64
// counts[M] | u64 prefix[M], M = n_steps x n_waves rounded up to even (16-B rows)
__host__ __device__ inline int64_t scan_items(int64_t n_steps, int64_t n_waves) { return n_steps * n_waves; }
__host__ __device__ inline int64_t scratch_need(int64_t items) { return 16 + 16 * ((items + 1) / 2 * 2); }

// Count launch: wave (kc, w) counts the endings of steps kc * 32 .. + 31 among envs
// 64 w .. 64 w + 63. The done column alone is read (1 B per env and step). Every load
// is unconditional so that kUnroll of them are in flight together: a lane past n_envs
// reads the last env's byte and a step past the end the last step's, and the predicate
// drops what they loaded (a load behind a branch waits for itself before the next).
__global__ __launch_bounds__(kWave) void k_ep_count(const Scan a, uint64_t* __restrict__ counts) {
  const int lane = threadIdx.x;
  const uint32_t w = blockIdx.x % (uint32_t)a.n_waves;
  const int k0 = (int)(blockIdx.x / (uint32_t)a.n_waves) * kCountSteps;
  const int e = (int)w * kWave + lane;
  const bool active = e < a.n_envs;
  const int n = min(kCountSteps, a.n_steps - k0);
  const uint8_t* __restrict__ d = a.done + (int64_t)k0 * a.stride + min(e, a.n_envs - 1);
  uint64_t* __restrict__ out = counts + (int64_t)k0 * a.n_waves + w;
  for (int j = 0; j < n; j += kUnroll) {
    uint8_t b[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) b[u] = d[(int64_t)min(j + u, n - 1) * a.stride];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint64_t m = __ballot(active && b[u] != 0);
      if (lane == 0 && j + u < n) out[(int64_t)(j + u) * a.n_waves] = (uint64_t)__popcll(m);
    }
  }
}

// Scan launch: workgroup b owns counts [b * chunk, (b + 1) * chunk) (chunk a multiple
// of the tile). It first sums every count before its range itself -- at most
// kScanBlocks workgroups, so the counts are read kScanBlocks / 2 times over on
// average, out of L2, which is 16 B per (step, wave) against the 448 B of records
// behind it -- and then scans its own range tile by tile. No workgroup waits for
// another. Counts and prefix are separate arrays: a range's counts are still being
// summed by later workgroups while its prefix is written.
__global__ __launch_bounds__(kScanThreads) void k_ep_scan(const uint64_t* __restrict__ counts,
                                                          uint64_t* __restrict__ prefix, const int64_t items,
                                                          const int64_t chunk, int64_t* __restrict__ base_slot,
                                                          int64_t* __restrict__ total) {
  __shared__ uint64_t wsum[kScanWaves];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  const int64_t begin = (int64_t)blockIdx.x * chunk;
  const int64_t end = begin + chunk < items ? begin + chunk : items;
  uint64_t acc = 0;
#pragma unroll 8
  for (int64_t i = 2 * t; i < begin; i += kScanTile) {  // (begin is a multiple of the tile: whole pairs)
    const ulong2 v = *reinterpret_cast<const ulong2*>(counts + i);
    acc += v.x + v.y;
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) wsum[wv] = acc;
  __syncthreads();
  uint64_t running = 0;
#pragma unroll
  for (int j = 0; j < kScanWaves; ++j) running += wsum[j];
  __syncthreads();
  for (int64_t tile = begin; tile < end; tile += kScanTile) {
    const int64_t i = tile + 2 * t;
    uint64_t c0 = 0, c1 = 0;
    if (i + 1 < end) {
      const ulong2 v = *reinterpret_cast<const ulong2*>(counts + i);
      c0 = v.x, c1 = v.y;
    } else if (i < end) {
      c0 = counts[i];
    }
    const uint64_t local = c0 + c1;
    uint64_t incl = local;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const uint64_t y = __shfl_up(incl, o);
      if (lane >= o) incl += y;
    }
    if (lane == kWave - 1) wsum[wv] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int j = 0; j < kScanWaves; ++j) {
      before += j < wv ? wsum[j] : 0;
      all += wsum[j];
    }
    const uint64_t excl = running + before + incl - local;
    if (i + 1 < end)
      *reinterpret_cast<ulong2*>(prefix + i) = ulong2{excl, excl + c0};
    else if (i < end)
      prefix[i] = excl;
    running += all;
    __syncthreads();
  }
  if (blockIdx.x == gridDim.x - 1 && t == 0) {  // the last range ends at `items`: running = all found
    const int64_t old = *total;
    *base_slot = old;
    *total = old + (int64_t)running;
  }
}

// One step of the walk for one lane: the f64 add and the length, and where the wave
// has an ending (one wave-uniform branch, not taken in most steps) the entry of each
// ending lane at the log's old total + the (step, wave)'s scanned count + the lane's
// rank among the wave's endings.
__device__ __forceinline__ void ep_step(const Scan& a, const int64_t step, const int env, const float r,
                                        const bool ended, const uint32_t term, const int64_t first,
                                        uint4* __restrict__ entries, double& score, int32_t& len) {
  score = score + (double)r;
  ++len;
  const uint64_t m = __ballot(ended);
  if (m != 0ull) {
    if (ended) {
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      const int64_t pos = first + rank;
      if (pos < a.cap) {
        const uint64_t es = (uint64_t)step;
        const uint64_t sc = (uint64_t)__double_as_longlong(score);
        entries[2 * pos] = uint4{(uint32_t)es, (uint32_t)(es >> 32), (uint32_t)sc, (uint32_t)(sc >> 32)};
        entries[2 * pos + 1] = uint4{(uint32_t)env, (uint32_t)len, term, 0u};
      }
      score = 0.0;
      len = 0;
    }
  }
}

// Emit launch: wave w walks its 64 envs through the K steps, kEmitUnroll steps' loads in
// flight at a time (a 256-B reward row and two 64-B byte rows per step; the walk's
// only dependent chain is one f64 add per step). The loads are unconditional, as in
// the count launch: a lane past n_envs reads the last env's columns and never ends.
__global__ __launch_bounds__(kWave) void k_ep_emit(const Scan a, const uint64_t* __restrict__ prefix,
                                                   const int64_t* __restrict__ base_slot,
                                                   double* __restrict__ carry_score,
                                                   int32_t* __restrict__ carry_len, char* __restrict__ log) {
  const int lane = threadIdx.x;
  const int w = blockIdx.x;
  const int e = w * kWave + lane;
  const bool active = e < a.n_envs;
  const int el = min(e, a.n_envs - 1);
  double score = carry_score[el];
  int32_t len = carry_len[el];
  const int64_t base = *base_slot;
  const char* __restrict__ rp = a.reward + 4 * (int64_t)el;
  const uint8_t* __restrict__ dp = a.done + el;
  const uint8_t* __restrict__ tp = a.term + el;
  const uint64_t* __restrict__ pp = prefix + w;
  uint4* __restrict__ entries = reinterpret_cast<uint4*>(log + kHeaderBytes);
  const int env = a.env_base + e;
  int k = 0;
  for (; k + kEmitUnroll <= a.n_steps; k += kEmitUnroll) {
    float r[kEmitUnroll];
    uint8_t d[kEmitUnroll], tm[kEmitUnroll];
    uint64_t pf[kEmitUnroll];
#pragma unroll
    for (int u = 0; u < kEmitUnroll; ++u) {
      const int64_t off = (int64_t)(k + u) * a.stride;
      r[u] = *reinterpret_cast<const float*>(rp + off);
      d[u] = dp[off];
      tm[u] = tp[off];
      pf[u] = pp[(int64_t)(k + u) * a.n_waves];
    }
#pragma unroll
    for (int u = 0; u < kEmitUnroll; ++u)
      ep_step(a, a.step0 + k + u, env, r[u], active && d[u] != 0, tm[u], base + (int64_t)pf[u], entries, score, len);
  }
  for (; k < a.n_steps; ++k) {  // the last K mod kEmitUnroll steps
    const int64_t off = (int64_t)k * a.stride;
    ep_step(a, a.step0 + k, env, *reinterpret_cast<const float*>(rp + off), active && dp[off] != 0, tp[off],
            base + (int64_t)pp[(int64_t)k * a.n_waves], entries, score, len);
  }
  if (active) {
    carry_score[e] = score;
    carry_len[e] = len;
  }
}

int check_scan(const SacenvEpisodeScan* s) {
  if (s == nullptr) return SACENV_E_NULL;
  if (s->n_envs < 1 || s->n_pad < s->n_envs || s->n_pad % kWave != 0 || s->n_steps < 1 || s->cap < 0 ||
      s->env_base < 0 || (int64_t)s->env_base + s->n_envs > INT32_MAX)
    return SACENV_E_SIZE;
  if (scan_items(s->n_steps, s->n_pad / kWave) >= (int64_t)1 << 31) return SACENV_E_SIZE;
  if (s->reward_off < 0 || s->done_off < 0 || s->term_off < 0 || s->rec_stride < 0 || s->reward_off % 4 != 0)
    return SACENV_E_RANGE;
  if (s->n_steps > 1 && (s->rec_stride == 0 || s->rec_stride % 4 != 0)) return SACENV_E_RANGE;
  return SACENV_OK;
}

int status() {
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? SACENV_OK : (int)err;
}

}  // namespace

extern "C" {

int sacenv_episodes_scratch_bytes(const SacenvEpisodeScan* s, int64_t* bytes) {
  const int rc = check_scan(s);
  if (rc) return rc;
  if (bytes == nullptr) return SACENV_E_NULL;
  *bytes = scratch_need(scan_items(s->n_steps, s->n_pad / kWave));
  return SACENV_OK;
}

int sacenv_episodes_update(const SacenvEpisodeScan* s, const void* records, void* carry, void* log, void* scratch,
                           int64_t scratch_bytes, void* stream) {
  const int rc = check_scan(s);
  if (rc) return rc;
  if (records == nullptr || carry == nullptr || log == nullptr || scratch == nullptr) return SACENV_E_NULL;
  if ((uintptr_t)records % 4 != 0 || (uintptr_t)carry % 8 != 0 || (uintptr_t)log % 16 != 0 ||
      (uintptr_t)scratch % 16 != 0)
    return SACENV_E_RANGE;
  const int32_t n_waves = s->n_pad / kWave;
  const int64_t items = scan_items(s->n_steps, n_waves);
  if (scratch_bytes < scratch_need(items)) return SACENV_E_SIZE;
  const char* rec = static_cast<const char*>(records);
  Scan a;
  a.reward = rec + s->reward_off;
  a.done = reinterpret_cast<const uint8_t*>(rec + s->done_off);
  a.term = reinterpret_cast<const uint8_t*>(rec + s->term_off);
  a.stride = s->rec_stride;
  a.step0 = s->step0;
  a.cap = s->cap;
  a.n_envs = s->n_envs;
  a.n_waves = n_waves;
  a.n_steps = s->n_steps;
  a.env_base = s->env_base;
  char* sc = static_cast<char*>(scratch);
  int64_t* base_slot = reinterpret_cast<int64_t*>(sc);
  uint64_t* counts = reinterpret_cast<uint64_t*>(sc + 16);
  uint64_t* prefix = counts + (items + 1) / 2 * 2;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t k_chunks = (s->n_steps + kCountSteps - 1) / kCountSteps;
  hipLaunchKernelGGL(k_ep_count, dim3((uint32_t)(k_chunks * n_waves)), dim3(kWave), 0, st, a, counts);
  // ranges of whole tiles, at most kScanBlocks of them
  const int64_t tiles = (items + kScanTile - 1) / kScanTile;
  const int64_t chunk = (tiles + kScanBlocks - 1) / kScanBlocks * kScanTile;
  const int64_t blocks = (items + chunk - 1) / chunk;
  hipLaunchKernelGGL(k_ep_scan, dim3((uint32_t)blocks), dim3(kScanThreads), 0, st, counts, prefix, items, chunk,
                     base_slot, reinterpret_cast<int64_t*>(log));
  double* carry_score = static_cast<double*>(carry);
  hipLaunchKernelGGL(k_ep_emit, dim3((uint32_t)n_waves), dim3(kWave), 0, st, a, prefix, base_slot, carry_score,
                     reinterpret_cast<int32_t*>(carry_score + s->n_pad), static_cast<char*>(log));
  return status();
}

}  // extern "C"

// ---------------------------------------------------------------------------------------
// The population scoreboard (include/sacenv_scoreboard.h): main.py:99-108 per member, from
// the log above.
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

namespace {

using namespace sacenv_board;

constexpr int kBoardThreads = 1024;
constexpr int kBoardWaves = kBoardThreads / kWave;
constexpr int kBoardPer = 2;                              // entries per lane and round
constexpr int kBoardRound = kBoardPer * kBoardThreads;
constexpr int kCopyThreads = 256;
constexpr int kCopyChunks = 64;                           // at most this many workgroups per member's slab
constexpr int kCopyUnroll = 4;

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
  const uint4* __restrict__ entries = reinterpret_cast<const uint4*>(a.log + kHeaderBytes);

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
        rank[u] = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
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
  const float4* __restrict__ src = weights + (int64_t)m * vecs;
  float4* __restrict__ dst = snapshot + (int64_t)m * vecs;
  const int64_t stride = (int64_t)gridDim.x * kCopyThreads;
  int64_t i = (int64_t)blockIdx.x * kCopyThreads + threadIdx.x;
  for (; i + (kCopyUnroll - 1) * stride < vecs; i += kCopyUnroll * stride) {
    float4 v[kCopyUnroll];
#pragma unroll
    for (int u = 0; u < kCopyUnroll; ++u) v[u] = src[i + u * stride];
#pragma unroll
    for (int u = 0; u < kCopyUnroll; ++u) dst[i + u * stride] = v[u];
  }
  for (; i < vecs; i += stride) dst[i] = src[i];
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
  Board a;
  a.log = static_cast<const char*>(log);
  a.board = static_cast<char*>(board);
  a.cap = b->cap;
  a.members = b->members;
  a.epm = b->envs_per_member;
  a.env_base = b->env_base;
  a.lookback = b->lookback;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_board_update, dim3((uint32_t)b->members), dim3(kBoardThreads), 0, st, a);
  const int64_t vecs = copy ? b->member_floats / 4 : 0;
  const int64_t per = (int64_t)kCopyThreads * kCopyUnroll;
  int64_t chunks = (vecs + per - 1) / per;
  chunks = chunks < 1 ? 1 : chunks > kCopyChunks ? kCopyChunks : chunks;
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
