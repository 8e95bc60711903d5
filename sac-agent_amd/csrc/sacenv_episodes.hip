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
// The population scoreboard (sacenv_board.hip) reads that log.

#include "sacenv_episodes.h"
#include "sacenv_wave_core.h"

namespace {

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
      const int64_t pos = first + ballot_rank(m);
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
