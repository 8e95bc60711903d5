// sacenv_replay_prio.h — the device code of the prioritized population replay
// (include/sacenv_prioritized_replay.h): per member a 64-ary sum tree over
// the ring rows' u32 priorities, in a buffer beside the replay arena. sacenv_replay_pop.hip
// includes it after sacenv_replay_core.h and holds the entry points.
//
// One wave owns one node: it loads the node's 64 children in one coalesced access (256 B of
// leaves, 512 B of u64 nodes), and either sums them (the repair) or takes their prefix sum
// and ballots for the child to descend into (the draw). Everything is integer, so no order
// of summation shows in the bytes.
//
// Phases that read what an earlier phase wrote are separate launches (leaves -> level 1 ->
// levels >= 2): stream order is the only cross-workgroup hand-off here. Inside the last
// launch one workgroup per member builds level k from level k - 1 that its own waves wrote;
// between two levels every thread passes an agent-scope fence (its stores are out, its L1
// is fresh) and the workgroup's barrier.
#pragma once

#include "sacenv_philox.h"
#include "sacenv_prioritized_replay.h"

namespace {

constexpr int kPrioLevels = SACENV_REPLAY_PRIO_MAX_LEVELS;
constexpr int kPrioFan = 64;            // children per node: one per lane
constexpr int kPrioThreads = 256;       // the wave-per-node kernels: four nodes per workgroup
constexpr int kPrioMemberThreads = 1024;  // the one-workgroup-per-member kernels
constexpr uint32_t kPrioCap = SACENV_REPLAY_PRIO_MAX_LEAF;
static_assert(kPrioFan == kWave, "a lane per child");

// a member's slab: the layout all members share, on the launch's base moved by m slabs
struct PT {
  char* b;
  int64_t member_bytes;
  int32_t levels, pad;
  int64_t count[kPrioLevels], offset[kPrioLevels];
};

struct PrioHeader {
  uint64_t total;
  uint32_t max_leaf, zero;
  int64_t calls;
};

struct PrioSeeds {
  uint64_t v[SACENV_REPLAY_POP_MAX_MEMBERS];
};

__host__ __device__ inline void prio_layout(int64_t M, SacenvReplayPrioLayout* o) {
  int64_t off = SACENV_REPLAY_PRIO_HEADER_BYTES, n = M;
  int k = 0;
  for (; k < kPrioLevels; ++k) {
    o->count[k] = n;
    o->offset[k] = off;
    off = align256(off + (k == 0 ? 4 : 8) * n);
    if (n <= kPrioFan) break;
    n = (n + kPrioFan - 1) / kPrioFan;
  }
  o->levels = k + 1;  // (M < 2^31: the loop breaks at k <= 5)
  o->pad = 0;
  for (++k; k < kPrioLevels; ++k) o->count[k] = o->offset[k] = 0;
  o->member_bytes = off;
}

__device__ __forceinline__ char* prio_slab(const PT& t, int64_t m) { return t.b + m * t.member_bytes; }
__device__ __forceinline__ PrioHeader* prio_header(char* slab) { return reinterpret_cast<PrioHeader*>(slab); }
__device__ __forceinline__ uint32_t* prio_leaves(const PT& t, char* slab) {
  return reinterpret_cast<uint32_t*>(slab + t.offset[0]);
}

// the sum of a u64 over the wave, in every lane
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) v += __shfl_xor((unsigned long long)v, d, kWave);
  return v;
}

// the inclusive prefix sum of a u64 over the wave
__device__ __forceinline__ uint64_t wave_scan64(uint64_t v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint64_t u = __shfl_up((unsigned long long)v, d, kWave);
    v += lane >= d ? u : 0ull;
  }
  return v;
}

// entry `c` of level k (0 past the level's end): u32 leaves, u64 nodes
__device__ __forceinline__ uint64_t prio_entry(const char* slab, int64_t off, int64_t count, bool leaves, int64_t c) {
  if (c >= count) return 0ull;
  return leaves ? (uint64_t)reinterpret_cast<const uint32_t*>(slab + off)[c]
                : reinterpret_cast<const uint64_t*>(slab + off)[c];
}

// ---- init: grid (blocks, P) x 256. Zero the slab in 16-B stores; the header rides in the first two.
__device__ __forceinline__ void prio_init_body(const PT& t, char* slab) {
  const int64_t vecs = t.member_bytes / 16, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < vecs; i += stride)
    store16(slab + 16 * i, 0ull, i == 0 ? (uint64_t)SACENV_REPLAY_PRIO_ONE : 0ull);  // total | max_leaf, 0 ; calls, 0
}

// ---- mark: the rows of one store. The ring rows are [base, base + rows) mod M.
struct PrioSpan {
  int64_t base, rows;
};
__device__ __forceinline__ PrioSpan prio_span(int64_t M, int64_t c0, int64_t n) {
  const int64_t first = n > M ? n - M : 0;  // store_body's rule
  return PrioSpan{(c0 + first) % M, n - first};
}

// grid (blocks, P) x 256, striding
__device__ __forceinline__ void prio_mark_body(const PT& t, char* slab, int64_t c0, int64_t n) {
  const int64_t M = t.count[0];
  const PrioSpan s = prio_span(M, c0, n);
  const uint32_t v = prio_header(slab)->max_leaf;
  uint32_t* __restrict__ leaf = prio_leaves(t, slab);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < s.rows; j += stride) {
    int64_t row = s.base + j;
    row = row >= M ? row - M : row;
    leaf[row] = v;
  }
}

// one wave: level-1 node `node` from its leaves
__device__ __forceinline__ void prio_l1_node(const PT& t, char* slab, int64_t node, int lane) {
  const uint64_t s = wave_sum64(prio_entry(slab, t.offset[0], t.count[0], true, node * kPrioFan + lane));
  if (lane == 0) reinterpret_cast<uint64_t*>(slab + t.offset[1])[node] = s;
}

// grid (ceil(W / 4), P) x 256, wave w of the member: the w-th level-1 node over the span's rows,
// those of [base, min(base + rows, M)) first, then those of the wrapped part [0, base + rows - M).
// W >= both counts together (the host: min(rows / 64 + 3, count[1] + 1)).
__device__ __forceinline__ void prio_l1_span_body(const PT& t, char* slab, int64_t c0, int64_t n) {
  const int64_t M = t.count[0];
  const PrioSpan s = prio_span(M, c0, n);
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t w = (int64_t)blockIdx.x * (kPrioThreads / kWave) + threadIdx.x / kWave;
  const int64_t e = s.base + s.rows, e1 = e < M ? e : M;
  const int64_t a1 = s.base / kPrioFan, cnt1 = (e1 - 1) / kPrioFan - a1 + 1;
  const int64_t cnt2 = e > M ? (e - M - 1) / kPrioFan + 1 : 0;
  int64_t node;
  if (w < cnt1) node = a1 + w;
  else if (w - cnt1 < cnt2) node = w - cnt1;
  else return;
  prio_l1_node(t, slab, node, lane);
}

// grid (ceil(batch / 4), P) x 256, wave i of the member: the level-1 node of row idx[i]
__device__ __forceinline__ void prio_l1_idx_body(const PT& t, char* slab, int batch, const int64_t* __restrict__ idx) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = (int64_t)blockIdx.x * (kPrioThreads / kWave) + threadIdx.x / kWave;
  if (i >= batch) return;
  const int64_t row = idx[i];
  if (row < 0 || row >= t.count[0]) return;
  prio_l1_node(t, slab, row / kPrioFan, lane);
}

// grid (1, P) x 1 024: levels 2 .. top from the level below, wave per node, then the total from
// the top level (<= 64 entries).
__device__ __forceinline__ void prio_upper_body(const PT& t, char* slab) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  constexpr int kWaves = kPrioMemberThreads / kWave;
#pragma unroll
  for (int k = 2; k < kPrioLevels; ++k) {
    if (k >= t.levels) break;
    uint64_t* __restrict__ out = reinterpret_cast<uint64_t*>(slab + t.offset[k]);
    for (int64_t node0 = wv; node0 < t.count[k]; node0 += 4 * kWaves) {  // four nodes' loads in flight per wave
      uint64_t v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t node = node0 + u * kWaves;
        v[u] = node < t.count[k]
                   ? prio_entry(slab, t.offset[k - 1], t.count[k - 1], false, node * kPrioFan + lane)
                   : 0ull;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t node = node0 + u * kWaves;
        const uint64_t s = wave_sum64(v[u]);
        if (lane == 0 && node < t.count[k]) out[node] = s;
      }
    }
    __threadfence();
    __syncthreads();
  }
  if (wv == 0) {
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < kPrioLevels; ++k)
      if (k == t.levels - 1) v = prio_entry(slab, t.offset[k], t.count[k], k == 0, lane);
    const uint64_t s = wave_sum64(v);
    if (lane == 0) prio_header(slab)->total = s;
  }
}

// ---- set / update_td: grid (1, P) x 1 024. The batch in chunks of 1 024 positions, in order:
// inside a chunk a position is dropped if a later one of the chunk names its row (LDS), and a
// later chunk's stores follow an earlier chunk's (fence + barrier), so the highest position wins.
// max_leaf follows the winners only. In one chunk they are known as they are written. Across
// chunks a winner of its chunk may lose to a later chunk, so a batch of more than one chunk is
// read once more when all leaves are in place: a position counts if the row now holds its
// value -- true for every winner, and for a loser only with a value that a winner wrote.
struct PrioTd {
  const float* sq1;
  const float* sq2;
  double alpha, eps;
};

__device__ __forceinline__ uint32_t prio_clamp(uint32_t v) { return v < 1u ? 1u : (v > kPrioCap ? kPrioCap : v); }

__device__ __forceinline__ uint32_t prio_td_leaf(const PrioTd& td, int64_t i) {
  const double r1 = sqrt((double)td.sq1[i]);
  const double a = (td.sq2 != nullptr ? 0.5 * (r1 + sqrt((double)td.sq2[i])) : r1) + td.eps;
  if (!(a >= 0.0)) return 1u;  // NaN (a NaN or negative td_sq), before pow: pow(NaN, 0) is 1
  const double s = pow(a, td.alpha) * 65536.0;
  if (!(s >= 1.0)) return 1u;
  return s >= (double)kPrioCap ? kPrioCap : (uint32_t)floor(s);
}

template <bool kTd>
__device__ __forceinline__ void prio_write_body(const PT& t, char* slab, int batch, const int64_t* __restrict__ idx,
                                                const uint32_t* __restrict__ leaf_in, const PrioTd& td) {
  __shared__ __attribute__((aligned(16))) uint32_t s_row[kPrioMemberThreads];
  __shared__ uint32_t s_max[kPrioMemberThreads / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  const int64_t M = t.count[0];
  uint32_t* __restrict__ leaf = prio_leaves(t, slab);
  const bool one_chunk = batch <= kPrioMemberThreads;
  uint32_t mx = 0;
  for (int64_t c = 0; c < batch; c += kPrioMemberThreads) {
    const int64_t i = c + tid;
    const int len = batch - c < kPrioMemberThreads ? (int)(batch - c) : kPrioMemberThreads;
    const int64_t row = i < batch ? idx[i] : -1;
    const bool in = row >= 0 && row < M;
    const uint32_t mine = in ? (uint32_t)row : 0xFFFFFFFFu;  // (M < 2^31: no row is the marker)
    s_row[tid] = mine;
    __syncthreads();
    // a later position of the chunk with this row? Four positions per broadcast LDS read, from the
    // wave's first position on (positions past `len` hold the marker, which no valid row equals)
    bool later = false;
    for (int j = tid & ~(kWave - 1); j < len; j += 4) {
      const uint4 r = *reinterpret_cast<const uint4*>(&s_row[j]);
      later |= (j > tid && r.x == mine) | (j + 1 > tid && r.y == mine) | (j + 2 > tid && r.z == mine) |
               (j + 3 > tid && r.w == mine);
    }
    if (in && !later) {
      const uint32_t v = kTd ? prio_td_leaf(td, i) : prio_clamp(leaf_in[i]);
      leaf[row] = v;
      mx = one_chunk && v > mx ? v : mx;
    }
    __threadfence();
    __syncthreads();  // s_row is rewritten; the next chunk's stores come after this one's
  }
  if (!one_chunk) {
    for (int64_t i = tid; i < batch; i += kPrioMemberThreads) {
      const int64_t row = idx[i];
      if (row < 0 || row >= M) continue;
      const uint32_t v = kTd ? prio_td_leaf(td, i) : prio_clamp(leaf_in[i]);
      mx = leaf[row] == v && v > mx ? v : mx;
    }
  }
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t u = __shfl_xor(mx, d, kWave);
    mx = u > mx ? u : mx;
  }
  if (lane == 0) s_max[wv] = mx;
  __syncthreads();
  if (tid == 0) {
    PrioHeader* h = prio_header(slab);
    uint32_t v = h->max_leaf;
    for (int q = 0; q < kPrioMemberThreads / kWave; ++q) v = s_max[q] > v ? s_max[q] : v;
    h->max_leaf = v;
  }
}

// ---- the draw: grid (ceil(batch / 4), P) x 256, one wave per slot
__device__ __forceinline__ void prio_draw_body(const PT& t, char* slab, uint32_t m, int batch, int64_t call,
                                               uint64_t seed, int64_t* __restrict__ idx,
                                               uint32_t* __restrict__ leaf_out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t j = (int64_t)blockIdx.x * (kPrioThreads / kWave) + threadIdx.x / kWave;
  if (j >= batch) return;
  const PrioHeader* h = prio_header(slab);
  const uint64_t T = h->total, B = (uint64_t)batch, uj = (uint64_t)j;
  if (T == 0) {
    if (lane == 0) {
      idx[j] = -1;
      leaf_out[j] = 0u;
    }
    return;
  }
  const uint64_t q = T / B, r = T - q * B;  // r, j < 2^31: r (j + 1) < 2^62
  const uint64_t lo = q * uj + r * uj / B, hi = q * (uj + 1) + r * (uj + 1) / B;
  uint64_t ctr[4] = {uj, (uint64_t)(call >= 0 ? call : h->calls), (uint64_t)m, 0ull};
  philox4x64_10(ctr, seed, SACENV_REPLAY_PRIO_KEY1);
  uint64_t tt = lo + __umul64hi(ctr[0], hi - lo);
  int64_t node = 0;
  uint64_t v = 0;
  bool found = true;
#pragma unroll
  for (int k = kPrioLevels - 1; k >= 0; --k) {
    if (k >= t.levels) continue;
    v = prio_entry(slab, t.offset[k], t.count[k], k == 0, node * kPrioFan + lane);
    const uint64_t incl = wave_scan64(v, lane);
    const unsigned long long hit = __ballot(incl > tt);
    if (hit == 0ull) {  // (a tree that does not add up: a caller's own writes)
      found = false;
      break;
    }
    const int f = __ffsll(hit) - 1;
    tt -= __shfl((unsigned long long)(incl - v), f, kWave);
    v = __shfl((unsigned long long)v, f, kWave);
    node = node * kPrioFan + f;
  }
  if (lane == 0) {
    idx[j] = found ? node : -1;
    leaf_out[j] = found ? (uint32_t)v : 0u;
  }
}

// ---- after the draw: grid (1, P) x 1 024 (a pow per thread at batch 1 024). weights = (min leaf / leaf)^beta, and the count's advance
// kAnneal (include/sacenv_weighted_learn.h): beta runs from b.beta to b.beta1 over b.anneal samples,
// by the sample's number -- b.call, or the slab's count from BEFORE this sample's advance, which
// thread 0 reads once and hands to the others through LDS before it advances
struct PrioBeta {
  double beta, beta1;
  int64_t anneal, call;
};

template <bool kAnneal>
__device__ __forceinline__ void prio_finish_body(char* slab, int batch, const uint32_t* __restrict__ leaf_out,
                                                 float* __restrict__ weights, const PrioBeta& b, bool advance) {
  __shared__ uint32_t s_min[kPrioMemberThreads / kWave];
  __shared__ int64_t s_calls;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  double beta = b.beta;
  if (kAnneal) {
    int64_t k = b.call;
    if (k < 0) {
      if (tid == 0) s_calls = prio_header(slab)->calls;
      __syncthreads();
      k = s_calls;
    }
    k = k < b.anneal ? k : b.anneal;
    beta = b.beta + (b.beta1 - b.beta) * ((double)k / (double)b.anneal);
  }
  if (advance && tid == 0) prio_header(slab)->calls += 1;
  if (weights == nullptr) return;
  uint32_t mn = 0xFFFFFFFFu;
  for (int i = tid; i < batch; i += kPrioMemberThreads) {
    const uint32_t v = leaf_out[i];
    mn = v < mn ? v : mn;
  }
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t u = __shfl_xor(mn, d, kWave);
    mn = u < mn ? u : mn;
  }
  if (lane == 0) s_min[wv] = mn;
  __syncthreads();
  for (int q = 0; q < kPrioMemberThreads / kWave; ++q) mn = s_min[q] < mn ? s_min[q] : mn;
  for (int i = tid; i < batch; i += kPrioMemberThreads) {
    const uint32_t v = leaf_out[i];
    weights[i] = v == 0u ? 0.f : (float)pow((double)mn / (double)v, beta);
  }
}

inline PT make_pt(const SacenvReplayParams& p, void* state) {
  SacenvReplayPrioLayout L;
  prio_layout(p.mem_size, &L);
  PT t;
  t.b = static_cast<char*>(state);
  t.member_bytes = L.member_bytes;
  t.levels = L.levels;
  t.pad = 0;
  for (int k = 0; k < kPrioLevels; ++k) {
    t.count[k] = L.count[k];
    t.offset[k] = L.offset[k];
  }
  return t;
}

}  // namespace
