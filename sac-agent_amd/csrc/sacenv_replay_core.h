// sacenv_replay_core.h — what the one-buffer unit (sacenv_replay.hip) and the population
// unit (sacenv_replay_pop.hip) share: the constants, the arena layout, RB, the device
// bodies of the five one-buffer kernels, the sharded and staged geometry, the pieces every
// draw and gather is built from (block_rank; draw_open / fill_masked / draw_close on the
// MT19937 block twist; gather_split), and the host rules both units apply (the parameter
// and call checks, the store's and the gather's grid). No kernel and no entry point lives
// here: each unit wraps the bodies in its own kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sacenv.h"
#include "sacenv_wave_core.h"   // kWave, status()

#include "mt19937.h"

namespace {

__host__ __device__ inline int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }

__host__ __device__ inline void replay_layout(const SacenvReplayParams& p, SacenvReplayLayout* o) {
  const int64_t M = p.mem_size;
  int64_t off = 0;
  o->state = off;
  off = align256(off + 4 * M * p.obs_dim);
  o->new_state = off;
  off = align256(off + 4 * M * p.obs_dim);
  o->action = off;
  off = align256(off + 4 * M * p.act_dim);
  o->reward = off;
  off = align256(off + 8 * M);
  o->terminal = off;
  off = align256(off + M);
  o->mem_cntr = off;
  off += 256;
  o->mt_key = off;
  off = align256(off + 4 * kMtN);
  o->mt_pos = off;
  off += 256;
  o->total_bytes = off;
}

struct RB {
  char* b;
  SacenvReplayLayout L;
  __device__ float* state() const { return reinterpret_cast<float*>(b + L.state); }
  __device__ float* new_state() const { return reinterpret_cast<float*>(b + L.new_state); }
  __device__ float* action() const { return reinterpret_cast<float*>(b + L.action); }
  __device__ double* reward() const { return reinterpret_cast<double*>(b + L.reward); }
  __device__ uint8_t* terminal() const { return reinterpret_cast<uint8_t*>(b + L.terminal); }
  __device__ int64_t* cntr() const { return reinterpret_cast<int64_t*>(b + L.mem_cntr); }
  __device__ uint32_t* key() const { return reinterpret_cast<uint32_t*>(b + L.mt_key); }
  __device__ int32_t* pos() const { return reinterpret_cast<int32_t*>(b + L.mt_pos); }
};

// The bodies of the five one-buffer kernels are device functions: sacenv_replay.hip wraps
// each in a kernel, and sacenv_replay_pop.hip runs them under a second grid dimension over
// the members of a population. They index by blockIdx.x / gridDim.x only.
__device__ __forceinline__ void init_body(const RB& r, uint32_t seed) {
  if (threadIdx.x != 0) return;
  uint32_t x = seed;  // init_genrand (numpy RandomState._legacy_seeding)
  for (int i = 0; i < kMtN; ++i) {
    r.key()[i] = x;
    x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)(i + 1);
  }
  *r.pos() = kMtN;
  *r.cntr() = 0;
}

// store_transition for rows [0, n): row i -> (mem_cntr + i) % M. Rows that a
// later row of the same call overwrites (i < n - M) are skipped, so the ring
// ends exactly as n sequential calls leave it. Element-parallel over the
// (n - first) x (D + A + 1) stored columns with 32-bit index math. mem_cntr
// advances in a second launch (k_rb_advance), after every workgroup has read
// it: stream order instead of a grid-wide atomic (one word takes ~90
// returning atomics/µs) or an agent-scope acq_rel fence per workgroup. With the
// count from the host (host_cntr >= 0) no workgroup reads it, so the first one
// writes the advanced count and the second launch goes (one fixed launch cost,
// ~5 us, per stored step).
__device__ __forceinline__ void store_body(const SacenvReplayParams& p, const RB& r, int64_t host_cntr,
                                           int64_t advance, int64_t n, int64_t offset,
                                           const float* __restrict__ state, const float* __restrict__ action,
                                           const void* __restrict__ reward, const float* __restrict__ new_state,
                                           const float* __restrict__ final_state, const uint8_t* __restrict__ code,
                                           uint8_t* __restrict__ last_term) {
  const int64_t M = p.mem_size, c0 = (host_cntr >= 0 ? host_cntr : *r.cntr()) + offset;
  if (host_cntr >= 0 && blockIdx.x == 0 && threadIdx.x == 0) *r.cntr() = host_cntr + advance;  // buffer.py:22
  const int64_t first = n > M ? n - M : 0;
  const uint32_t rows = (uint32_t)(n - first);
  const uint32_t base = (uint32_t)((c0 + first) % M);  // ring row of stored row 0
  const uint32_t D = (uint32_t)p.obs_dim, A = (uint32_t)p.act_dim, Mu = (uint32_t)M;
  const uint32_t nD = rows * D, nA = rows * A, stored = nD + nA + rows;
  // with last_term, rows a later row overwrites still update their env's byte
  const uint32_t total = stored + (last_term != nullptr ? (uint32_t)first : 0u);
  for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < total; q += gridDim.x * blockDim.x) {
    if (q < nD) {
      const uint32_t j = q / D, k = q - j * D;
      uint32_t row = base + j;
      row = row >= Mu ? row - Mu : row;
      const int64_t src = (first + j) * (int64_t)D + k;
      r.state()[(int64_t)row * D + k] = state[src];
      const float* ns = (final_state != nullptr && code[first + j] != 0) ? final_state : new_state;
      r.new_state()[(int64_t)row * D + k] = ns[src];
    } else if (q < nD + nA) {
      const uint32_t qq = q - nD, j = qq / A, k = qq - j * A;
      uint32_t row = base + j;
      row = row >= Mu ? row - Mu : row;
      r.action()[(int64_t)row * A + k] = action[(first + j) * (int64_t)A + k];
    } else if (q < stored) {
      const uint32_t j = q - nD - nA;
      uint32_t row = base + j;
      row = row >= Mu ? row - Mu : row;
      const int64_t i = first + j;
      r.reward()[row] = p.reward_f32 ? (double)static_cast<const float*>(reward)[i]
                                     : static_cast<const double*>(reward)[i];
      uint32_t cd = code[i];
      if (last_term != nullptr) {
        // main.py:83 tests info['termination'], which only the termination
        // chain writes (boat_env.py:84-105) and reset never clears (:120-126):
        // codes 1..5 overwrite env i's last termination, others keep it
        if (cd >= 1u && cd <= 5u) last_term[i] = (uint8_t)cd;
        else cd = last_term[i];
      }
      r.terminal()[row] = (uint8_t)((p.terminal_mask >> (cd < 31 ? cd : 31)) & 1u);
    } else {
      const int64_t i = q - stored;  // a row the ring drops: only its env's byte
      const uint32_t cd = code[i];
      if (cd >= 1u && cd <= 5u) last_term[i] = (uint8_t)cd;
    }
  }
}

__device__ __forceinline__ void advance_body(const RB& r, int64_t n) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *r.cntr() += n;  // buffer.py:22
}

// np.random.choice(max_mem, batch) with replace=True, p=None: numpy legacy
// randint(0, max_mem) -> masked rejection on 32-bit words (rng = max_mem-1;
// rng == 0 draws nothing); words in order, accepted words fill the batch in
// order, the stream stops after the batch-th accepted word: k_rb_draw_many below
// (one 1 024-thread workgroup).

// Sharded rows (sacenv_replay_sample_shard): ring row p holds the transition
// with the latest global sequence number s <= mem_cntr - 1, s = p (mod M); this
// shard wrote it iff (s mod period) is in [lo, hi). Rows of other shards come
// out as zero bits.
struct Shard {
  int64_t period, lo, hi;  // period 0: every row is this shard's
};
__device__ __forceinline__ bool owns(const Shard& sh, int64_t cnt, int64_t M, int64_t row) {
  if (sh.period == 0) return true;
  const int64_t s = row + M * ((cnt - 1 - row) / M);
  const int64_t u = s % sh.period;
  return u >= sh.lo && u < sh.hi;
}

// The gather's column split, one thread per output element: thread q of the grid maps to
// (state / new_state | action | reward + terminal, sampled row i, column k), and `at` resolves
// idx[i] to a GatherRow -- the slab the row lies in, the row, and whether it is there at all (a
// row that is not reads nothing: zero bits). Outputs are [..][batch][..] with this call's
// rows from row out0 on; a null output is skipped.
struct GatherRow {
  RB rb;
  int64_t row;
  bool in;
};
template <class At>
__device__ __forceinline__ void gather_split(const SacenvReplayParams& p, int batch, const int64_t* __restrict__ idx,
                                             int64_t out0, float* __restrict__ st, float* __restrict__ ac,
                                             double* __restrict__ rw, float* __restrict__ ns,
                                             uint8_t* __restrict__ tm, const At& at) {
  const int D = p.obs_dim, A = p.act_dim;
  const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t nd = (int64_t)batch * D, na = (int64_t)batch * A;
  int64_t i, k;
  int part;
  if (q < nd) {
    i = q / D, k = q - i * D, part = 0;
  } else if (q < nd + na) {
    const int64_t qq = q - nd;
    i = qq / A, k = qq - i * A, part = 1;
  } else if (q < nd + na + batch) {
    i = q - nd - na, k = 0, part = 2;
  } else {
    return;
  }
  const GatherRow g = at(idx[i]);
  const int64_t row = g.row, o = out0 + i;
  if (part == 0) {
    if (st) st[o * D + k] = g.in ? g.rb.state()[row * D + k] : 0.f;
    if (ns) ns[o * D + k] = g.in ? g.rb.new_state()[row * D + k] : 0.f;
  } else if (part == 1) {
    if (ac) ac[o * A + k] = g.in ? g.rb.action()[row * A + k] : 0.f;
  } else {
    if (rw) rw[o] = g.in ? g.rb.reward()[row] : 0.0;
    if (tm) tm[o] = g.in ? g.rb.terminal()[row] : (uint8_t)0;
  }
}

// one buffer's ring rows: a row of the ring that this shard wrote (an index outside the ring
// -- a caller's, sacenv_replay_gather -- reads nothing)
__device__ __forceinline__ void gather_body(const SacenvReplayParams& p, const RB& r, int batch,
                                            const int64_t* __restrict__ idx, float* __restrict__ st,
                                            float* __restrict__ ac, double* __restrict__ rw,
                                            float* __restrict__ ns, uint8_t* __restrict__ tm, const Shard& sh) {
  const int64_t cnt = *r.cntr(), M = p.mem_size;
  gather_split(p, batch, idx, 0, st, ac, rw, ns, tm, [&](int64_t row) {
    return GatherRow{r, row, row >= 0 && row < M && owns(sh, cnt, M, row)};
  });
}

// ---------------------------------------------------------------------------
// The staged sampler: the pooled buffer of main.py:78-90 -- every rank's envs
// storing one transition each per step, one learn() (sample_buffer,
// buffer.py:24-35) after every step -- sampled out of the rows the persistent
// step launch wrote (sacenv_boat_segment's `stage`), with no ring. A ring of M
// rows that takes `period` rows per step holds the last M sequence numbers;
// with M <= seg * period every row learn k of segment g can reach (and the row
// before it, for s) lies in segment g or g - 1, so two staged segments ARE the
// ring. The index draws depend only on the sampling stream and the counts
// stored, so segment g's are drawn before it steps, and the launch writes only
// the rows some learn will read (sacenv_replay_stage_mark).

struct StagedGeom {
  int64_t period, offset, g;
  int n, n_pad, seg, exp2;
  double r_mem, r_period;  // 1 / mem_size, 1 / period (host IEEE divisions)
};

// floor(x / d) for 0 <= x < 2^52 and 0 < d < 2^31 from the rounded reciprocal rd:
// the double estimate is off by at most one, fixed by one step each way (a 64-bit
// integer division is a ~50-instruction sequence on the GPU)
__device__ __forceinline__ int64_t div_floor(int64_t x, int64_t d, double rd) {
  int64_t q = (int64_t)((double)x * rd);
  q -= q * d > x ? 1 : 0;
  q += (q + 1) * d <= x ? 1 : 0;
  return q;
}

// The staged segment buffers are ENV-MAJOR (round 6): env e's 64-B row of step j of a
// segment at (e x seg + j) x 64, its mark bits in the ceil(seg / 64) words from e x
// that, bit j % 64 -- a row and its predecessor (the row before it: its s) share a
// mark word (one atomic) and mostly a 128-B line.
__device__ __forceinline__ int64_t stage_row(const StagedGeom& G, int e, int64_t j) {
  return ((int64_t)e * G.seg + j) * 64;
}
__device__ __forceinline__ void mark_rows(unsigned long long* __restrict__ marks, const StagedGeom& G, int e,
                                          int64_t j, unsigned long long bits) {
  const int W = (G.seg + 63) / 64;
  atomicOr(&marks[(int64_t)e * W + (j >> 6)], bits << (j & 63));
}

// ring row `row` at learn time (cntr rows stored) -> (global step q, global env u)
__device__ __forceinline__ void resolve(int64_t row, int64_t cntr, int64_t M, const StagedGeom& G, int64_t* q,
                                        int64_t* u) {
  // the latest sequence number = row (mod M) below cntr
  const int64_t s = row + M * div_floor(cntr - 1 - row, M, G.r_mem);
  *q = div_floor(s, G.period, G.r_period);
  *u = s - *q * G.period;
}

// The draws walk one MT19937 stream per buffer with one 1 024-thread workgroup: a whole
// 624-word block is tempered and tested at once (thread i: word i), and accepted words are
// ranked with a ballot per wave and a prefix over the waves.
constexpr int kDrawThreads = 1024;
__device__ __forceinline__ void mt_twist_block(const uint32_t* __restrict__ o, uint32_t* __restrict__ n, int tid) {
  constexpr int kD = kMtN - kMtM;  // 227
  if (tid < kD) n[tid] = mt_mix(o[tid], o[tid + 1], o[tid + kMtM]);
  __syncthreads();
  if (tid < kD) n[kD + tid] = mt_mix(o[kD + tid], o[kD + tid + 1], n[tid]);
  __syncthreads();
  if (tid < kMtN - 1 - 2 * kD) n[2 * kD + tid] = mt_mix(o[2 * kD + tid], o[2 * kD + tid + 1], n[kD + tid]);
  __syncthreads();
  if (tid == 0) n[kMtN - 1] = mt_mix(o[kMtN - 1], n[0], n[kMtM - 1]);
  __syncthreads();
}

// The taking threads of a kThreads-thread workgroup before this one, its waves in order:
// returns the exclusive rank, *total the workgroup's count. One barrier; wcnt (LDS
// [kThreads / kWave]) is free again after the caller's next barrier.
template <int kThreads>
__device__ __forceinline__ int block_rank(bool take, int* wcnt, int* total) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  const unsigned long long bal = __ballot(take);
  if (lane == 0) wcnt[wv] = __popcll(bal);
  __syncthreads();
  int before = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < kThreads / kWave; ++w) {
    const int c = wcnt[w];
    before += w < wv ? c : 0;
    sum += c;
  }
  *total = sum;
  return before + __popcll(bal & ((1ull << lane) - 1ull));
}

// A workgroup's view of one buffer's stream while it draws: the key block pair in LDS, the
// position of the next word in blk[cur], and whether blk[cur] is no longer the arena's key.
struct DrawBlock {
  uint32_t (*blk)[kMtN];  // LDS [2][kMtN]
  int* wcnt;              // LDS [kDrawThreads / kWave]
  int* s_end;             // LDS
  int cur, pos;
  bool advanced;
};

// Opens r's stream on the workgroup's LDS (one stream per workgroup): false for a poisoned
// stream (a staged draw ran short: the caller draws nothing, and the poison stays).
__device__ __forceinline__ bool draw_open(DrawBlock& d, const RB& r) {
  __shared__ uint32_t blk[2][kMtN];
  __shared__ int wcnt[kDrawThreads / kWave];
  __shared__ int s_end;
  d = DrawBlock{blk, wcnt, &s_end, 0, *r.pos(), false};
  if (d.pos < 0) return false;
  for (int i = threadIdx.x; i < kMtN; i += kDrawThreads) blk[0][i] = r.key()[i];
  __syncthreads();
  return true;
}

// the stream's state after the draws: the key if a fill twisted it, and the position
__device__ __forceinline__ void draw_close(const DrawBlock& d, const RB& r) {
  if (d.advanced)
    for (int i = threadIdx.x; i < kMtN; i += kDrawThreads) r.key()[i] = d.blk[d.cur][i];
  if (threadIdx.x == 0) *r.pos() = d.pos;
}

// One masked-rejection fill: `count` accepted words (w & mask <= rng, rng >= 1) from position
// d.pos on, in order, to put(0 .. count - 1, w); the stream stops after the last accepted word
// (the word 623 of a block leaves pos = 624: the next fill twists first). A block that holds
// fewer than the words still wanted is taken whole and the next one twisted. Every thread of
// the workgroup calls it with the same arguments, and fills with different ranges and counts
// run back to back on one stream.
// Two barriers a round -- block_rank's, and one after s_end is written and wcnt read -- and a
// third in the round that ends the fill, after s_end is read. The third is not needed for
// the LDS traffic: whoever writes s_end next (the next fill's first round) does so behind
// that round's block_rank barrier, which no thread passes before every thread has read s_end
// here, and wcnt's next writer is behind the second barrier, as in every round. It stays
// because without it the compiler peels the first round out of the loop (each fill's code
// x 1.4).
template <class Put>
__device__ __forceinline__ void fill_masked(DrawBlock& d, uint32_t rng, int count, const Put& put) {
  const int tid = threadIdx.x;
  const uint32_t mask = range_mask32(rng);
  int filled = 0;
  for (;;) {
    if (d.pos >= kMtN) {
      mt_twist_block(d.blk[d.cur], d.blk[d.cur ^ 1], tid);
      d.cur ^= 1;
      d.pos = 0;
      d.advanced = true;
    }
    const bool valid = tid >= d.pos && tid < kMtN;
    const uint32_t w = valid ? (mt_temper(d.blk[d.cur][tid]) & mask) : 0u;
    const bool acc = valid && w <= rng;
    int total;
    const int rank = block_rank<kDrawThreads>(acc, d.wcnt, &total);
    const int take = count - filled;
    if (acc && rank < take) put(filled + rank, w);
    const bool done = total >= take;  // the take-th accepted word ends the fill
    if (done && acc && rank == take - 1) *d.s_end = tid;
    __syncthreads();
    if (done) {
      d.pos = *d.s_end + 1;
      __syncthreads();  // (see above)
      return;
    }
    filled += total;
    d.pos = kMtN;
  }
}

// n_batches consecutive np.random.choice(min(cntr_k, M), batch) calls on one stream, one fill
// each. kSample: one sample_buffer(batch) at the device count (sacenv_replay_sample: no
// learn() skip below batch rows; graph-capturable like the store), else the nb learns of a
// staged segment at counts cntr_k = cntr0 + (k + 1) * period (learn k follows step k's
// stores), learns with cntr_k < batch skipped (continuous_agent.py:97-98: idx = -1, no words).
template <bool kSample>
__device__ __forceinline__ void draw_many_body(const SacenvReplayParams& p, const RB& r, int batch, int nb,
                                               int64_t cntr0, int64_t period, int64_t* __restrict__ idx) {
  const int tid = threadIdx.x;
  DrawBlock d;
  if (!draw_open(d, r)) {
    for (int64_t i = tid; i < (int64_t)nb * batch; i += kDrawThreads) idx[i] = -1;
    return;
  }
  for (int k = 0; k < nb; ++k) {
    const int64_t c = kSample ? *r.cntr() : cntr0 + (int64_t)(k + 1) * period;
    const int64_t max_mem = c < p.mem_size ? c : p.mem_size;
    const uint32_t rng = (uint32_t)(max_mem - 1);
    const bool skip = !kSample && c < batch;
    int64_t* const out = idx + (int64_t)k * batch;
    if (skip || rng == 0u) {  // learn() returns before sampling, or numpy's off + 0: no words
      for (int i = tid; i < batch; i += kDrawThreads) out[i] = skip ? -1 : 0;
      continue;
    }
    fill_masked(d, rng, batch, [&](int i, uint32_t w) { out[i] = (int64_t)w; });
  }
  draw_close(d, r);
}

int check_replay(const SacenvReplayParams* p) {
  if (p == nullptr) return SACENV_E_NULL;
  if (p->mem_size <= 0 || p->mem_size > 0x7FFFFFFFLL || p->obs_dim <= 0 || p->act_dim <= 0)
    return SACENV_E_SIZE;  // 32-bit ring rows; randint on 32-bit words
  return SACENV_OK;
}

// The store's grid for n rows per buffer: the min(n, M) rows the ring keeps x (D + A + 1)
// columns, and with last_term one element per row it drops; at most 8192 blocks of 256
// (store_body strides).
inline int store_grid(const SacenvReplayParams* p, int64_t n, const uint8_t* last_term, int64_t* blocks) {
  const int64_t rows = n > p->mem_size ? p->mem_size : n;
  const int64_t total = rows * ((int64_t)p->obs_dim + p->act_dim + 1) + (last_term ? n - rows : 0);
  if (total >= (1LL << 32)) return SACENV_E_SIZE;  // 32-bit element index per buffer and call
  *blocks = (total + 255) / 256;
  if (*blocks > 8192) *blocks = 8192;
  return SACENV_OK;
}

// a buffer's elements of one sample or gather, and the gather's grid.x: one thread each
inline int64_t batch_elems(const SacenvReplayParams* p, int32_t batch) {
  return (int64_t)batch * ((int64_t)p->obs_dim + p->act_dim + 1);
}
inline unsigned gather_blocks(const SacenvReplayParams* p, int32_t batch) {
  return (unsigned)((batch_elems(p, batch) + 255) / 256);
}

// the argument rules of the sample / gather family, after the parameters' (a gather has no
// `stored`)
inline int check_batch_call(const void* arena, const int64_t* idx, int32_t batch, int64_t stored = 1) {
  if (batch < 0) return SACENV_E_SIZE;
  if (stored <= 0) return SACENV_E_SIZE;  // np.random.choice(0, n) raises
  if (arena == nullptr || idx == nullptr) return SACENV_E_NULL;
  return SACENV_OK;
}

RB make_rb(const SacenvReplayParams& p, void* arena) {
  RB r;
  r.b = static_cast<char*>(arena);
  replay_layout(p, &r.L);
  return r;
}

}  // namespace
