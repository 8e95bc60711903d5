// sacenv_replay_pop.hip — the replay buffers of a population in one set of launches
// (include/sacenv_population_replay.h; the buffers of the reference's hyper-parameter
// search, main.py -p N: one agent/buffer.py ring and one np.random stream per agent).
//
// P buffers: the one-buffer kernels of sacenv_replay.hip with a second grid dimension
// over the members. Member m = blockIdx.y runs init_body / store_body / advance_body /
// draw_many_body<true> / gather_body, unchanged, on its own RB -- the launch's RB
// (member 0's base and the layout all members share) with the base moved by m x
// member_bytes -- and on its own rows of the [P][n][..] inputs and [P][batch][..]
// outputs. The bodies index by blockIdx.x / gridDim.x only. No per-member struct is
// indexed by a run-time value (that costs scratch); the one
// per-member table, the seeds of the init launch, is read from the kernel arguments
// with scalar loads at an SGPR offset, as PopArgs is in sacenv_sac_pop.hip.
//
// Every draw and gather of both units is built from one set of pieces in
// sacenv_replay_core.h: draw_open / fill_masked / draw_close -- the
// stream in LDS, numpy's masked-rejection round, the write-back -- under block_rank, and
// gather_split, the column split and the five stores over a resolver from an index to
// (slab, row, valid). This is a translation unit of its own all the same: the one-buffer
// kernels, and above all the staged, side and stand-in kernels of the timed replay path,
// are compiled where they were, alone (tools/kernel_diff.py; DESIGN.md §4.6.1 has the
// result and the resource table).
//
// The pooled sample (include/sacenv_population_share.h) lives here too: two
// kernels of their own, k_rb_draw_pool and k_rb_gather_pool, after the five above.
//
// The prioritized sample (include/sacenv_prioritized_replay.h) has its entry points
// at the end; its device code is sacenv_replay_prio.h, and its gather is k_rb_gather_pop above.
// The annealed sample of include/sacenv_weighted_learn.h is the same launches with one more argument.
#include "sacenv_replay_core.h"

#include "sacenv_population_replay.h"
#include "sacenv_population_share.h"
#include "sacenv_replay_prio.h"
#include "sacenv_weighted_learn.h"   // (the annealed prioritized sample, the last entry point here)

namespace {

constexpr int kRbPopMax = SACENV_REPLAY_POP_MAX_MEMBERS;

struct PopSeeds {
  uint32_t v[kRbPopMax];
};

__device__ __forceinline__ RB member_rb(const RB& r, int64_t member_bytes, int64_t m) {
  RB rm = r;
  rm.b = r.b + m * member_bytes;
  return rm;
}

// grid (1, P)
__global__ void __launch_bounds__(kWave) k_rb_init_pop(RB r, int64_t member_bytes, PopSeeds seeds) {
  init_body(member_rb(r, member_bytes, blockIdx.y), seeds.v[blockIdx.y]);
}

// grid (min(blocks, 8192), P): member m's n rows of the [P][n][..] inputs
__global__ void __launch_bounds__(256) k_rb_store_pop(SacenvReplayParams p, RB r, int64_t member_bytes,
                                                      int64_t host_cntr, int64_t advance, int64_t n,
                                                      const float* __restrict__ state,
                                                      const float* __restrict__ action,
                                                      const void* __restrict__ reward,
                                                      const float* __restrict__ new_state,
                                                      const float* __restrict__ final_state,
                                                      const uint8_t* __restrict__ code,
                                                      uint8_t* __restrict__ last_term) {
  const int64_t m = blockIdx.y, rows = m * n, D = p.obs_dim, A = p.act_dim;
  store_body(p, member_rb(r, member_bytes, m), host_cntr, advance, n, 0, state + rows * D, action + rows * A,
             static_cast<const char*>(reward) + rows * (p.reward_f32 ? 4 : 8), new_state + rows * D,
             final_state != nullptr ? final_state + rows * D : nullptr, code + rows,
             last_term != nullptr ? last_term + rows : nullptr);
}

// grid (1, P)
__global__ void k_rb_advance_pop(RB r, int64_t member_bytes, int64_t n) {
  advance_body(member_rb(r, member_bytes, blockIdx.y), n);
}

// grid (1, P) x 1 024 threads: one workgroup per member, each on its own key, position and count
__global__ void __launch_bounds__(kDrawThreads) k_rb_draw_pop(SacenvReplayParams p, RB r, int64_t member_bytes,
                                                              int batch, int64_t* __restrict__ idx) {
  const int64_t m = blockIdx.y;
  draw_many_body<true>(p, member_rb(r, member_bytes, m), batch, 1, 0, 0, idx + m * batch);
}

// grid (ceil(batch x (D + A + 1) / 256), P): member m's rows into the [P][batch][..] outputs
__global__ void __launch_bounds__(256) k_rb_gather_pop(SacenvReplayParams p, RB r, int64_t member_bytes, int batch,
                                                       const int64_t* __restrict__ idx, float* __restrict__ st,
                                                       float* __restrict__ ac, double* __restrict__ rw,
                                                       float* __restrict__ ns, uint8_t* __restrict__ tm) {
  const int64_t m = blockIdx.y, rows = m * batch, D = p.obs_dim, A = p.act_dim;
  gather_body(p, member_rb(r, member_bytes, m), batch, idx + rows, st != nullptr ? st + rows * D : nullptr,
              ac != nullptr ? ac + rows * A : nullptr, rw != nullptr ? rw + rows : nullptr,
              ns != nullptr ? ns + rows * D : nullptr, tm != nullptr ? tm + rows : nullptr, Shard{0, 0, 0});
}

// ---------------------------------------------------------------------------
// The pooled sample (include/sacenv_population_share.h): member m draws B - K rows of its own
// ring and K rows of the whole arena from its own stream, and the gather reads each row from
// its owner's slab. The draw is two fills of the shared masked-rejection round (fill_masked)
// between one draw_open and one draw_close, the gather a second resolver over gather_split.

// RandomState_m.choice(s, batch - pool) then RandomState_m.choice(P * s, pool) on member m's
// stream at its own count, as global rows owner * M + row into idx[0, batch). One workgroup.
__device__ __forceinline__ void draw_pool_body(const SacenvReplayParams& p, const RB& r, uint32_t m, uint32_t P,
                                               int batch, int pool, int64_t* __restrict__ idx) {
  const int tid = threadIdx.x;
  DrawBlock d;
  if (!draw_open(d, r)) {
    for (int i = tid; i < batch; i += kDrawThreads) idx[i] = -1;
    return;
  }
  const int64_t M = p.mem_size, c = *r.cntr();
  const uint32_t s = (uint32_t)(c < M ? c : M);  // 1 <= s < 2^31 (the host refuses an empty ring)
  const int own = batch - pool;
  const int64_t base = (int64_t)m * M;
  if (own > 0) {
    if (s <= 1u) {  // numpy's off + 0: no words
      for (int i = tid; i < own; i += kDrawThreads) idx[i] = base;
    } else {
      fill_masked(d, s - 1u, own, [&](int i, uint32_t w) { idx[i] = base + (int64_t)w; });
    }
  }
  if (pool > 0) {
    const uint64_t range = (uint64_t)P * s;  // <= 2^32 (the host's rule), so rng fits 32 bits
    int64_t* __restrict__ out = idx + own;
    if (range <= 1u) {
      for (int i = tid; i < pool; i += kDrawThreads) out[i] = 0;
    } else {
      fill_masked(d, (uint32_t)(range - 1u), pool, [&](int i, uint32_t g) {
        const uint32_t owner = g / s;  // g < P * s: owner < P, row < s <= M
        out[i] = (int64_t)owner * M + (int64_t)(g - owner * s);
      });
    }
  }
  draw_close(d, r);
}

// grid (1, P) x 1 024 threads: one workgroup per member, each on its own key, position and count
__global__ void __launch_bounds__(kDrawThreads) k_rb_draw_pool(SacenvReplayParams p, RB r, int64_t member_bytes,
                                                               int batch, int pool, int64_t* __restrict__ idx) {
  const int64_t m = blockIdx.y;
  draw_pool_body(p, member_rb(r, member_bytes, m), (uint32_t)m, gridDim.y, batch, pool, idx + m * batch);
}

// grid (ceil(batch x (D + A + 1) / 256), P): member m's rows of the [P][batch][..] outputs; the
// row at global index g is row g % M of slab g / M; g outside [0, P x M) gives zero bits.
// P x M <= 2^32 and M < 2^31: 32-bit division.
__global__ void __launch_bounds__(256) k_rb_gather_pool(SacenvReplayParams p, RB r, int64_t member_bytes, int batch,
                                                        const int64_t* __restrict__ idx, float* __restrict__ st,
                                                        float* __restrict__ ac, double* __restrict__ rw,
                                                        float* __restrict__ ns, uint8_t* __restrict__ tm) {
  const int64_t rows = (int64_t)blockIdx.y * batch, top = (int64_t)gridDim.y * p.mem_size;
  const uint32_t M = (uint32_t)p.mem_size;
  gather_split(p, batch, idx + rows, rows, st, ac, rw, ns, tm, [&](int64_t g) {
    const bool in = g >= 0 && g < top;
    const uint32_t gu = in ? (uint32_t)g : 0u, owner = gu / M;
    return GatherRow{member_rb(r, member_bytes, owner), (int64_t)(gu - owner * M), in};
  });
}

int rb_pop_check(const SacenvReplayParams* p, int32_t members) {
  const int rc = check_replay(p);
  if (rc) return rc;
  if (members < 1 || members > kRbPopMax) return SACENV_E_SIZE;
  return SACENV_OK;
}

bool aligned256(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 255u) == 0u; }

int gather_pop(const SacenvReplayParams* p, int32_t members, const RB& r, int32_t batch, const int64_t* idx,
               float* state, float* action, double* reward, float* new_state, uint8_t* terminal, void* stream) {
  hipLaunchKernelGGL(k_rb_gather_pop, dim3(gather_blocks(p, batch), members), dim3(256), 0, (hipStream_t)stream, *p,
                     r, r.L.total_bytes, batch, idx, state, action, reward, new_state, terminal);
  return status();
}

// the rules of a population sample / gather: the one-buffer call's, the arena's alignment (a
// member's arena starts member_bytes, a multiple of 256, after the last) and a 32-bit count of
// a member's elements (the gather's grid.x is that count / 256)
int check_pop_batch_call(const SacenvReplayParams* p, int32_t members, const void* arena, const int64_t* idx,
                         int32_t batch, int64_t stored = 1) {
  int rc = rb_pop_check(p, members);
  if (rc || (rc = check_batch_call(arena, idx, batch, stored))) return rc;
  if (!aligned256(arena) || batch_elems(p, batch) >= (1LL << 32)) return SACENV_E_SIZE;
  return SACENV_OK;
}

}  // namespace

extern "C" int sacenv_replay_pop_layout(const SacenvReplayParams* p, int32_t members, SacenvReplayPopLayout* out) {
  const int rc = rb_pop_check(p, members);
  if (rc) return rc;
  if (out == nullptr) return SACENV_E_NULL;
  SacenvReplayLayout L;
  replay_layout(*p, &L);
  out->member_bytes = L.total_bytes;
  out->total_bytes = members * L.total_bytes;
  out->max_members = kRbPopMax;
  out->pad = 0;
  return SACENV_OK;
}

extern "C" int sacenv_replay_pop_init(const SacenvReplayParams* p, int32_t members, void* arena,
                                      const uint32_t* seeds, void* stream) {
  const int rc = rb_pop_check(p, members);
  if (rc) return rc;
  if (arena == nullptr || seeds == nullptr) return SACENV_E_NULL;
  if (!aligned256(arena)) return SACENV_E_SIZE;
  // One member is one buffer: its launches are the one-buffer kernels (here and in the
  // three entry points below). The population kernels take more arguments and move every
  // pointer, which P >= 2 repays and P = 1 would only pay (measured).
  if (members == 1) return sacenv_replay_init(p, arena, seeds[0], stream);
  PopSeeds s{};
  for (int m = 0; m < members; ++m) s.v[m] = seeds[m];
  const RB r = make_rb(*p, arena);
  hipLaunchKernelGGL(k_rb_init_pop, dim3(1, members), dim3(kWave), 0, (hipStream_t)stream, r, r.L.total_bytes, s);
  return status();
}

extern "C" int sacenv_replay_pop_store(const SacenvReplayParams* p, int32_t members, void* arena, int64_t cntr,
                                       int64_t n, const float* state, const float* action, const void* reward,
                                       const float* new_state, const float* final_state, const uint8_t* code,
                                       uint8_t* last_term, void* stream) {
  int rc = rb_pop_check(p, members);
  if (rc) return rc;
  if (cntr < -1) return SACENV_E_RANGE;
  if (n < 0) return SACENV_E_SIZE;
  if (n == 0) return SACENV_OK;
  if (!arena || !state || !action || !reward || !new_state || !code) return SACENV_E_NULL;
  if (!aligned256(arena)) return SACENV_E_SIZE;
  int64_t blocks;
  if ((rc = store_grid(p, n, last_term, &blocks))) return rc;
  if (members == 1)
    return cntr >= 0 ? sacenv_replay_store_env_at(p, arena, cntr, n, state, action, reward, new_state, final_state,
                                                  code, last_term, stream)
                     : sacenv_replay_store_env(p, arena, n, state, action, reward, new_state, final_state, code,
                                               last_term, stream);
  const RB r = make_rb(*p, arena);
  hipLaunchKernelGGL(k_rb_store_pop, dim3((unsigned)blocks, members), dim3(256), 0, (hipStream_t)stream, *p, r,
                     r.L.total_bytes, cntr, n, n, state, action, reward, new_state, final_state, code, last_term);
  if ((rc = status())) return rc;
  if (cntr >= 0) return SACENV_OK;  // the first workgroup of every member wrote the advanced count
  hipLaunchKernelGGL(k_rb_advance_pop, dim3(1, members), dim3(kWave), 0, (hipStream_t)stream, r, r.L.total_bytes, n);
  return status();
}

extern "C" int sacenv_replay_pop_sample(const SacenvReplayParams* p, int32_t members, void* arena, int32_t batch,
                                        int64_t stored, int64_t* idx, float* state, float* action, double* reward,
                                        float* new_state, uint8_t* terminal, void* stream) {
  int rc = check_pop_batch_call(p, members, arena, idx, batch, stored);
  if (rc) return rc;
  if (batch == 0) return SACENV_OK;
  if (members == 1)
    return sacenv_replay_sample(p, arena, batch, stored, idx, state, action, reward, new_state, terminal, stream);
  const RB r = make_rb(*p, arena);
  hipLaunchKernelGGL(k_rb_draw_pop, dim3(1, members), dim3(kDrawThreads), 0, (hipStream_t)stream, *p, r,
                     r.L.total_bytes, batch, idx);
  if ((rc = status())) return rc;
  return gather_pop(p, members, r, batch, idx, state, action, reward, new_state, terminal, stream);
}

extern "C" int sacenv_replay_pop_gather(const SacenvReplayParams* p, int32_t members, void* arena, int32_t batch,
                                        const int64_t* idx, float* state, float* action, double* reward,
                                        float* new_state, uint8_t* terminal, void* stream) {
  const int rc = check_pop_batch_call(p, members, arena, idx, batch);
  if (rc) return rc;
  if (batch == 0) return SACENV_OK;
  if (members == 1)
    return sacenv_replay_gather(p, arena, batch, idx, state, action, reward, new_state, terminal, stream);
  return gather_pop(p, members, make_rb(*p, arena), batch, idx, state, action, reward, new_state, terminal, stream);
}

// ---- include/sacenv_population_share.h

namespace {

// the family's rules (check_pop_batch_call), then the pool's own: the pool rows, and a pool of
// at most 2^32 rows (numpy's 32-bit word path; a global row as a 32-bit number in the gather)
int check_pool_call(const SacenvReplayParams* p, int32_t members, const void* arena, const int64_t* idx,
                    int32_t batch, int32_t pool_rows, int64_t stored = 1) {
  const int rc = check_pop_batch_call(p, members, arena, idx, batch, stored);
  if (rc) return rc;
  if (pool_rows < 0 || pool_rows > batch) return SACENV_E_SIZE;
  if ((int64_t)members * p->mem_size > (1LL << 32)) return SACENV_E_SIZE;
  return SACENV_OK;
}

int gather_pool(const SacenvReplayParams* p, int32_t members, const RB& r, int32_t batch, const int64_t* idx,
                float* state, float* action, double* reward, float* new_state, uint8_t* terminal, void* stream) {
  hipLaunchKernelGGL(k_rb_gather_pool, dim3(gather_blocks(p, batch), members), dim3(256), 0, (hipStream_t)stream,
                     *p, r, r.L.total_bytes, batch, idx, state, action, reward, new_state, terminal);
  return status();
}

}  // namespace

extern "C" int sacenv_replay_pop_sample_pool(const SacenvReplayParams* p, int32_t members, void* arena,
                                             int32_t batch, int32_t pool_rows, int64_t stored, int64_t* idx,
                                             float* state, float* action, double* reward, float* new_state,
                                             uint8_t* terminal, void* stream) {
  int rc = check_pool_call(p, members, arena, idx, batch, pool_rows, stored);
  if (rc) return rc;
  if (batch == 0) return SACENV_OK;
  const RB r = make_rb(*p, arena);
  hipLaunchKernelGGL(k_rb_draw_pool, dim3(1, members), dim3(kDrawThreads), 0, (hipStream_t)stream, *p, r,
                     r.L.total_bytes, batch, pool_rows, idx);
  if ((rc = status())) return rc;
  return gather_pool(p, members, r, batch, idx, state, action, reward, new_state, terminal, stream);
}

extern "C" int sacenv_replay_pop_gather_pool(const SacenvReplayParams* p, int32_t members, void* arena,
                                             int32_t batch, const int64_t* idx, float* state, float* action,
                                             double* reward, float* new_state, uint8_t* terminal, void* stream) {
  const int rc = check_pool_call(p, members, arena, idx, batch, 0);
  if (rc) return rc;
  if (batch == 0) return SACENV_OK;
  return gather_pool(p, members, make_rb(*p, arena), batch, idx, state, action, reward, new_state, terminal,
                     stream);
}

// ---- include/sacenv_prioritized_replay.h

namespace {

// grid (blocks, P)
__global__ void __launch_bounds__(256) k_prio_init(PT t) { prio_init_body(t, prio_slab(t, blockIdx.y)); }

// member m's count before the store: the host's, or the one in its arena
__device__ __forceinline__ int64_t prio_c0(const RB& r, int64_t member_bytes, int64_t host_cntr) {
  return host_cntr >= 0 ? host_cntr : *member_rb(r, member_bytes, blockIdx.y).cntr();
}

// grid (blocks, P)
__global__ void __launch_bounds__(256) k_prio_mark(PT t, RB r, int64_t member_bytes, int64_t host_cntr, int64_t n) {
  prio_mark_body(t, prio_slab(t, blockIdx.y), prio_c0(r, member_bytes, host_cntr), n);
}

// grid (ceil(W / 4), P)
__global__ void __launch_bounds__(kPrioThreads) k_prio_l1_span(PT t, RB r, int64_t member_bytes, int64_t host_cntr,
                                                               int64_t n) {
  prio_l1_span_body(t, prio_slab(t, blockIdx.y), prio_c0(r, member_bytes, host_cntr), n);
}

// grid (ceil(batch / 4), P)
__global__ void __launch_bounds__(kPrioThreads) k_prio_l1_idx(PT t, int batch, const int64_t* __restrict__ idx) {
  prio_l1_idx_body(t, prio_slab(t, blockIdx.y), batch, idx + (int64_t)blockIdx.y * batch);
}

// grid (1, P)
__global__ void __launch_bounds__(kPrioMemberThreads) k_prio_upper(PT t) {
  prio_upper_body(t, prio_slab(t, blockIdx.y));
}

// grid (1, P)
template <bool kTd>
__global__ void __launch_bounds__(kPrioMemberThreads) k_prio_write(PT t, int batch, const int64_t* __restrict__ idx,
                                                                    const uint32_t* __restrict__ leaf, PrioTd td,
                                                                    int64_t member_stride) {
  const int64_t m = blockIdx.y;
  PrioTd tm = td;
  if (kTd) {
    tm.sq1 = td.sq1 + m * member_stride;
    tm.sq2 = td.sq2 != nullptr ? td.sq2 + m * member_stride : nullptr;
  }
  prio_write_body<kTd>(t, prio_slab(t, m), batch, idx + m * batch, kTd ? nullptr : leaf + m * batch, tm);
}

// grid (ceil(batch / 4), P)
__global__ void __launch_bounds__(kPrioThreads) k_prio_draw(PT t, int batch, int64_t call, PrioSeeds seeds,
                                                            int64_t* __restrict__ idx,
                                                            uint32_t* __restrict__ leaf_out) {
  const int64_t m = blockIdx.y;
  prio_draw_body(t, prio_slab(t, m), (uint32_t)m, batch, call, seeds.v[m], idx + m * batch, leaf_out + m * batch);
}

// grid (1, P); kAnneal: the exponent by the sample's number (include/sacenv_weighted_learn.h)
template <bool kAnneal>
__global__ void __launch_bounds__(kPrioMemberThreads) k_prio_finish(PT t, int batch, const uint32_t* __restrict__ leaf_out,
                                                              float* __restrict__ weights, PrioBeta b, int advance) {
  const int64_t m = blockIdx.y;
  prio_finish_body<kAnneal>(prio_slab(t, m), batch, leaf_out + m * batch,
                            weights != nullptr ? weights + m * batch : nullptr, b, advance != 0);
}

bool finite_nonneg(double x) { return x >= 0.0 && x <= 1.7976931348623157e308; }  // (false for NaN)

// levels >= 2 and the total, after the leaves and level 1 are in place
int prio_repair_upper(const PT& t, int32_t members, void* stream) {
  hipLaunchKernelGGL(k_prio_upper, dim3(1, members), dim3(kPrioMemberThreads), 0, (hipStream_t)stream, t);
  return status();
}

// the launches of sacenv_replay_prio_set and sacenv_replay_prio_update_td
template <bool kTd>
int prio_write(const SacenvReplayParams* p, int32_t members, void* state, int32_t batch, const int64_t* idx,
               const uint32_t* leaf, const PrioTd& td, int64_t member_stride, void* stream) {
  const PT t = make_pt(*p, state);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_prio_write<kTd>, dim3(1, members), dim3(kPrioMemberThreads), 0, s, t, (int)batch, idx, leaf, td,
                     member_stride);
  if (t.levels >= 2) {
    const unsigned blocks = (unsigned)(((int64_t)batch + 3) / 4);
    hipLaunchKernelGGL(k_prio_l1_idx, dim3(blocks, members), dim3(kPrioThreads), 0, s, t, (int)batch, idx);
  }
  const int rc = status();
  return rc ? rc : prio_repair_upper(t, members, stream);
}

}  // namespace

extern "C" int sacenv_replay_prio_layout(const SacenvReplayParams* p, int32_t members, SacenvReplayPrioLayout* out) {
  const int rc = rb_pop_check(p, members);
  if (rc) return rc;
  if (out == nullptr) return SACENV_E_NULL;
  prio_layout(p->mem_size, out);
  out->total_bytes = members * out->member_bytes;
  return SACENV_OK;
}

extern "C" int sacenv_replay_prio_init(const SacenvReplayParams* p, int32_t members, void* state, void* stream) {
  const int rc = rb_pop_check(p, members);
  if (rc) return rc;
  if (state == nullptr) return SACENV_E_NULL;
  if (!aligned256(state)) return SACENV_E_SIZE;
  const PT t = make_pt(*p, state);
  int64_t blocks = (t.member_bytes / 16 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_prio_init, dim3((unsigned)blocks, members), dim3(256), 0, (hipStream_t)stream, t);
  return status();
}

extern "C" int sacenv_replay_prio_mark_stored(const SacenvReplayParams* p, int32_t members, const void* arena,
                                              void* state, int64_t cntr, int64_t n, void* stream) {
  int rc = rb_pop_check(p, members);
  if (rc) return rc;
  if (cntr < -1) return SACENV_E_RANGE;
  if (n < 0) return SACENV_E_SIZE;
  if (n == 0) return SACENV_OK;
  if (state == nullptr || (cntr < 0 && arena == nullptr)) return SACENV_E_NULL;
  if (!aligned256(state) || (cntr < 0 && !aligned256(arena))) return SACENV_E_SIZE;
  const PT t = make_pt(*p, state);
  const RB r = make_rb(*p, const_cast<void*>(arena));  // (read only, and only with cntr == -1)
  const int64_t rows = n > p->mem_size ? p->mem_size : n;
  int64_t blocks = (rows + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_prio_mark, dim3((unsigned)blocks, members), dim3(256), 0, s, t, r, r.L.total_bytes, cntr, n);
  if (t.levels >= 2) {
    int64_t waves = rows / kPrioFan + 3;  // the span's level-1 nodes: at most this many, and count[1] + 1
    if (waves > t.count[1] + 1) waves = t.count[1] + 1;
    hipLaunchKernelGGL(k_prio_l1_span, dim3((unsigned)((waves + 3) / 4), members), dim3(kPrioThreads), 0, s, t, r,
                       r.L.total_bytes, cntr, n);
  }
  if ((rc = status())) return rc;
  return prio_repair_upper(t, members, stream);
}

extern "C" int sacenv_replay_prio_set(const SacenvReplayParams* p, int32_t members, void* state, int32_t batch,
                                      const int64_t* idx, const uint32_t* leaf, void* stream) {
  const int rc = rb_pop_check(p, members);
  if (rc) return rc;
  if (batch < 0) return SACENV_E_SIZE;
  if (batch == 0) return SACENV_OK;
  if (state == nullptr || idx == nullptr || leaf == nullptr) return SACENV_E_NULL;
  if (!aligned256(state)) return SACENV_E_SIZE;
  return prio_write<false>(p, members, state, batch, idx, leaf, PrioTd{nullptr, nullptr, 0.0, 0.0}, 0, stream);
}

extern "C" int sacenv_replay_prio_update_td(const SacenvReplayParams* p, int32_t members, void* state, int32_t batch,
                                            const int64_t* idx, const float* td_sq1, const float* td_sq2,
                                            int64_t member_stride, double alpha, double eps, void* stream) {
  const int rc = rb_pop_check(p, members);
  if (rc) return rc;
  if (batch < 0 || member_stride < 0) return SACENV_E_SIZE;
  if (!finite_nonneg(alpha) || !finite_nonneg(eps)) return SACENV_E_RANGE;
  if (batch == 0) return SACENV_OK;
  if (state == nullptr || idx == nullptr || td_sq1 == nullptr) return SACENV_E_NULL;
  if (!aligned256(state)) return SACENV_E_SIZE;
  return prio_write<true>(p, members, state, batch, idx, nullptr, PrioTd{td_sq1, td_sq2, alpha, eps}, member_stride,
                          stream);
}

namespace {

// the launches of both samples, after their checks: b.anneal == 0 is the plain one
int prio_sample(const SacenvReplayParams* p, int32_t members, void* arena, void* state, int32_t batch, int64_t call,
                const uint64_t* seeds, int64_t* idx, uint32_t* leaf_out, float* weights, const PrioBeta& b, float* st,
                float* action, double* reward, float* new_state, uint8_t* terminal, void* stream) {
  if (batch == 0) return SACENV_OK;
  if (arena == nullptr || state == nullptr || seeds == nullptr || idx == nullptr || leaf_out == nullptr)
    return SACENV_E_NULL;
  if (!aligned256(arena) || !aligned256(state) || batch_elems(p, batch) >= (1LL << 32)) return SACENV_E_SIZE;
  const PT t = make_pt(*p, state);
  PrioSeeds sd{};
  for (int m = 0; m < members; ++m) sd.v[m] = seeds[m];
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_prio_draw, dim3((unsigned)(((int64_t)batch + 3) / 4), members), dim3(kPrioThreads), 0, s, t,
                     (int)batch, call, sd, idx, leaf_out);
  if (weights != nullptr || call < 0) {
    if (b.anneal > 0)
      hipLaunchKernelGGL(k_prio_finish<true>, dim3(1, members), dim3(kPrioMemberThreads), 0, s, t, (int)batch,
                         leaf_out, weights, b, call < 0 ? 1 : 0);
    else
      hipLaunchKernelGGL(k_prio_finish<false>, dim3(1, members), dim3(kPrioMemberThreads), 0, s, t, (int)batch,
                         leaf_out, weights, b, call < 0 ? 1 : 0);
  }
  const int rc = status();
  if (rc) return rc;
  return sacenv_replay_pop_gather(p, members, arena, batch, idx, st, action, reward, new_state, terminal, stream);
}

}  // namespace

extern "C" int sacenv_replay_prio_sample(const SacenvReplayParams* p, int32_t members, void* arena, void* state,
                                         int32_t batch, int64_t call, const uint64_t* seeds, int64_t* idx,
                                         uint32_t* leaf_out, float* weights, double beta, float* st, float* action,
                                         double* reward, float* new_state, uint8_t* terminal, void* stream) {
  const int rc = rb_pop_check(p, members);
  if (rc) return rc;
  if (batch < 0) return SACENV_E_SIZE;
  if (call < -1 || !finite_nonneg(beta)) return SACENV_E_RANGE;
  return prio_sample(p, members, arena, state, batch, call, seeds, idx, leaf_out, weights, PrioBeta{beta, beta, 0, call},
                     st, action, reward, new_state, terminal, stream);
}

// ---- include/sacenv_weighted_learn.h: the sample with its weights' exponent annealed
extern "C" int sacenv_replay_prio_sample_annealed(const SacenvReplayParams* p, int32_t members, void* arena,
                                                  void* state, int32_t batch, int64_t call, const uint64_t* seeds,
                                                  int64_t* idx, uint32_t* leaf_out, float* weights, double beta0,
                                                  double beta1, int64_t anneal_calls, float* st, float* action,
                                                  double* reward, float* new_state, uint8_t* terminal,
                                                  void* stream) {
  const int rc = rb_pop_check(p, members);
  if (rc) return rc;
  if (batch < 0) return SACENV_E_SIZE;
  if (call < -1 || !finite_nonneg(beta0) || !finite_nonneg(beta1) || anneal_calls < 1) return SACENV_E_RANGE;
  return prio_sample(p, members, arena, state, batch, call, seeds, idx, leaf_out, weights,
                     PrioBeta{beta0, beta1, anneal_calls, call}, st, action, reward, new_state, terminal, stream);
}
