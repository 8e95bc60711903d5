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
// This is a translation unit of its own, which shares the device bodies and the host
// rules with sacenv_replay.hip through sacenv_replay_core.h: the one-buffer kernels, and
// above all the staged, side and stand-in kernels of the timed replay path, are compiled
// where they were, alone (tools/kernel_diff.py; DESIGN.md §4.6.1 has the result and the
// resource table).
#include "sacenv_replay_core.h"

#include "sacenv_population_replay.h"

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
