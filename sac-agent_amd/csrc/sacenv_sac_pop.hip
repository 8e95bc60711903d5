// sacenv_sac_pop.hip — a population of SAC agents in one set of launches
// (include/sacenv_population.h; the reference's hyper-parameter search, main.py -p N).
//
// P agents: the kernels of sacenv_sac.hip with a second grid dimension over the
// members. Member m = blockIdx.y runs rows_body / update_body / act_body,
// unchanged, on its own SacArgs: the launch's SacArgs (member 0's pointers, the
// shared layout and Adam scalars) with every pointer moved by m member strides
// and the six per-member scalars taken from a table in the kernel arguments.
//
// This is a translation unit of its own, which shares the device bodies and the
// host helpers with sacenv_sac.hip through sacenv_sac_core.h: compiled in one
// unit, a second caller of the bodies changes how the compiler schedules the
// one-agent kernels (tools/kernel_diff.py), and those stay as they are.
//
// rows_body and update_body index SacArgs' arrays by role and net, which are
// run-time values: a by-value copy of the member's SacArgs with such an index on
// it lives in private memory (688 B of scratch per lane). The act kernel indexes
// by constants only. The rows kernel calls rows_body once per (phase, role)
// under a test of both, which makes the role a constant inside each call -- given
// that everything below the body is inlined, hence the always_inline pushed over
// the include (one agent's kernels inline all of it too). The update kernel keeps
// the member's SacArgs in LDS. DESIGN.md §4.8 has the resource table.
#pragma clang attribute push(__attribute__((always_inline)), apply_to = function)
#include "sacenv_sac_core.h"
#pragma clang attribute pop

#include "sacenv_prioritized_replay.h"   // (its one accessor of the learn scratch lives here, at the end)
#include "sacenv_weighted_learn.h"       // (sacenv_sac_pop_learn_weighted: the learn with a weight per row)

namespace {

constexpr int kPopMax = SACENV_SAC_POP_MAX_MEMBERS;

struct PopArgs {
  int64_t w_stride;   // floats between two members' weights slabs
  int64_t s_stride;   // bytes between two members' scratch slabs (a multiple of 16)
  PopMember hp[kPopMax];
};
static_assert(sizeof(SacArgs) + sizeof(PopArgs) + 64 <= 4096, "the population kernels' arguments must stay under 4 KB");

template <typename T>
__device__ __forceinline__ T* shift_bytes(T* p, int64_t bytes) {
  return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + (uintptr_t)bytes);
}

// member m's arguments: the batch tensors are [P][B][..], the losses [P][4]
__device__ __forceinline__ SacArgs member_args(const SacArgs& a, const PopArgs& q, int m) {
  SacArgs am = a;
  const int64_t sb = (int64_t)m * q.s_stride, rows = (int64_t)m * a.B;
  am.P = a.P + (int64_t)m * q.w_stride;
  am.stamps = shift_bytes(a.stamps, sb);
  am.rows = shift_bytes(a.rows, sb);
  am.xt = shift_bytes(a.xt, sb);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    am.na[t].h1t = shift_bytes(a.na[t].h1t, sb);
    am.na[t].h2t = shift_bytes(a.na[t].h2t, sb);
    am.na[t].dz1t = shift_bytes(a.na[t].dz1t, sb);
    am.na[t].dz2t = shift_bytes(a.na[t].dz2t, sb);
  }
  if (a.losses != nullptr) am.losses = a.losses + 4 * (int64_t)m;
  if (a.s != nullptr) {  // null in the act launch: no batch there
    am.s = a.s + rows * a.D;
    am.s2 = a.s2 + rows * a.D;
    am.act = a.act + rows;
    am.rew = a.rew + rows;
    am.done = a.done + rows;
    am.eps1 = a.eps1 + rows;
    am.eps2 = a.eps2 + rows;
    if (a.isw != nullptr) am.isw = a.isw + rows;
  }
  const PopMember h = q.hp[m];
  am.gamma = h.gamma;
  am.scale = h.scale;
  am.tau = h.tau;
  am.omtau = h.omtau;
  am.nstep_actor = h.nstep_actor;
  am.nstep_critic = h.nstep_critic;
  return am;
}

template <int PH, int R>
__device__ __forceinline__ void rows_case(const SacArgs& am, RowLds& l, int phase, int role, int vb) {
  if (phase == PH && role == R) rows_body(am, l, phase, vb);
}

// grid (roles * B / 16, P); registers as k_sac_rows
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(1, 2)))
k_sac_rows_pop(SacArgs a, PopArgs q, int phase) {
  __shared__ RowLds l;
  const SacArgs am = member_args(a, q, blockIdx.y);
  const int vb = blockIdx.x, role = vb / (am.B / kRows);  // as rows_body takes them
  // one call per (phase, role): inside each, the role -- and with it every index
  // into SacArgs' arrays -- is a constant, so the copy stays in registers
  rows_case<0, 0>(am, l, phase, role, vb);
  rows_case<0, 1>(am, l, phase, role, vb);
  rows_case<0, 2>(am, l, phase, role, vb);
  rows_case<0, 3>(am, l, phase, role, vb);
  rows_case<1, 0>(am, l, phase, role, vb);
  rows_case<1, 1>(am, l, phase, role, vb);
  rows_case<1, 2>(am, l, phase, role, vb);
  rows_case<1, 3>(am, l, phase, role, vb);
  rows_case<1, 4>(am, l, phase, role, vb);
  rows_case<1, 5>(am, l, phase, role, vb);
  rows_case<2, 0>(am, l, phase, role, vb);
  rows_case<2, 1>(am, l, phase, role, vb);
  rows_case<2, 2>(am, l, phase, role, vb);
  rows_case<2, 3>(am, l, phase, role, vb);
}

// update_body places its fc2 tiles by b & 7 (workgroups go to the XCDs round-robin
// in launch order, x fastest): grid.x is kUpdateBlocks rounded up to a multiple of
// 8, so that every member's block b lands on XCD b % 8 as in the one-agent launch
constexpr int kUpdateBlocksPop =
#ifdef SACENV_POP_PLAIN_GRID
    kUpdateBlocks;  // the measured alternative: member m's blocks shifted by m XCDs
#else
    (kUpdateBlocks + 7) & ~7;
#endif

__global__ void __launch_bounds__(kThreads) k_sac_update_pop(SacArgs a, PopArgs q) {
  __shared__ float sm[kUpdLds];
  if (blockIdx.x >= kUpdateBlocks) return;  // the padding
  // update_body indexes SacArgs' arrays by the block's net, a run-time value: a
  // by-value copy would live in private memory (688 B of scratch per lane), so
  // thread 0 writes the member's arguments to LDS (one wave per SIMD here:
  // registers to spare for the pointers that are SGPRs in k_sac_update)
  __shared__ SacArgs am;
  if (threadIdx.x == 0) am = member_args(a, q, blockIdx.y);
  __syncthreads();
  update_body(am, sm, blockIdx.x);
}

// grid (ceil(n / 64), P): member m's n rows of obs / eps / out / logp
__global__ void __launch_bounds__(kThreads) k_sac_act_pop(SacArgs a, PopArgs q, const float* __restrict__ obs, int n,
                                                            const float* __restrict__ eps, float* __restrict__ out,
                                                            float* __restrict__ logp) {
  __shared__ ActLds l;
  const int m = blockIdx.y;
  const SacArgs am = member_args(a, q, m);
  const int64_t r = (int64_t)m * n;
  act_body(l, am, obs + r * a.D, n, eps + r, out + r, logp != nullptr ? logp + r : nullptr, ActHandoff{});
}

int pop_check(const SacenvSacParams* p, int32_t members, bool act) {
  if (p == nullptr) return SACENV_E_NULL;
  SacenvSacParams c = *p;
  if (act) c.batch = 256;  // unused by the act kernel, as in sacenv_sac_act
  const int rc = check(&c);
  if (rc != SACENV_OK) return rc;
  if (members < 1 || members > kPopMax) return SACENV_E_SIZE;
  return SACENV_OK;
}

void make_pop_layout(const SacenvSacParams* p, int32_t members, SacenvSacPopLayout* out) {
  SacenvSacLayout L;
  make_layout(p, &L);
  out->member_floats = (L.total_floats + 3) & ~int64_t(3);
  out->scratch_bytes = (L.scratch_bytes + 15) & ~int64_t(15);
  out->total_floats = members * out->member_floats;
  out->total_scratch_bytes = members * out->scratch_bytes;
  out->max_members = kPopMax;
  out->pad = 0;
}

}  // namespace

extern "C" int sacenv_sac_pop_layout(const SacenvSacParams* p, int32_t members, SacenvSacPopLayout* out) {
  if (p == nullptr || out == nullptr) return SACENV_E_NULL;
  const int rc = pop_check(p, members, false);
  if (rc != SACENV_OK) return rc;
  make_pop_layout(p, members, out);
  return SACENV_OK;
}

extern "C" int sacenv_sac_pop_sync(const SacenvSacParams* p, int32_t members, float* weights, void* stream) {
  const int rc = pop_check(p, members, false);
  if (rc != SACENV_OK) return rc;
  if (weights == nullptr) return SACENV_E_NULL;
  if (!aligned16(weights)) return SACENV_E_SIZE;
  SacenvSacPopLayout L;
  make_pop_layout(p, members, &L);
  for (int m = 0; m < members; ++m) {  // not on the hot path: one launch per member
    const int rs = sacenv_sac_sync(p, weights + m * L.member_floats, stream);
    if (rs != SACENV_OK) return rs;
  }
  return SACENV_OK;
}

extern "C" int sacenv_sac_pop_act(const SacenvSacParams* p, int32_t members, const float* weights, const float* obs,
                                  int32_t n, const float* eps, float* action, float* log_prob, void* stream) {
  const int rc = pop_check(p, members, true);
  if (rc != SACENV_OK) return rc;
  if (n < 0) return SACENV_E_SIZE;
  if (n == 0) return SACENV_OK;
  if (weights == nullptr || obs == nullptr || eps == nullptr || action == nullptr) return SACENV_E_NULL;
  if (!aligned16(weights)) return SACENV_E_SIZE;
  SacenvSacParams c = *p;
  c.batch = 256;
  SacenvSacPopLayout L;
  make_pop_layout(&c, members, &L);
  const SacArgs a = make_args(&c, const_cast<float*>(weights));
  PopArgs q{};
  q.w_stride = L.member_floats;
  const int blocks = (n + kActRows - 1) / kActRows;
  hipLaunchKernelGGL(k_sac_act_pop, dim3(blocks, members), dim3(kThreads), 0, (hipStream_t)stream, a, q, obs, (int)n,
                     eps, action, log_prob);
  return (int)hipGetLastError();
}

// include/sacenv_weighted_learn.h: row_weights [members][batch] or null (sacenv_sac_pop_learn: null)
extern "C" int sacenv_sac_pop_learn_weighted(const SacenvSacParams* p, int32_t members, const SacenvSacMember* hp,
                                             float* weights, void* scratch, const float* state,
                                             const float* action, const double* reward, const float* new_state,
                                             const uint8_t* done, const float* eps1, const float* eps2,
                                             int32_t adam_step, float* losses, const float* row_weights,
                                             void* stream) {
  const int rc = pop_check(p, members, false);
  if (rc != SACENV_OK) return rc;
  if (hp == nullptr || weights == nullptr || scratch == nullptr || state == nullptr || action == nullptr ||
      reward == nullptr || new_state == nullptr || done == nullptr || eps1 == nullptr || eps2 == nullptr)
    return SACENV_E_NULL;
  if (adam_step < 1) return SACENV_E_RANGE;
  if (!aligned16(weights) || !aligned16(scratch)) return SACENV_E_SIZE;
  if (members == 1) {
    // One member is one agent: its launches are the one-agent kernels. The population
    // kernels cost ~5 us more per learn() (the member's arguments in LDS
    // in the update launch, one code path per critic in the row launches), which P >= 2
    // repays many times over and P = 1 would only pay.
    SacenvSacParams one = *p;
    one.lr_actor = hp[0].lr_actor;
    one.lr_critic = hp[0].lr_critic;
    one.gamma = hp[0].gamma;
    one.tau = hp[0].tau;
    one.reward_scale = hp[0].reward_scale;
    return sacenv_sac_learn_weighted(&one, weights, scratch, state, action, reward, new_state, done, eps1, eps2,
                                     adam_step, losses, row_weights, stream);
  }
  SacenvSacPopLayout L;
  make_pop_layout(p, members, &L);
  SacArgs a = make_args(p, weights);  // member 0's pointers; the kernels move them by the strides
  a.s = state;
  a.act = action;
  a.rew = reward;
  a.s2 = new_state;
  a.done = done;
  a.eps1 = eps1;
  a.eps2 = eps2;
  a.losses = losses;
  a.isw = row_weights;
  const double bc1 = set_learn_common(a, p, scratch, adam_step);
  PopArgs q{};
  q.w_stride = L.member_floats;
  q.s_stride = L.scratch_bytes;
  for (int m = 0; m < members; ++m)
    q.hp[m] = member_scalars(hp[m].lr_actor, hp[m].lr_critic, hp[m].gamma, hp[m].tau, hp[m].reward_scale, bc1);
  set_member(a, q.hp[0]);
  const int nrb = p->batch / kRows;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sac_rows_pop, dim3(4 * nrb, members), dim3(kThreads), 0, s, a, q, 0);
  hipLaunchKernelGGL(k_sac_rows_pop, dim3(6 * nrb, members), dim3(kThreads), 0, s, a, q, 1);
  hipLaunchKernelGGL(k_sac_rows_pop, dim3(4 * nrb, members), dim3(kThreads), 0, s, a, q, 2);
  hipLaunchKernelGGL(k_sac_update_pop, dim3(kUpdateBlocksPop, members), dim3(kThreads), 0, s, a, q);
  return (int)hipGetLastError();
}

extern "C" int sacenv_sac_pop_learn(const SacenvSacParams* p, int32_t members, const SacenvSacMember* hp,
                                    float* weights, void* scratch, const float* state, const float* action,
                                    const double* reward, const float* new_state, const uint8_t* done,
                                    const float* eps1, const float* eps2, int32_t adam_step, float* losses,
                                    void* stream) {
  return sacenv_sac_pop_learn_weighted(p, members, hp, weights, scratch, state, action, reward, new_state, done, eps1,
                                       eps2, adam_step, losses, nullptr, stream);
}

// ---- include/sacenv_prioritized_replay.h: where role_critic_loss leaves (q - q_hat)^2 per batch
// row (F_LC1, F_LC2 of the one RowField enum), as float offsets into one member's learn scratch
extern "C" int sacenv_replay_prio_learn_rows(const SacenvSacParams* sp, int64_t* td_sq1_off, int64_t* td_sq2_off) {
  const int rc = check(sp);
  if (rc != SACENV_OK) return rc;
  if (td_sq1_off == nullptr || td_sq2_off == nullptr) return SACENV_E_NULL;
  const int64_t rows = learn_rows_offset(sp);
  *td_sq1_off = rows + (int64_t)F_LC1 * sp->batch;  // rowf()
  *td_sq2_off = rows + (int64_t)F_LC2 * sp->batch;
  return SACENV_OK;
}
