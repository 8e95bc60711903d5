// sacenv_sac.hip — the SAC agent on gfx950.
//
// ContinuousAgent.choose_action (agent/continuous_agent.py:57-61) for N
// observations at once, and ContinuousAgent.learn (:96-154) over the five
// networks of networks/networks.py:14-133, as fp32 MFMA kernels
// (v_mfma_f32_16x16x4_f32: f32 in, f32 accumulate, an fmaf chain per output).
//
// learn() in four launches. Every gradient of one learn() is taken at the
// parameters the call starts with: the value step (:121-125) changes only the
// value net, which neither the actor loss nor the critic loss reads; the
// critics step after the actor loss (:127-137 vs :139-150); the value-phase
// gradients that reach actor and critics are zeroed before their own losses
// (:133, :139-140). So the four losses are independent and the kernels run
// them side by side:
//
//   phase 0 (row blocks x 4 roles): actor forward + both policy draws, value
//     forward, critic 1 / 2 forward on the stored actions.
//   phase 1 (x 6): critic c at the rsample() actions with dq/da (actor loss);
//     critic c's own loss backward (target forward for value_, done-masked;
//     q_hat = scale * reward + gamma * value_); critic c at the sample()
//     actions (value target).
//   phase 2 (x 4): actor backward (min of the critics, tanh-squashed Normal
//     log-prob), value backward (value_target = min q - log_prob), each layer
//     split over two workgroups by output features.
//   phase 3: weight gradients as batch reductions (dW = dZ^T H on MFMA), Adam
//     (torch.optim.Adam, foreach form) on the four optimised nets, the target
//     soft update (:63-77), the transposes, and the four losses.
//
// Row blocks are 16 batch rows per 256-thread workgroup. A dense layer of a
// row block is Y^T = W X^T: wave w owns output features [64w, 64w + 64) as
// four 16x16 tiles; the weights are the MFMA A operand straight from L2
// (float4 per lane), the activations the B operand from LDS ([row][feature],
// 4-float pad). k runs in blocks of 16 with lane (i, kq) supplying
// k = 16 kb + 4 kq + s in step s — the same permutation on both operands, so
// each lane reads one float4 of each per block. Activations that phase 3
// reduces over the batch are stored feature-major [256][B].
//
// The device bodies and the host helpers are in sacenv_sac_core.h, which the
// population unit (sacenv_sac_pop.hip) includes too; this file holds the
// one-agent kernels and the entry points of include/sacenv.h.
#include "sacenv_sac_core.h"

#include "sacenv_weighted_learn.h"   // (sacenv_sac_learn_weighted: the learn with a weight per row)

namespace {

// one or two workgroups per CU: registers for kPrefetch k-blocks of weights in flight
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(1, 2))) k_sac_rows(SacArgs a, int phase) {
  __shared__ RowLds l;
  STAMP(a, phase, 0);
  rows_body(a, l, phase, blockIdx.x);
  STAMP(a, phase, 15);
}

__global__ void __launch_bounds__(kThreads) k_sac_update(SacArgs a) {
  __shared__ float sm[kUpdLds];
  STAMP(a, 3, 0);
  update_body(a, sm, blockIdx.x);
  STAMP(a, 3, 15);
}

// kernel copies of fc2.weight: fragment order for nets 0..4, transposed for 0..3
__global__ void __launch_bounds__(kThreads) k_sac_sync(SacArgs a) {
  const int t = blockIdx.y;
  const float* w2 = a.P + a.net[t] + a.off[net_shape(t)].t[2];
  for (int e = blockIdx.x * kThreads + threadIdx.x; e < kH * kH; e += gridDim.x * kThreads) {
    const int n = e >> 8, k = e & (kH - 1);
    const float v = w2[e];
    a.P[a.w2f[t] + swz(n, k)] = v;
    if (t < 4) a.P[a.w2tf[t] + swz(k, n)] = v;
  }
}

}  // namespace

extern "C" int sacenv_sac_layout(const SacenvSacParams* p, SacenvSacLayout* out) {
  if (p == nullptr || out == nullptr) return SACENV_E_NULL;
  const int rc = check(p);
  if (rc != SACENV_OK) return rc;
  make_layout(p, out);
  return SACENV_OK;
}

extern "C" int sacenv_sac_sync(const SacenvSacParams* p, float* weights, void* stream) {
  const int rc = check(p);
  if (rc != SACENV_OK) return rc;
  if (weights == nullptr) return SACENV_E_NULL;
  if (!aligned16(weights)) return SACENV_E_SIZE;
  const SacArgs a = make_args(p, weights);
  hipLaunchKernelGGL(k_sac_sync, dim3(64, 5), dim3(kThreads), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

__global__ void __launch_bounds__(kThreads) k_sac_act(SacArgs a, const float* __restrict__ obs, int n,
                                                        const float* __restrict__ eps, float* __restrict__ out,
                                                        float* __restrict__ logp, ActHandoff h) {
  __shared__ ActLds l;
  act_body(l, a, obs, n, eps, out, logp, h);
}

// The closed loop's form (sacenv_sac_act_handoff): the same code held to 128
// architectural VGPRs (~150 allocated, no spills) so that one policy wave fits
// beside an owner wave of the segment launch (~320 VGPRs) on a SIMD's 512,
// and launched with its LDS padded to kHandoffLds (> half of a CU's 160 KB):
// a CU then holds at most ONE policy workgroup, which always leaves room for
// the CU's owner waves -- no arrangement of dispatched policy workgroups can
// keep an owner wave out (sacenv.closed_loop's co-residency plan).
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_num_vgpr(128)))
k_sac_act_lean(SacArgs a, const float* __restrict__ obs, int n, const float* __restrict__ eps,
               float* __restrict__ out, float* __restrict__ logp, ActHandoff h) {
  __shared__ ActLds l;
  act_body(l, a, obs, n, eps, out, logp, h);
}

static int sac_act(const SacenvSacParams* p, const float* weights, const float* obs, int32_t n, const float* eps,
                   float* action, float* log_prob, const ActHandoff& h, void* stream) {
  if (p == nullptr) return SACENV_E_NULL;
  if (p->hidden != kH || p->n_actions != 1 || p->obs_dim < 1 || p->obs_dim > 14) return SACENV_E_SIZE;
  if (n < 0) return SACENV_E_SIZE;
  if (n == 0) return SACENV_OK;
  if (weights == nullptr || obs == nullptr || eps == nullptr || action == nullptr) return SACENV_E_NULL;
  if (!aligned16(weights)) return SACENV_E_SIZE;
  SacenvSacParams q = *p;
  q.batch = 256;  // unused by the act kernel
  const SacArgs a = make_args(&q, const_cast<float*>(weights));
  const int blocks = (n + kActRows - 1) / kActRows;
  if (h.obs_ready != nullptr)  // LDS padded: at most one policy workgroup per CU (kHandoffLds)
    hipLaunchKernelGGL(k_sac_act_lean, dim3(blocks), dim3(kThreads), kHandoffLds - sizeof(ActLds),
                       (hipStream_t)stream, a, obs, (int)n, eps, action, log_prob, h);
  else
    hipLaunchKernelGGL(k_sac_act, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, a, obs, (int)n, eps, action,
                       log_prob, h);
  return (int)hipGetLastError();
}

extern "C" int sacenv_sac_act(const SacenvSacParams* p, const float* weights, const float* obs, int32_t n,
                              const float* eps, float* action, float* log_prob, void* stream) {
  return sac_act(p, weights, obs, n, eps, action, log_prob, ActHandoff{}, stream);
}

// The hand-off act kernel's resources for the closed loop's co-residency plan
// (sacenv.h): resident workgroups per CU alone, the grid for n rows, VGPRs per
// lane (architectural + accumulation, as allocated) and LDS bytes per workgroup.
extern "C" int sacenv_sac_act_occupancy(int32_t n, int32_t* blocks_per_cu, int32_t* grid, int32_t* vgprs,
                                        int32_t* lds_bytes) {
  if (blocks_per_cu == nullptr || grid == nullptr || vgprs == nullptr || lds_bytes == nullptr) return SACENV_E_NULL;
  if (n < 0) return SACENV_E_SIZE;
  int nb = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_sac_act_lean, kThreads,
                                                               kHandoffLds - sizeof(ActLds));
  if (e != hipSuccess) return (int)e;
  hipFuncAttributes fa{};
  e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k_sac_act_lean));
  if (e != hipSuccess) return (int)e;
  *blocks_per_cu = nb;
  *grid = (n + kActRows - 1) / kActRows;
  *vgprs = fa.numRegs;
  *lds_bytes = kHandoffLds;  // static + the padding at launch
  return SACENV_OK;
}

extern "C" int sacenv_sac_act_handoff(const SacenvSacParams* p, const float* weights, const float* obs,
                                      int32_t n, const float* eps, float* action, const uint32_t* obs_ready,
                                      uint32_t obs_want, uint32_t* act_ready, uint32_t act_value,
                                      int32_t* status, void* stream) {
  if (obs_ready == nullptr || act_ready == nullptr) return SACENV_E_NULL;
  if (obs_want >= 0x80000000u || act_value >= 0x80000000u) return SACENV_E_RANGE;
  return sac_act(p, weights, obs, n, eps, action, nullptr, ActHandoff{obs_ready, obs_want, act_ready, act_value, status},
                 stream);
}

// include/sacenv_weighted_learn.h: row_weights [batch] or null (sacenv_sac_learn: null)
extern "C" int sacenv_sac_learn_weighted(const SacenvSacParams* p, float* weights, void* scratch, const float* state,
                                         const float* action, const double* reward, const float* new_state,
                                         const uint8_t* done, const float* eps1, const float* eps2,
                                         int32_t adam_step, float* losses, const float* row_weights, void* stream) {
  const int rc = check(p);
  if (rc != SACENV_OK) return rc;
  if (weights == nullptr || scratch == nullptr || state == nullptr || action == nullptr || reward == nullptr ||
      new_state == nullptr || done == nullptr || eps1 == nullptr || eps2 == nullptr)
    return SACENV_E_NULL;
  if (adam_step < 1) return SACENV_E_RANGE;
  if (!aligned16(weights) || !aligned16(scratch)) return SACENV_E_SIZE;
  SacArgs a = make_args(p, weights);
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
  set_member(a, member_scalars(p->lr_actor, p->lr_critic, p->gamma, p->tau, p->reward_scale, bc1));
  const int nrb = p->batch / kRows;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sac_rows, dim3(4 * nrb), dim3(kThreads), 0, s, a, 0);
  hipLaunchKernelGGL(k_sac_rows, dim3(6 * nrb), dim3(kThreads), 0, s, a, 1);
  hipLaunchKernelGGL(k_sac_rows, dim3(4 * nrb), dim3(kThreads), 0, s, a, 2);
  hipLaunchKernelGGL(k_sac_update, dim3(kUpdateBlocks), dim3(kThreads), 0, s, a);
  return (int)hipGetLastError();
}

extern "C" int sacenv_sac_learn(const SacenvSacParams* p, float* weights, void* scratch, const float* state,
                                const float* action, const double* reward, const float* new_state,
                                const uint8_t* done, const float* eps1, const float* eps2, int32_t adam_step,
                                float* losses, void* stream) {
  return sacenv_sac_learn_weighted(p, weights, scratch, state, action, reward, new_state, done, eps1, eps2, adam_step,
                                   losses, nullptr, stream);
}
