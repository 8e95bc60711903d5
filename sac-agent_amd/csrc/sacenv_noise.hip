// sacenv_noise.hip — counter-based policy noise (include/sacenv_noise.h): the standard
// normal draws of choose_action and learn, for every member of a population and for up
// to four draws, in one launch.
//
// A thread owns one Philox4x64-10 block (sacenv_philox.h): counter (j, call, stream, 0)
// under key (member's seed, SACENV_NOISE_KEY1) gives four 64-bit words, two Box-Muller
// pairs, elements 4j .. 4j + 3 of the member's row of that call. Everything is f64 until
// the last rounding, with sincospi's exact argument reduction (the header has the
// contract; tests/noise_oracle.py restates it).
//
// Launch shape: grid (W, members) x 64 threads. blockIdx.y is the member, so its seed is
// one scalar load from the kernel arguments at an SGPR offset (as PopArgs in
// sacenv_sac_pop.hip and the seeds of sacenv_replay_pop.hip are read); blockIdx.x runs
// over the draws' workgroups one draw after the other (draw d owns [first[d], first[d+1])),
// so the descriptor a workgroup works on is chosen by scalar compares, with no table
// indexed by a run-time value. Within a draw a member's calls x ceil(n / 4) blocks are
// numbered call-major and dealt 64 to a workgroup: short rows (a learn's 256 values are 64
// blocks, one wave) waste no lanes, and the grid stays small whatever calls and n are.
// Nothing is read from memory and nothing is kept on the device between calls.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sacenv_noise.h"
#include "sacenv_philox.h"

namespace {

constexpr int kNoiseThreads = 64;
constexpr int kNoiseMaxMembers = SACENV_NOISE_MAX_MEMBERS;
constexpr int kNoiseMaxDraws = SACENV_NOISE_MAX_STREAMS;

struct NoiseSeeds {
  uint64_t v[kNoiseMaxMembers];
};

struct NoiseDrawArgs {
  uint64_t stream, first_call;
  float* out;
  uint32_t n, bpr;      // values and Philox blocks (ceil(n / 4)) of one row
  uint32_t blocks;      // calls x bpr: one member's Philox blocks of this draw
  uint32_t first;       // the draw's first blockIdx.x
};

struct NoiseArgs {
  NoiseDrawArgs d[kNoiseMaxDraws];   // unused slots: blocks == 0, first == the grid's width
  int32_t members;
};
static_assert(sizeof(NoiseSeeds) + sizeof(NoiseArgs) <= 1024, "the noise kernel's arguments stay small");

// one Box-Muller pair from two words: (r cospi(2 u2), r sinpi(2 u2)), u1 in (0, 1], u2 in [0, 1)
__device__ __forceinline__ void normal_pair(uint64_t wa, uint64_t wb, float* z0, float* z1) {
  constexpr double k2m53 = 1.0 / 9007199254740992.0;
  const double u1 = (double)((wa >> 11) + 1ull) * k2m53;
  const double u2 = (double)(wb >> 11) * k2m53;
  const double r = sqrt(-2.0 * log(u1));
  double s, c;
  sincospi(2.0 * u2, &s, &c);
  *z0 = (float)(r * c);
  *z1 = (float)(r * s);
}

__global__ void __launch_bounds__(kNoiseThreads) k_noise_normal(NoiseSeeds seeds, NoiseArgs a) {
  const uint32_t bx = blockIdx.x, m = blockIdx.y;
  // the draw of this workgroup: the last whose first workgroup is <= bx (uniform: SGPR selects)
  NoiseDrawArgs d = a.d[0];
#pragma unroll
  for (int k = 1; k < kNoiseMaxDraws; ++k)
    if (bx >= a.d[k].first) d = a.d[k];
  const uint32_t t = (bx - d.first) * kNoiseThreads + threadIdx.x;   // < 2^31: blocks <= calls x n
  if (t >= d.blocks) return;
  const uint32_t call = t / d.bpr, j = t - call * d.bpr;
  uint64_t c[4] = {(uint64_t)j, d.first_call + (uint64_t)call, d.stream, 0ull};
  philox4x64_10(c, seeds.v[m], SACENV_NOISE_KEY1);
  float z[4];
  normal_pair(c[0], c[1], &z[0], &z[1]);
  normal_pair(c[2], c[3], &z[2], &z[3]);
  // row (call, m) of out [calls][members][n]; calls x members x n < 2^31 (checked on the host)
  const uint32_t i0 = 4u * j;
  float* const o = d.out + ((int64_t)call * a.members + m) * d.n + i0;
  const uint32_t left = d.n - i0;   // >= 1
  if (left >= 4u && (reinterpret_cast<uintptr_t>(o) & 15u) == 0u) {
    *reinterpret_cast<float4*>(o) = make_float4(z[0], z[1], z[2], z[3]);
    return;
  }
  o[0] = z[0];
  if (left > 1u) o[1] = z[1];
  if (left > 2u) o[2] = z[2];
  if (left > 3u) o[3] = z[3];
}

}  // namespace

extern "C" int sacenv_noise_normal(int32_t members, const uint64_t* seeds, int32_t n_draws,
                                   const SacenvNoiseDraw* draws, void* stream) {
  if (members < 1 || members > kNoiseMaxMembers || n_draws < 1 || n_draws > kNoiseMaxDraws) return SACENV_E_SIZE;
  if (seeds == nullptr || draws == nullptr) return SACENV_E_NULL;
  NoiseArgs a{};
  a.members = members;
  uint64_t width = 0;   // workgroups along x: < 4 x (2^31 / 64 + 1)
  for (int k = 0; k < n_draws; ++k) {
    const SacenvNoiseDraw& q = draws[k];
    if (q.calls < 1 || q.n < 0) return SACENV_E_SIZE;
    if ((int64_t)q.calls * members * q.n >= (1LL << 31)) return SACENV_E_SIZE;
    NoiseDrawArgs& d = a.d[k];
    d.first = (uint32_t)width;
    if (q.n == 0) continue;   // (blocks == 0: no workgroup is the draw's)
    if (q.out == nullptr) return SACENV_E_NULL;
    if ((reinterpret_cast<uintptr_t>(q.out) & 3u) != 0u) return SACENV_E_SIZE;
    d.stream = q.stream;
    d.first_call = q.first_call;
    d.out = q.out;
    d.n = (uint32_t)q.n;
    d.bpr = (d.n + 3u) / 4u;
    d.blocks = (uint32_t)q.calls * d.bpr;   // <= calls x n < 2^31
    width += (d.blocks + kNoiseThreads - 1) / kNoiseThreads;
  }
  for (int k = n_draws; k < kNoiseMaxDraws; ++k) a.d[k].first = (uint32_t)width;
  if (width == 0) return SACENV_OK;
  NoiseSeeds s{};
  for (int m = 0; m < members; ++m) s.v[m] = seeds[m];
  hipLaunchKernelGGL(k_noise_normal, dim3((unsigned)width, (unsigned)members), dim3(kNoiseThreads), 0,
                     (hipStream_t)stream, s, a);
  return (int)hipGetLastError();
}
