// sacenv_philox.h — Philox4x64-10 (Salmon, Moraes, Dror, Shaw, "Parallel random numbers:
// as easy as 1, 2, 3", SC'11; numpy ships it as np.random.Philox), the one counter-based
// generator of the library. The staged replay's sampler (sacenv_replay.hip, key (seed, 0))
// and the policy noise (sacenv_noise.hip, key (seed, 0x6E6F697365)) take their words from
// it; oracle/ctr_sampler.py restates it and pins it word for word to numpy's.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ void philox4x64_10(uint64_t c[4], uint64_t k0, uint64_t k1) {
  constexpr uint64_t kM0 = 0xD2E7470EE14C6C93ull, kM1 = 0xCA5A826395121157ull;  // multipliers
  constexpr uint64_t kW0 = 0x9E3779B97F4A7C15ull, kW1 = 0xBB67AE8584CAA73Bull;  // Weyl key bumps
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t hi0 = __umul64hi(kM0, c[0]), lo0 = kM0 * c[0];
    const uint64_t hi1 = __umul64hi(kM1, c[2]), lo1 = kM1 * c[2];
    const uint64_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = lo1;
    c[2] = n2;
    c[3] = lo0;
    k0 += kW0;
    k1 += kW1;
  }
}

}  // namespace
