// sacenv_wave_core.h — what the episode log (sacenv_episodes.hip), the scoreboard
// (sacenv_board.hip), population selection (sacenv_select.hip) and the episode traces
// (sacenv_traces.hip) share: the wave's width, a
// lane's rank in a ballot, the 16-B store, the slab copy with its grid, and the launches'
// outcome (that one the replay units take too). No kernel and no entry point lives here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sacenv.h"

namespace {

constexpr int kWave = 64;
constexpr int kSlabLoads = 4;   // 16-B loads a lane of slab_copy has in flight

inline int status() {   // what the launches of an entry point left behind
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? SACENV_OK : (int)err;
}

// the set lanes of `mask` below this one
__device__ __forceinline__ uint32_t ballot_rank(const uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ __forceinline__ void store16(void* p, uint64_t a, uint64_t b) { *reinterpret_cast<ulong2*>(p) = ulong2{a, b}; }
__device__ __forceinline__ uint64_t pack32(int32_t lo, int32_t hi) { return (uint32_t)lo | ((uint64_t)(uint32_t)hi << 32); }

// Workgroup blockIdx.x of gridDim.x, kThreads lanes each, copies its share of `vecs` 16-B
// vectors: kSlabLoads loads in flight per lane, then the rest one by one. (Named values: in
// k_select_copy an array of them was put into LDS.)
template <int kThreads>
__device__ __forceinline__ void slab_copy(const float4* __restrict__ src, float4* __restrict__ dst,
                                          const int64_t vecs) {
  static_assert(kSlabLoads == 4, "four loads in flight per lane, written out");
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  for (; i + 3 * stride < vecs; i += 4 * stride) {
    const float4 v0 = src[i], v1 = src[i + stride], v2 = src[i + 2 * stride], v3 = src[i + 3 * stride];
    dst[i] = v0;
    dst[i + stride] = v1;
    dst[i + 2 * stride] = v2;
    dst[i + 3 * stride] = v3;
  }
  for (; i < vecs; i += stride) dst[i] = src[i];
}

// slab_copy's grid.x: one workgroup per threads x kSlabLoads vectors, at most `cap`
inline int64_t slab_chunks(const int64_t vecs, const int threads, const int cap) {
  const int64_t per = (int64_t)threads * kSlabLoads, chunks = (vecs + per - 1) / per;
  return chunks > cap ? cap : chunks;
}

}  // namespace
