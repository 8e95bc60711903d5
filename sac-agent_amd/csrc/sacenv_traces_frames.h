// sacenv_traces_frames.h — the device code of the episode frames (include/sacenv_frames.h),
// included by sacenv_traces.hip, the unit that owns the member buffers these kernels read. The
// rules of the picture are in the public header; what is here is how they are laid on the GPU.
//
// Three launches per render call, all reading `rows` from the member's header on the device:
//   k_fr_points  everything that belongs to a row or to a column, once: thread i turns row i
//                into fixed point (X, Y, heading, strip rows packed: 16 B) and into its boat
//                (three vertices and their box: 48 B); thread c < W writes column c of the
//                strip (its row j(c) and the two bands between j(c - 1) and j(c): 16 B);
//                thread 0 the background's four numbers.
//   k_fr_cover   one workgroup per 16 x 16 panel pixels, one pixel per thread. The points go
//                through LDS, kFrChunk segments at a time; the chunk's bounding box comes out of
//                the same pass, and a chunk whose box, grown by rad, misses the tile is skipped
//                (every point of its segments lies in the box, so no pixel of the tile is within
//                rad of them: nothing changes). Inside a chunk a wave (four pixel rows of the
//                tile) skips a segment whose own box, grown by rad, misses those rows, on scalar
//                registers; only the others reach the products. A tile whose pixels are all
//                covered stops early: segments are taken in order, so the first hit is the
//                smallest j.
//   k_fr_compose one thread per four pixels of a frame row, one 32-bit store; a workgroup writes
//                1 KiB of one frame. The frame index comes from blockIdx alone, so the frame's
//                step and boat are wave-uniform; no frame loops over segments (first[pixel] <= t),
//                and no division is made per pixel (a thread's row and column and the water level
//                come from reciprocals the host made; the two divisions left, the frame of a
//                workgroup and the cursor's column, are the same in every lane).
// No atomics: the same rows give the same bytes.
#pragma once

#include <string.h>

#include "sacenv_frames.h"
#include "sacenv_wave_core.h"

namespace {

constexpr int kFrChunk = SACENV_FRAMES_CHUNK;
constexpr int kFrTile = 16;                     // k_fr_cover's tile is kFrTile x kFrTile pixels
constexpr int kFrThreads = kFrTile * kFrTile;
constexpr int kFrWaves = kFrThreads / kWave;
constexpr int kFrWaveRows = kFrTile / kFrWaves;  // pixel rows of the tile one wave owns
constexpr int kFrRowWords = SACENV_TRACE_ROW_BYTES / 4;
constexpr int32_t kFrNone = INT32_MAX;
static_assert(kFrChunk + 1 <= kFrThreads, "one thread stages one point of a chunk");
static_assert(kWave % kFrTile == 0 && kFrWaveRows * kFrWaves == kFrTile, "a wave owns whole pixel rows of the tile");

// the scratch: geom int32 x 4 (rc, rt, rb, cg) | points int4 [R + 1] | boats int4 [R + 1][3] |
// strip columns int4 [W] | first int32 [HP][W]
__host__ __device__ inline int64_t fr_points_off() { return 16; }
__host__ __device__ inline int64_t fr_boats_off(const int32_t R) { return 16 + 16 * ((int64_t)R + 1); }
__host__ __device__ inline int64_t fr_cols_off(const int32_t R) { return 16 + 64 * ((int64_t)R + 1); }
__host__ __device__ inline int64_t fr_map_off(const int32_t R, const int32_t W) { return fr_cols_off(R) + 16 * (int64_t)W; }

// what the kernels need of the descriptor
struct Fr {
  const char* member;   // the member's header
  char* scratch;
  uint8_t* out;
  int64_t first_frame;
  int32_t W, H, S, HP, R, rad, rad2, boat_len, boat_half, every, n_frames, blocks_per_frame;
  uint32_t inv_wq, inv_hp;   // ceil(2^32 / (W / 4)), ceil(2^32 / HP)
  float x0, y0, sx, sy, goal_line, track_width;
};

struct FrDir {
  int16_t v[256][2];
};

// n / d through m = ceil(2^32 / d): exact while n (m d - 2^32) < 2^32, so for n < 2^32 / d
__host__ __device__ inline uint32_t fr_inverse(const uint32_t d) { return (uint32_t)((((uint64_t)1 << 32) + d - 1) / d); }

__device__ __forceinline__ float fr_clamp(const float v, const float lo, const float hi) {
  return !(v >= lo) ? lo : (v > hi ? hi : v);   // a NaN becomes lo
}

// coordinates lie in [-1024, 16 * 1024 + 1024]: a difference of two is at most 18432 < 2^14.2
__device__ __forceinline__ int32_t fr_fx(const Fr& a, const float x) {
  return (int32_t)rintf(fr_clamp((x - a.x0) * a.sx, -1024.0f, (float)(16 * a.W + 1024)));
}
__device__ __forceinline__ int32_t fr_fy(const Fr& a, const float y) {
  return (int32_t)rintf(fr_clamp((a.y0 - y) * a.sy, -1024.0f, (float)(16 * a.HP + 1024)));
}
__device__ __forceinline__ int32_t fr_strip_row(const Fr& a, const float v) {
  const float top = (float)(a.S - 1);
  return (int32_t)rintf(fr_clamp((1.0f - v) * 0.5f * top, 0.0f, top));
}

__device__ __forceinline__ int32_t fr_rows(const Fr& a) {   // the header's rows, kept inside the buffer
  const int32_t rows = reinterpret_cast<const SacenvTraceHeader*>(a.member)->rows;
  return rows < 0 ? 0 : (rows > a.R + 1 ? a.R + 1 : rows);
}

__device__ __forceinline__ const float* fr_row(const Fr& a, const int32_t i) {
  return reinterpret_cast<const float*>(a.member + SACENV_TRACE_HEADER_BYTES) + (int64_t)i * kFrRowWords;
}

// the action's and the rudder's strip rows of row i, packed
__device__ __forceinline__ int32_t fr_strip_rows(const Fr& a, const float* __restrict__ row) {
  return fr_strip_row(a, row[SACENV_OBS_DIM]) | (fr_strip_row(a, row[9] * 2.0f - 1.0f) << 16);
}

__global__ __launch_bounds__(256) void k_fr_points(const Fr a, const FrDir dir) {
  const int32_t rows = fr_rows(a);
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    *reinterpret_cast<int4*>(a.scratch) = int4{fr_fy(a, 0.0f) >> 4, fr_fy(a, a.track_width) >> 4,
                                               fr_fy(a, -a.track_width) >> 4, fr_fx(a, a.goal_line) >> 4};
  }
  if (i < a.W && rows > 0) {   // column i of the strip: j(i), the action's band, the rudder's band
    const int32_t j = (i * (rows - 1)) / (a.W - 1), jp = (max(i - 1, 0) * (rows - 1)) / (a.W - 1);
    const int32_t cur = fr_strip_rows(a, fr_row(a, j)), prev = fr_strip_rows(a, fr_row(a, jp));
    const int32_t a0 = prev & 0xFFFF, a1 = cur & 0xFFFF, r0 = prev >> 16, r1 = cur >> 16;
    reinterpret_cast<int4*>(a.scratch + fr_cols_off(a.R))[i] =
        int4{j, min(a0, a1) | (max(a0, a1) << 16), min(r0, r1) | (max(r0, r1) << 16), 0};
  }
  if (i >= rows) return;
  const float* __restrict__ row = fr_row(a, i);
  const float x = row[0] * a.goal_line;
  const float y = row[3] * (2.0f * a.track_width) - a.track_width;
  const int32_t hd = (int32_t)rintf(fr_clamp(row[6] * 256.0f, -8388608.0f, 8388608.0f)) & 255;
  const int32_t X = fr_fx(a, x), Y = fr_fy(a, y);
  reinterpret_cast<int4*>(a.scratch + fr_points_off())[i] = int4{X, Y, hd, fr_strip_rows(a, row)};
  // the boat: |V - P| <= (1024 * 1024 + 1024 * 1024) >> 10 = 2048
  const int32_t ux = dir.v[hd][0], uy = dir.v[hd][1];
  const int32_t fx = ux, fy = -uy, sx = uy, sy = ux, L = a.boat_len, G = a.boat_len >> 1, B = a.boat_half;
  const int32_t x0 = X + ((L * fx) >> 10), y0 = Y + ((L * fy) >> 10);
  const int32_t x1 = X + ((-G * fx - B * sx) >> 10), y1 = Y + ((-G * fy - B * sy) >> 10);
  const int32_t x2 = X + ((-G * fx + B * sx) >> 10), y2 = Y + ((-G * fy + B * sy) >> 10);
  int4* __restrict__ boat = reinterpret_cast<int4*>(a.scratch + fr_boats_off(a.R)) + 3 * (int64_t)i;
  boat[0] = int4{x0, y0, x1, y1};
  boat[1] = int4{x2, y2, 0, 0};
  boat[2] = int4{min(x0, min(x1, x2)), max(x0, max(x1, x2)), min(y0, min(y1, y2)), max(y0, max(y1, y2))};
}

__global__ __launch_bounds__(kFrThreads) void k_fr_cover(const Fr a) {
  __shared__ int32_t px[kFrChunk + 1], py[kFrChunk + 1];
  __shared__ int32_t box[kFrWaves][4];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  const int32_t c = blockIdx.x * kFrTile + (t & (kFrTile - 1)), r = blockIdx.y * kFrTile + t / kFrTile;
  const bool inside = c < a.W && r < a.HP;
  const int32_t cx = 16 * c + 8, cy = 16 * r + 8;
  // the tile's pixel centres, and those of this wave's rows
  const int32_t tx0 = 16 * kFrTile * (int32_t)blockIdx.x + 8, tx1 = tx0 + 16 * (kFrTile - 1);
  const int32_t ty0 = 16 * kFrTile * (int32_t)blockIdx.y + 8, ty1 = ty0 + 16 * (kFrTile - 1);
  const int32_t wy0 = ty0 + 16 * kFrWaveRows * __builtin_amdgcn_readfirstlane(wv), wy1 = wy0 + 16 * (kFrWaveRows - 1);
  const int32_t nseg = fr_rows(a) - 1;
  const int4* __restrict__ pts = reinterpret_cast<const int4*>(a.scratch + fr_points_off());
  int32_t first = inside ? kFrNone : 0;   // (a pixel outside the frame has nothing to look for)
  for (int32_t c0 = 0; c0 < nseg; c0 += kFrChunk) {
    // (also: the chunk before has been read by everybody)
    if (__syncthreads_and(first != kFrNone)) break;
    const int32_t n = min(kFrChunk, nseg - c0);   // segments c0 + 1 .. c0 + n, points c0 .. c0 + n
    int32_t x0 = INT32_MAX, x1 = INT32_MIN, y0 = INT32_MAX, y1 = INT32_MIN;
    if (t <= n) {
      const int4 p = pts[c0 + t];
      px[t] = p.x;
      py[t] = p.y;
      x0 = x1 = p.x;
      y0 = y1 = p.y;
    }
    if (wv * kWave <= n) {   // (waves that staged something)
#pragma unroll
      for (int o = kWave / 2; o > 0; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o));
        x1 = max(x1, __shfl_xor(x1, o));
        y0 = min(y0, __shfl_xor(y0, o));
        y1 = max(y1, __shfl_xor(y1, o));
      }
    }
    if (lane == 0) {
      box[wv][0] = x0;
      box[wv][1] = x1;
      box[wv][2] = y0;
      box[wv][3] = y1;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kFrWaves; ++w) {
      x0 = min(x0, box[w][0]);
      x1 = max(x1, box[w][1]);
      y0 = min(y0, box[w][2]);
      y1 = max(y1, box[w][3]);
    }
    if (x0 - a.rad > tx1 || x1 + a.rad < tx0 || y0 - a.rad > ty1 || y1 + a.rad < ty0) continue;   // (uniform)
    if (first != kFrNone) continue;
    for (int32_t k = 0; k < n; ++k) {
      // the segment's ends are the same in every lane: on scalar registers, and its box against
      // the wave's rows there too
      const int32_t ax = __builtin_amdgcn_readfirstlane(px[k]), ay = __builtin_amdgcn_readfirstlane(py[k]);
      const int32_t bx = __builtin_amdgcn_readfirstlane(px[k + 1]), by = __builtin_amdgcn_readfirstlane(py[k + 1]);
      if (min(ax, bx) - a.rad > tx1 || max(ax, bx) + a.rad < tx0 || min(ay, by) - a.rad > wy1 ||
          max(ay, by) + a.rad < wy0)
        continue;
      const int32_t dx = bx - ax, dy = by - ay, qx = cx - ax, qy = cy - ay;
      // |dx|, |dy|, |qx|, |qy| <= 18432: the three products below are at most 2 * 18432^2 < 2^29.4
      const int32_t dot = qx * dx + qy * dy, dd = dx * dx + dy * dy;
      bool hit;
      if (dot <= 0) {
        hit = qx * qx + qy * qy <= a.rad2;
      } else if (dot >= dd) {
        const int32_t ex = qx - dx, ey = qy - dy;
        hit = ex * ex + ey * ey <= a.rad2;
      } else {
        const int64_t cr = qx * dy - qy * dx;                    // |cr| < 2^29.4, its square < 2^59
        hit = cr * cr <= (int64_t)a.rad2 * dd;                   // rad2 <= 2^16: below 2^46
      }
      if (hit) {
        first = c0 + k + 1;
        break;
      }
    }
  }
  if (inside) reinterpret_cast<int32_t*>(a.scratch + fr_map_off(a.R, a.W))[(int64_t)r * a.W + c] = first;
}

// E(A, B, C): every factor is below 2^15, a product below 2^27 (|V - P| <= 2048, so
// |V_i - V_j| <= 4096 and |C - V| <= 21504)
__device__ __forceinline__ int32_t fr_edge(const int32_t ax, const int32_t ay, const int32_t bx, const int32_t by,
                                           const int32_t cx, const int32_t cy) {
  return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

__global__ __launch_bounds__(256) void k_fr_compose(const Fr a) {
  const int32_t f = blockIdx.x / a.blocks_per_frame;                       // (uniform)
  const int32_t item = (blockIdx.x - f * a.blocks_per_frame) * 256 + threadIdx.x;
  const int32_t wq = a.W / 4;
  if (item >= a.H * wq) return;
  const int32_t r = (int32_t)__umulhi((uint32_t)item, a.inv_wq);           // item / wq: item < 2^18, wq <= 2^8
  const int32_t c = (item - r * wq) * 4;
  const int32_t rows = fr_rows(a);
  // the frame's step: s * every >= s, so past the end without the product
  const int64_t s = a.first_frame + f;
  const int32_t t = rows == 0 ? -1 : (s >= rows - 1 ? rows - 1 : (int32_t)min(s * a.every, (int64_t)rows - 1));
  uint32_t px[4];
  if (r < a.HP) {
    const int4 g = *reinterpret_cast<const int4*>(a.scratch);              // rc, rt, rb, cg
    const int32_t dist = r > g.x ? r - g.x : g.x - r;
    const int32_t level = min(SACENV_FRAMES_WATER - 1, (int32_t)__umulhi((uint32_t)dist * 64u, a.inv_hp));
    // (rc lies in [-64, HP + 64], so dist <= HP + 64 and dist * 64 * HP <= 69 120 * 1016 < 2^27: the reciprocal is exact)
    uint32_t base = r < g.y || r > g.z ? SACENV_FRAMES_OUTSIDE : (uint32_t)level;
    if (r == g.y || r == g.z) base = SACENV_FRAMES_BOUNDARY;
    const int4 first = reinterpret_cast<const int4*>(a.scratch + fr_map_off(a.R, a.W))[((int64_t)r * a.W + c) / 4];
    const int32_t fs[4] = {first.x, first.y, first.z, first.w};
    const int32_t cy = 16 * r + 8;
    int4 v01 = {}, v2 = {};
    bool near = false;
    if (t >= 0) {
      const int4* __restrict__ boat = reinterpret_cast<const int4*>(a.scratch + fr_boats_off(a.R)) + 3 * (int64_t)t;
      const int4 bb = boat[2];                                             // (the box only saves the edge functions)
      near = cy >= bb.z && cy <= bb.w && 16 * c + 56 >= bb.x && 16 * c + 8 <= bb.y;
      if (near) {
        v01 = boat[0];
        v2 = boat[1];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t v = c + k == g.w ? SACENV_FRAMES_GOAL : base;
      if (fs[k] <= t) v = SACENV_FRAMES_PATH;
      if (near) {
        const int32_t cx = 16 * (c + k) + 8;
        if (fr_edge(v01.x, v01.y, v2.x, v2.y, cx, cy) >= 0 && fr_edge(v2.x, v2.y, v01.z, v01.w, cx, cy) >= 0 &&
            fr_edge(v01.z, v01.w, v01.x, v01.y, cx, cy) >= 0)
          v = SACENV_FRAMES_BOAT;
      }
      px[k] = v;
    }
  } else {
    const int32_t q = r - a.HP;
    const uint32_t base = q == ((a.S - 1) >> 1) ? SACENV_FRAMES_ZERO : SACENV_FRAMES_STRIP;
    const int32_t last = rows - 1;                                         // (rows - 1 <= 2^20, W - 1 < 2^10)
    const int32_t cursor = t < 0 ? -1 : (last > 0 ? t * (a.W - 1) / last : 0);   // (uniform)
    const int4* __restrict__ cols = reinterpret_cast<const int4*>(a.scratch + fr_cols_off(a.R)) + c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t v = base;
      if (t >= 0) {
        const int4 col = cols[k];                                          // j(c), the action's band, the rudder's
        if (col.x <= t) {
          if (q >= (col.z & 0xFFFF) && q <= (col.z >> 16)) v = SACENV_FRAMES_RUDDER;
          if (q >= (col.y & 0xFFFF) && q <= (col.y >> 16)) v = SACENV_FRAMES_ACTION;
        }
        if (c + k == cursor) v = SACENV_FRAMES_CURSOR;
      }
      px[k] = v;
    }
  }
  uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(a.out + ((int64_t)f * a.H + r) * a.W + c);
  *out = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
}

}  // namespace
