// sacenv_boat_draw.h — Boat(config) on the device: a drawing wave's LDS, the episode draw from the
// env's MT19937 stream (draw_knots_wave), its wave-wide fit (fit_store_wave: here, not with the wind
// code, because it works on DrawLds), the fresh state, and the twist of the next MT block (mt_ahead).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sacenv.h"
#include "sacenv_boat_arena.h"
#include "sacenv_boat_math.h"
#include "sacenv_boat_wind.h"
#include "mt19937.h"

#pragma clang fp contract(off)

namespace {

struct RngLds {           // an episode draw (k_refill: 5.3 KB, more waves per CU)
  uint32_t win[kWave];    // MT window (tempered words pos .. pos+63)
  uint32_t blk[2][kMtN];  // current MT block, next (twisted) block
  double y[2][kMaxK];     // knot values per curve (unfolded)
};
struct DrawLds : RngLds {  // draw + wave fit (init / host resets)
  double m[2][kMaxK];     // second derivatives / 6 per curve (unfolded)
  double g[kMaxK * kMaxK];
};

// ---------------------------------------------------------------- spline constants

__device__ __forceinline__ void load_g(const SacenvBoatParams& p, const double* g, DrawLds& l, int lane) {
  for (int i = lane; i < p.n_knots * p.n_knots; i += kWave) l.g[i] = g[i];
  __syncthreads();
}

// ---------------------------------------------------------------- episode draw

// The RNG half of Boat(config) for env `e`, by all 64 lanes (e uniform):
// np.random.randint(-hw, hw) (boat_env.py:147-150), then n knot values per
// random curve (wind.py:78; velocity first in exp 6) into l.y. Explicit
// draws (replays) bypass the RNG. Returns start_y in all lanes.
__device__ int32_t draw_knots_wave(const SacenvBoatParams& p, const Arena& A, RngLds& l, int e,
                                   int lane, const int32_t* ex_start_y, const double* ex_knots,
                                   int pos0 = -1, bool have_w0 = false, uint32_t w0_pre = 0u) {
  const int nk = p.n_knots;
  // draws follow the reference even when a recorded wind table overrides the
  // curves; only the spline fit is skipped then
  const int ndraw = n_curves(p.experiment);
  const int ncurves = owner_curves(p);
  if (ex_start_y != nullptr) {
    for (int c = 0; c < ncurves; ++c)
      if (lane < nk) l.y[c][lane] = ex_knots[c * nk + lane];
    return *ex_start_y;
  }
  MtStream st;
  st.gkey = A.mt_key() + (int64_t)e * kMtN;
  st.pos = pos0 >= 0 ? pos0 : A.i32(U_MTPOS)[e] & kMtPosMask;  // pos0: prefetched by the caller
  // (a pos0 past 624 lies in the block after mt_key: mt_fetch twists mt_key to it;
  // mt_finish stores the index plain, withdrawing mt_next)
  st.cur = 0;
  st.loaded = false;
  st.nxt_valid = false;
  st.advanced = false;
  const uint32_t rng = (uint32_t)(2 * p.start_y_half - 1), mask = range_mask32(rng);  // masked rejection
  uint32_t val = 0;
  const int need = 2 * nk * ndraw;  // words of the knot values after the randint
  // the first window, or the caller's copy of it (raw words pos0 .. pos0+63 of the
  // stored block, loaded ahead when the window does not cross the block end)
  const uint32_t w0 = have_w0 ? mt_temper(w0_pre) : mt_fetch(st, l, lane);
  const unsigned long long acc0 = __ballot(((w0 & mask) <= rng) && lane < kWave - need);
  if (acc0) {
    // fast path: one 64-word window holds the randint draw and every knot
    const int k = __ffsll((long long)acc0) - 1;
    val = (uint32_t)__builtin_amdgcn_readlane((int)w0, k) & mask;
    if (ndraw > 0) {  // window through LDS: per-lane gathers without bpermute
      l.win[lane] = w0;
      __syncthreads();
    }
    for (int c = 0; c < ndraw; ++c) {
      const int src = k + 1 + c * 2 * nk + ((2 * lane) & 31);
      const uint32_t wa = l.win[src & (kWave - 1)];
      const uint32_t wb = l.win[(src + 1) & (kWave - 1)];
      if (lane < nk) l.y[c][lane] = res53(wa, wb);  // np.random.sample
    }
    st.pos += k + 1 + need;
  } else {
    // general path: rejection runs past the window, or the knots do
    for (;;) {
      const uint32_t w = mt_fetch(st, l, lane);
      const unsigned long long acc = __ballot((w & mask) <= rng);
      if (acc) {
        const int k = __ffsll((long long)acc) - 1;
        val = (uint32_t)__builtin_amdgcn_readlane((int)w, k) & mask;
        st.pos += k + 1;
        break;
      }
      st.pos += kWave;
    }
    for (int c = 0; c < ndraw; ++c) {
      const uint32_t w = mt_fetch(st, l, lane);
      l.win[lane] = w;
      __syncthreads();
      const uint32_t wa = l.win[(2 * lane) & (kWave - 1)];
      const uint32_t wb = l.win[(2 * lane + 1) & (kWave - 1)];
      if (lane < nk) l.y[c][lane] = res53(wa, wb);
      __syncthreads();
      st.pos += 2 * nk;
    }
  }
  mt_finish(st, l, A.i32(U_MTPOS) + e, lane);
  return -p.start_y_half + (int32_t)val;
}

// The spline half: from the knot values in l.y (lanes 16c + j hold knot j of
// curve c), second derivatives m = G @ y, exact grid min/max, the min-max
// renormalisation (wind.py:87-89) and the table scaling (wind.py:86-99);
// stores the folded coefficients of `slot`. l.g must be loaded.
__device__ void fit_store_wave(const SacenvBoatParams& p, const Arena& A, DrawLds& l, int e, int slot,
                               int lane) {
  const int nk = p.n_knots;
  const int ncurves = owner_curves(p);
  if (ncurves == 0) return;
  __syncthreads();
  const int c = lane >> 4, j = lane & 15;
  const bool knot_lane = c < ncurves && j < nk;
  double yv = 0.0, mv = 0.0;
  if (knot_lane) {
    yv = l.y[c][j];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
      if (k < nk) mv += l.g[j * nk + k] * l.y[c][k];
    l.m[c][j] = mv;
  }
  __syncthreads();
  // lanes 32c + u work on curve c: S lanes per interval (4 if <= 8 intervals)
  double mn = INFINITY, mx = -INFINITY;
  {
    const int cc = lane >> 5, u = lane & 31;
    if (nk - 1 <= 8) {
      const int jj = u >> 2;
      if (cc < ncurves && jj < nk - 1)
        interval_extrema<4>(p, jj, u & 3, l.y[cc][jj], l.y[cc][jj + 1], l.m[cc][jj], l.m[cc][jj + 1], mn, mx);
    } else {
      if (cc < ncurves && u < nk - 1)
        interval_extrema<1>(p, u, 0, l.y[cc][u], l.y[cc][u + 1], l.m[cc][u], l.m[cc][u + 1], mn, mx);
    }
  }
  mn = group_min<16>(mn);
  mx = group_max<16>(mx);
  // curve c's extremes are the two rows of its half-wave: uniform values
  const double cmn0 = fmin(readlane_f64(mn, 0), readlane_f64(mn, 16));
  const double cmx0 = fmax(readlane_f64(mx, 0), readlane_f64(mx, 16));
  const double cmn1 = fmin(readlane_f64(mn, 32), readlane_f64(mn, 48));
  const double cmx1 = fmax(readlane_f64(mx, 32), readlane_f64(mx, 48));
  mn = c == 0 ? cmn0 : cmn1;
  mx = c == 0 ? cmx0 : cmx1;
  if (knot_lane) {
    fold_knot(p, c, mn, mx, yv, mv);
    *reinterpret_cast<double2*>(A.wind_knots() + 2 * A.wix(slot, c, j, e)) = double2{yv, mv};
  }
  __syncthreads();
}

// start y and (raw, or SACENV_OUT_KNOTS) the raw knot values of a drawn episode
__device__ __forceinline__ void store_draw(const SacenvBoatParams& p, const Arena& A, const RngLds& l,
                                           int e, int slot, int32_t start_y, int lane, bool raw = false) {
  const int nk = p.n_knots;
  const int ncurves = owner_curves(p);
  if (lane == 0) A.i32(U_STARTY)[(int64_t)slot * A.np + e] = start_y;
  const int c = lane >> 4, j = lane & 15;
  if (c < ncurves && j < nk) {
    if (raw) A.wind_knots()[2 * A.wix(slot, c, j, e)] = l.y[c][j];  // the fit's input, in the slot's y
    if (A.rk) A.knots_raw()[A.wix(slot, c, j, e)] = l.y[c][j];
  }
}

// Boat(config) in one go (init / host-driven resets): draw + fit into slot.
__device__ int32_t draw_episode_wave(const SacenvBoatParams& p, const Arena& A, DrawLds& l, int e,
                                     int slot, int lane, const int32_t* ex_start_y,
                                     const double* ex_knots) {
  const int32_t start_y = draw_knots_wave(p, A, l, e, lane, ex_start_y, ex_knots);
  __syncthreads();
  store_draw(p, A, l, e, slot, start_y, lane);
  fit_store_wave(p, A, l, e, slot, lane);
  return start_y;
}

// scalar state of a fresh Boat (boat_env.py:152-198) and its observation;
// the wind piece copy of the episode in `slot` starts at its first interval
__device__ __forceinline__ Obs fresh_state(const SacenvBoatParams& p, const Arena& A, const Tail& T, int e,
                                           int32_t start_y, int slot) {
  const double s_y = p.experiment == 2 ? (double)start_y : 0.0;  // :166-169
  const int nc = owner_curves(p);
  const uint32_t eo = (uint32_t)e * 8u;
  for (int c = 0; c < nc; ++c) {
    double q[4];
    A.piece(slot, c, 0, e, q);
    for (int k = 0; k < 4; ++k) A.f64e(U_COEF + 32 * c + 8 * k, eo) = q[k];
  }
  A.f64e(U_SX, eo) = 0.0;
  A.f64e(U_SY, eo) = s_y;
  A.f64e(U_SR, eo) = 0.0;
  A.f64e(U_VX, eo) = 0.0;
  A.f64e(U_VY, eo) = 0.0;
  A.f64e(U_VR, eo) = 0.0;
  A.f64e(U_RUD, eo) = 0.0;
  A.f64e(U_T, eo) = 0.0;
  A.f64e(U_EP, eo) = 0.0;  // :122
  A.i32(U_IDX)[e] = 0;
  if (p.out_flags & SACENV_OUT_ACCEL) {  // a fresh Boat's a_x, a_y, a_r are 0 (:182-196)
    A.at_e<double>(A.ur() + R_AX, eo) = 0.0;
    A.at_e<double>(A.ur() + R_AY, eo) = 0.0;
    A.at_e<double>(A.ur() + R_AR, eo) = 0.0;
  }
  return make_obs(p, obs_const(T), 0.0, 0.0, 0.0, s_y, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, (double)p.fuel0);
}

constexpr int kAheadEnvs = 8;  // envs per twist-ahead workgroup of the fit launch (mt_ahead)
// mt19937_gen of one block by one wave, from memory and in registers: word i
// needs old[i], old[i+1] and old[i+397] (i < 227) or new[i-227], so lane l
// forms the chains c, c+227, c+454 for c = l, l+64, l+128, l+192 (< 227) and
// every dependency but word 623's (new[0], new[396]: two readlanes) stays in
// the lane -- no LDS, no barriers. All loads complete before the first store,
// so o may be n (the block made current is twisted in place); with `cur`, the
// old block is also copied there.
__device__ __forceinline__ void mt_twist_regs(const uint32_t* o, uint32_t* n, uint32_t* cur, int lane) {
  constexpr int kD = kMtN - kMtM;  // 227
  uint32_t a0[4], a1[4], a2[4], b0[4], b1[4], c0[4], c1[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane + kWave * k;
    const bool ok = c < kD, okc = c < kMtN - 1 - 2 * kD;  // (c + 454 < 623)
    a0[k] = ok ? o[c] : 0u;
    a1[k] = ok ? o[c + 1] : 0u;
    a2[k] = ok ? o[c + kMtM] : 0u;
    b0[k] = ok ? o[c + kD] : 0u;
    b1[k] = ok ? o[c + kD + 1] : 0u;
    c0[k] = okc ? o[c + 2 * kD] : 0u;
    c1[k] = okc ? o[c + 2 * kD + 1] : 0u;
  }
  const uint32_t last = o[kMtN - 1];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  uint32_t nb2 = 0u, na0 = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane + kWave * k;
    if (c < kD) {
      const uint32_t na = mt_mix(a0[k], a1[k], a2[k]);
      const uint32_t nb = mt_mix(b0[k], b1[k], na);
      n[c] = na;
      n[c + kD] = nb;
      if (cur) cur[c] = a0[k], cur[c + kD] = b0[k];
      if (c < kMtN - 1 - 2 * kD) {
        n[c + 2 * kD] = mt_mix(c0[k], c1[k], nb);
        if (cur) cur[c + 2 * kD] = c0[k];
      }
      if (k == 0) na0 = na;
      if (k == 2) nb2 = nb;
    }
  }
  // word 623: mix(old[623], new[0], new[396]); new[396] = chain 169 = lane 41, k = 2
  const uint32_t n0 = (uint32_t)__builtin_amdgcn_readlane((int)na0, 0);
  const uint32_t n396 = (uint32_t)__builtin_amdgcn_readlane((int)nb2, kMtM - 1 - kD - 2 * kWave);
  if (lane == 0) {
    n[kMtN - 1] = mt_mix(last, n0, n396);
    if (cur) cur[kMtN - 1] = last;
  }
}

// The fit launch's first np/kAheadEnvs workgroups twist each env's next MT
// block ahead (mt_next, flagged kMtNextOk in U_MTPOS), so k_refill's 16-lane
// groups draw windows that cross a block end from memory instead of leaving
// the fast path for a wave-per-env draw with its twist (one in ~13 episodes).
// An env whose draws ran into mt_next (index past 624) first gets it as its
// current block. Needed by the envs that crossed or went through a wave draw
// since the last refill (all of them after seeding); the rest are skipped.
__device__ __forceinline__ void mt_ahead(const SacenvBoatParams& p, const Arena& A, int b, int lane) {
  const int e0 = b * kAheadEnvs;
  int v = 0;
  bool need = false;
  // (past 8 knots every draw is a wave draw, which withdraws mt_next: nothing to gain)
  if (lane < kAheadEnvs && e0 + lane < p.n_envs && p.n_knots <= 8) {
    v = A.i32(U_MTPOS)[e0 + lane];
    need = (v & kMtNextOk) == 0 || (v & kMtPosMask) > kMtN;
  }
  unsigned long long m = __ballot(need);
#pragma unroll 1
  while (m != 0ull) {  // uniform
    const int j = __ffsll((long long)m) - 1;
    m &= m - 1ull;
    const int e = e0 + j;
    const int vj = __builtin_amdgcn_readlane(v, j);
    const bool adv = (vj & kMtNextOk) != 0 && (vj & kMtPosMask) > kMtN;
    uint32_t* const key = A.mt_key() + (int64_t)e * kMtN;
    uint32_t* const nxt = A.mt_next() + (int64_t)e * kMtN;
    mt_twist_regs(adv ? nxt : key, nxt, adv ? key : nullptr, lane);
    if (lane == 0) A.i32(U_MTPOS)[e] = ((vj & kMtPosMask) - (adv ? kMtN : 0)) | kMtNextOk;
  }
}

}  // namespace
