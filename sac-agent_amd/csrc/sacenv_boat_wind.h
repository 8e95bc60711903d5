// sacenv_boat_wind.h — the wind curve: the spline piece the step evaluates (wind_at), the DPP /
// readlane helpers, the exact grid extrema of a fitted interval, fold_knot and the refill's group
// fit (fit_group). fit_store_wave needs the drawing wave's LDS: it is in sacenv_boat_draw.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sacenv.h"
#include "sacenv_boat_arena.h"

#pragma clang fp contract(off)

namespace {

struct Knot {
  int j;
  double t;
};

__device__ __forceinline__ Knot knot_coord(const SacenvBoatParams& p, int i) {
  const double s = (double)i * p.knot_step;
  int j = (int)s;
  if (j > p.n_knots - 2) j = p.n_knots - 2;
  return Knot{j, s - (double)j};
}

// Not-a-knot cubic on interval [j, j+1] in second-derivative form.
__device__ __forceinline__ double spline_piece(double y0, double y1, double m0, double m1, double t) {
  const double u = 1.0 - t;
  return u * y0 + t * y1 + (u * u * u - u) * m0 + (t * t * t - t) * m1;
}

__device__ __forceinline__ double curve_env(const SacenvBoatParams& p, const Arena& A, int slot, int c,
                                            int e, int i) {
  const Knot k = knot_coord(p, i);
  double q[4];
  A.piece(slot, c, k.j, e, q);
  return spline_piece(q[0], q[2], q[1], q[3], k.t);
}

// Wind.get_wind(index) (wind.py:20-24) for the tables of wind.py:26-99.
__device__ __forceinline__ void wind_at(const SacenvBoatParams& p, const Arena& A, const double* table,
                                        int slot, int e, int idx, double& wv, double& wa) {
  if (idx > p.wind_len - 1) idx = p.wind_len - 1;  // reference: IndexError
  if (idx < 0) idx = 0;
  if (p.use_wind_table) {
    wv = table[idx];
    wa = table[p.wind_len + idx];
    return;
  }
  switch (p.experiment) {
    case 3:
      wv = p.max_velocity;
      wa = p.wind_dir_rad;
      return;
    case 4:
      wv = curve_env(p, A, slot, 0, e, idx);
      wa = p.wind_dir_rad;
      return;
    case 5: {
      wv = p.max_velocity;
      const double r = curve_env(p, A, slot, 0, e, idx) <= 0.5 / 2 ? 0.0 : 1.0;  // wind.py:92-99
      wa = (r * kPi) + kPi / 2;
      return;
    }
    case 6:
      wv = curve_env(p, A, slot, 0, e, idx);
      wa = curve_env(p, A, slot, 1, e, idx);
      return;
    default:  // 1, 2: no wind
      wv = 0.0;
      wa = 0.0;
      return;
  }
}

// ---------------------------------------------------------------- cross-lane helpers

// DPP lane permutes (gfx9 dpp_ctrl): register-to-register, no LDS round trip.
template <int kCtrl>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), kCtrl, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), kCtrl, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
// min / max over each aligned group of GS lanes (8, or 16: a whole DPP row), in every lane
template <int GS>
__device__ __forceinline__ double group_min(double v) {
  v = fmin(v, dpp_f64<0xB1>(v));  // quad_perm [1,0,3,2]
  v = fmin(v, dpp_f64<0x4E>(v));  // quad_perm [2,3,0,1]
  v = fmin(v, dpp_f64<0x141>(v));  // row_half_mirror: the other quad of the 8
  if (GS == 16) v = fmin(v, dpp_f64<0x140>(v));  // row_mirror: the other 8 of the row
  return v;
}
template <int GS>
__device__ __forceinline__ double group_max(double v) {
  v = fmax(v, dpp_f64<0xB1>(v));
  v = fmax(v, dpp_f64<0x4E>(v));
  v = fmax(v, dpp_f64<0x141>(v));
  if (GS == 16) v = fmax(v, dpp_f64<0x140>(v));
  return v;
}
// lane i + 1's value (row_shl:1; the row's last lane keeps its own, unused)
__device__ __forceinline__ double next_lane_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), 0x101, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), 0x101, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int src) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src),
                          __builtin_amdgcn_readlane(__double2loint(v), src));
}
// Orders a wave's LDS accesses: what its lanes wrote before is visible to what they read
// after. A wave's LDS accesses run in issue order, so only the compiler must keep them
// in order: no workgroup barrier (a step workgroup may hold several owner waves, or toy waves).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Wave-wide inclusive prefix sum: row shifts, then row_bcast15/31 carry rows.
__device__ __forceinline__ int wave_incl_scan(int x) {
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true);   // row_shr:1
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true);   // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true);   // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true);   // row_shr:8
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);  // row_bcast:15
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);  // row_bcast:31
  return x;
}

// ---------------------------------------------------------------- spline extrema

// Grid-sample min/max of one spline interval: the cubic is monotone between
// its critical points, so the extreme grid samples of interval j are its
// first/last grid points and the neighbours of each critical point
// (tests/test_host_cpu.py::test_grid_extrema_rule_is_exact). The ten
// candidates are split over S lanes (lane s evaluates candidates s, s+S, ...);
// critical points need only grid-point accuracy, so approximate rcp/rsq do.
// Interval j's piece is (y0, y1, a, b) = (y[j], y[j+1], m[j], m[j+1]): every
// candidate lies in [lo, hi], whose grid samples all fall in interval j.
// The grid indices [lo, hi] of interval j (a launch constant per interval: the
// fit kernel forms it once per lane, not per fit).
struct IvGrid {
  double jd, lod, hid;
  bool valid;
};
__device__ __forceinline__ IvGrid interval_grid(const SacenvBoatParams& p, int j) {
  const int L = p.wind_len;
  // (inv = RN(1/knot_step) puts ceil(j inv) within one of the first grid index of
  // interval j: start one below and step up, and symmetrically for the last)
  int lo = (int)ceil((double)j * p.knot_inv) - 1;
  if (lo < 0) lo = 0;
  while (lo < L && knot_coord(p, lo).j < j) ++lo;
  int hi = (int)floor((double)(j + 1) * p.knot_inv) + 1;
  if (hi > L - 1) hi = L - 1;
  while (hi >= 0 && knot_coord(p, hi).j > j) --hi;
  return IvGrid{(double)j, (double)lo, (double)hi, lo <= hi};
}

template <int S>
__device__ __forceinline__ void interval_extrema_on(const SacenvBoatParams& p, const IvGrid& gr, int s,
                                                    double y0, double y1, double a, double b, double& mn,
                                                    double& mx) {
  mn = INFINITY;
  mx = -INFINITY;
  if (!gr.valid) return;
  const double inv = p.knot_inv;
  const double qa = 3.0 * (b - a), qb = 6.0 * a, qc = y1 - y0 - 2.0 * a - b;
  // the piece in the power basis, f(t) = y0 + c1 t + c2 t^2 + c3 t^3 (spline_piece
  // expanded: c1 = y1 - y0 - 2 m0 - m1, c2 = 3 m0, c3 = m1 - m0): 3 FMAs per
  // candidate instead of spline_piece's 11 operations. The extreme grid samples
  // agree with spline_piece's evaluation of them to a few ulp (the renormalisation
  // bar is the reference's interp1d samples, 1e-12: test_wind_tables_vs_reference)
  const double c1 = qc, c2 = 3.0 * a, c3 = b - a;
  double r0 = -1.0, r1 = -1.0;  // roots of the derivative in [0,1]; -1 = none
  const double scale = fabs(qa) + fabs(qb) + fabs(qc);
  if (fabs(qa) <= 1e-14 * scale) {
    if (qb != 0.0) r0 = -qc * __builtin_amdgcn_rcp(qb);
  } else {
    // a tiny curve's quadratic (knots below 1e-150: the squares would underflow) scaled
    // by a power of two to scale in [0.5, 1): the same roots. ldexp on each coefficient
    // is exact down to subnormal knots (the factor itself can pass 2^1023)
    double sa = qa, sb = qb, sc = qc;
    if (scale < 0x1p-500) {
      const int up = -__builtin_amdgcn_frexp_exp(scale);
      sa = ldexp(qa, up), sb = ldexp(qb, up), sc = ldexp(qc, up);
    }
    const double disc = sb * sb - 4.0 * sa * sc;
    if (disc >= 0.0) {
      const double sq = disc > 0.0 ? disc * __builtin_amdgcn_rsq(disc) : 0.0;
      const double q = -0.5 * (sb + copysign(sq, sb));
      r0 = q * __builtin_amdgcn_rcp(sa);
      if (q != 0.0) r1 = sc * __builtin_amdgcn_rcp(q);
    }
  }
  const bool ok0 = r0 > -0.01 && r0 < 1.01, ok1 = r1 > -0.01 && r1 < 1.01;
  // the candidates as doubles (exact small integers): every one lies in [lo, hi],
  // i.e. in interval j, so its knot coordinate is t = i * knot_step - j, the same
  // double knot_coord forms -- no integer conversions per candidate (v_cvt costs
  // 8 cycles at one wave per SIMD, tools/ubench/valu_mix.hip)
  const double jd = gr.jd, lod = gr.lod, hid = gr.hid;
  const double i0 = ok0 ? floor((jd + r0) * inv) : lod;
  const double i1 = ok1 ? floor((jd + r1) * inv) : lod;
#pragma unroll
  for (int t = 0; t < (10 + S - 1) / S; ++t) {
    const int q = s + S * t;  // candidate number 0..9
    double i;
    if (q == 0) {
      i = lod;
    } else if (q == 1) {
      i = hid;
    } else {
      const bool first = q < 6;
      const double d = (double)((first ? q - 2 : q - 6) - 1);
      const bool ok = first ? ok0 : ok1;
      i = fmin(fmax((first ? i0 : i1) + d, lod), hid);
      i = ok ? i : lod;
    }
    if (q < 10) {
      const double t = i * p.knot_step - jd;
      const double v = fma(fma(fma(c3, t, c2), t, c1), t, y0);
      mn = fmin(mn, v);
      mx = fmax(mx, v);
    }
  }
}
template <int S>
__device__ __forceinline__ void interval_extrema(const SacenvBoatParams& p, int j, int s, double y0,
                                                 double y1, double a, double b, double& mn,
                                                 double& mx) {
  interval_extrema_on<S>(p, interval_grid(p, j), s, y0, y1, a, b, mn, mx);
}

// wind.py:87-89 min-max renormalisation of one knot's (value, 2nd derivative)
// when the grid samples leave [0, 1], then the table scaling of wind.py:86-89
// (velocity * max_v, angle * pi * 2; exp 5 keeps the unit curve for the
// rectifier, wind.py:92-99)
__device__ __forceinline__ void fold_knot(const SacenvBoatParams& p, int c, double mn, double mx, double& yv,
                                          double& mv) {
  if (mn < 0.0 || mx > 1.0) {
    const double span = mx - mn;
    yv = (yv - mn) / span;
    mv = mv / span;
  }
  if (p.experiment == 4 || (p.experiment == 6 && c == 0)) {
    yv = yv * p.max_velocity;
    mv = mv * p.max_velocity;
  } else if (p.experiment == 6 && c == 1) {
    yv = yv * kPi * 2;
    mv = mv * kPi * 2;
  }
}

// The refill's fit (k_refill_fit: sacenv_boat_refill, launch 2) of the episodes
// launch 1 drew. A group of GS lanes (8, or 16 for more than 8 knots) fits one
// (env, curve): lane j forms m[j] = (G @ y)[j] and the grid extrema of
// interval j, the group reduces min/max by shuffles, and lane j folds and
// stores knot j (the operations of fit_store_wave in the same order:
// bit-identical coefficients).
//
// Per lane, what depends only on j (a lane constant: the group's lanes are the
// knots) is formed once per launch, by the kernel: G's row jj in registers (zero
// past nk) and interval j's grid range. kFull (nk == GS) drops every per-knot bound
// check. The group's shuffles are DPP moves inside a 16-lane row (no LDS round trip).
template <int GS, bool kFull>
__device__ __forceinline__ void fit_group(const SacenvBoatParams& p, const Arena& A, const double (&gr)[GS],
                                          const IvGrid& ig, int item, int j, int jj, int j1, int nc) {
  const int nk = kFull ? GS : p.n_knots;
  const int rr = item / nc, c = item - rr * nc;
  const int e = A.refill_list(0)[rr], f0 = A.refill_list(1)[rr], f1 = A.refill_list(2)[rr];
  for (int f = f0; f < f1; ++f) {  // uniform across the group
    const int slot = f % kSlots;
    // the curve's nk drawn knots, in the slot's y fields (k_refill put them there);
    // every lane of the group reads them all before any lane writes the fitted pairs
    const double* kr = A.wind_knots() + 2 * A.wix(slot, c, 0, e);
    double yk[GS];
#pragma unroll
    for (int k = 0; k < GS; ++k) yk[k] = kr[2 * (kFull || k < nk ? k : nk - 1)];
    double yv = kr[2 * jj];
    const double y1 = kr[2 * j1];
    // m = G @ y in the reference's order (terms past nk: none when kFull; else a
    // select, so no +0.0 term can turn a -0.0 sum into +0.0)
    double mv = 0.0;
#pragma unroll
    for (int k = 0; k < GS; ++k) {
      const double s = mv + gr[k] * yk[k];
      mv = kFull || k < nk ? s : mv;
    }
    const double m1 = next_lane_f64(mv);
    double mn, mx;
    interval_extrema_on<1>(p, ig, 0, yv, y1, mv, m1, mn, mx);  // (ig invalid: +-inf)
    mn = group_min<GS>(mn);
    mx = group_max<GS>(mx);
    if (kFull || j < nk) {
      fold_knot(p, c, mn, mx, yv, mv);
      *reinterpret_cast<double2*>(A.wind_knots() + 2 * A.wix(slot, c, j, e)) = double2{yv, mv};
    }
  }
}

}  // namespace
