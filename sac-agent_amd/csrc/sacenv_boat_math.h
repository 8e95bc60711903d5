// sacenv_boat_math.h — the step's hand-written fp64 math: the polynomial constants as
// VGPR copies (TrigK, vconst), exp_v, sin_taylor, sincos_*, trig3 and div_c, and the
// normalised observation (Obs, ObsConst, make_obs).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sacenv.h"
#include "sacenv_boat_arena.h"

#pragma clang fp contract(off)

namespace {

// A wave-uniform test: does any active lane hold x? Where x is one compare with no
// other use the compiler branches on the compare's own lane mask; where x has other
// uses (the step's refresh predicate) it rebuilds the mask with a 0/1 select and a
// second compare, and does so for __builtin_amdgcn_ballot_w64 too, alone or as the
// scalar or of one ballot per compare (the same or one instruction more: DESIGN §4.1).
__device__ __forceinline__ bool any_lane(bool x) { return __ballot(x) != 0ull; }

// The polynomial coefficients below as loop-invariant VGPR copies (trig_k(),
// once per launch). Written as plain fma() with literals, the compiler builds
// each 64-bit coefficient with two v_mov_b32 and a v_fmac; read from SGPRs,
// it rebuilt them with two s_mov_b32 per use inside the step loop (the SGPR
// file is full with the loop's addresses): ~60 SALU issue slots per step.
struct TrigK {
  double s[10];  // sine series: 1/21!, -1/19!, 1/17!, ..., -1/3! (sincos_fast uses the last 8)
  double c[7];   // cosine series: 1/16!, -1/14!, ..., 1/4!
  double e[10];  // exp_v's polynomial (ocml's exp coefficients)
  // exp_v's other constants: log2(e), -ln2 high / low, and its overflow / underflow
  // bounds. As literals the loop rebuilt each one with two s_mov_b32 every step (an
  // SALU op between f64 ops costs ~7 cycles of one wave's issue): as VGPR copies the
  // persistent step measured 1.189 -> 1.157 us (round 6, alternating A/B)
  double ec[5];
};
__device__ __forceinline__ double vconst(double x) {
  double r;
  asm volatile("v_mov_b64 %0, %1" : "=v"(r) : "s"(x));
  return r;
}
template <bool kV = true>  // kV: VGPR copies (the multi-step loop); else plain constants
__device__ __forceinline__ TrigK trig_k() {
  constexpr double sn[10] = {1.9572941063391262e-20,  -8.22063524662432950e-18, 2.8114572543455206e-15,
                             -7.647163731819816e-13,  1.6059043836821613e-10,   -2.505210838544172e-08,
                             2.7557319223985893e-06,  -1.984126984126984e-04,   8.333333333333333e-03,
                             -1.6666666666666666e-01};
  constexpr double cs[7] = {4.779477332387385e-14, -1.1470745597729725e-11, 2.08767569878681e-09,
                            -2.755731922398589e-07, 2.48015873015873e-05,   -1.388888888888889e-03,
                            4.1666666666666664e-02};
  TrigK k;
#pragma unroll
  for (int i = 0; i < 10; ++i) k.s[i] = kV ? vconst(sn[i]) : sn[i];
#pragma unroll
  for (int i = 0; i < 7; ++i) k.c[i] = kV ? vconst(cs[i]) : cs[i];
  constexpr double ex[10] = {2.5022322536502990e-08, 2.7630903490112654e-07, 2.755751454582531e-06,
                             2.480149103909504e-05,  1.9841269589115522e-04, 1.3888888945916382e-03,
                             8.333333333455043e-03,  4.1666666666519754e-02, 1.6666666666666477e-01,
                             5.000000000000012e-01};
#pragma unroll
  for (int i = 0; i < 10; ++i) k.e[i] = kV ? vconst(ex[i]) : ex[i];
  constexpr double ec[5] = {1.4426950408889634, -0.69314718055994529, -2.3190468138462996e-17, 1024.0,
                            -1075.0};
#pragma unroll
  for (int i = 0; i < 5; ++i) k.ec[i] = kV ? vconst(ec[i]) : ec[i];
  return k;
}
__device__ __forceinline__ double fma_v(double a, double b, double c) {
  double r;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// exp(x): ocml's __ocml_exp_f64 restated operation for operation (the same
// double for every x, NaN and the range ends included: within 1 ulp of glibc,
// tools/ubench notes), its polynomial read from VGPRs. Inlined from the
// library, the compiler kept the coefficients in VGPRs but fed them to
// v_fmac, copying each one first: 9 v_mov_b64 a step.
__device__ __forceinline__ double exp_v(double x, const TrigK& K) {
  const double n = rint(x * K.ec[0]);
  double r = fma(K.ec[1], n, x);
  r = fma(K.ec[2], n, r);
  double q = fma_v(K.e[0], r, K.e[1]);
#pragma unroll
  for (int i = 2; i < 10; ++i) q = fma_v(r, q, K.e[i]);
  q = fma(r, q, 1.0);
  q = fma(r, q, 1.0);
  double e = ldexp(q, (int)n);
  e = K.ec[3] < x ? __builtin_inf() : e;
  return K.ec[4] > x ? 0.0 : e;
}

// sin(x) for |x| <= kSinBound with no argument reduction: x + x^3 P(x^2), P
// the Taylor series through x^21 (truncation < 1e-20, below half an ulp),
// about 12 FMAs against ocml's reduction + two polynomials + select.
constexpr double kSinBound = 1.25;
__device__ __forceinline__ double sin_taylor(double x, const TrigK& K) {
  const double z = x * x;
  double q = fma_v(z, K.s[0], K.s[1]);
#pragma unroll
  for (int i = 2; i < 10; ++i) q = fma_v(q, z, K.s[i]);
  return fma(x * z, q, x);  // the negated series of before, bit for bit
}

// sincos_fast's tail: the series values from the two polynomials, then the
// quadrant of k = rint(x 2/pi) (swap, and the signs as sign-bit xors)
__device__ __forceinline__ void sincos_quadrant(double r, double z, double ps, double pc, double k, double* sp,
                                                double* cp) {
  const double sr = fma(r * z, ps, r);
  const double cr = 1.0 - fma(-(z * z), pc, 0.5 * z);
  const int q = (int)k;
  const double a = (q & 1) ? cr : sr, b = (q & 1) ? sr : cr;  // sin, cos of r + (q&1) pi/2
  // negate by the quadrant as a sign-bit xor on the high word (the same double as
  // -a, signed zeros and NaNs included): q & 2 for sin, (q + 1) & 2 for cos, moved
  // to bit 31 by one shift each -- 5 VALU fewer than two compares and selects
  const uint64_t ms = (uint64_t)(((uint32_t)q << 30) & 0x80000000u) << 32;
  const uint64_t mc = (uint64_t)((((uint32_t)q + 1u) << 30) & 0x80000000u) << 32;
  *sp = __longlong_as_double((long long)((uint64_t)__double_as_longlong(a) ^ ms));
  *cp = __longlong_as_double((long long)((uint64_t)__double_as_longlong(b) ^ mc));
}

// sin and cos of x for |x| <= kCwBound: k = rint(x 2/pi), r = x - k pi/2 by fma
// in three Cody-Waite terms (each fma rounds once: r within ~1 ulp), Taylor
// polynomials on |r| <= pi/4 (sin through r^17, cos through r^16: truncation
// below 1e-17) and the quadrant swap. Within 1 ulp of glibc's sin/cos up to
// 1e13 (measured, 2e6 samples per decade); the bound keeps (int)k exact.
constexpr double kCwBound = 1.0e5;
__device__ __forceinline__ void sincos_fast(double x, double* sp, double* cp, const TrigK& K) {
  const double k = rint(x * 0.6366197723675814);
  double r = fma(-k, 1.5707963267948966, x);
  r = fma(-k, 6.123233995736766e-17, r);
  r = fma(-k, -1.4973849048591698e-33, r);
  const double z = r * r;
  double ps = fma_v(z, K.s[2], K.s[3]);
#pragma unroll
  for (int i = 4; i < 10; ++i) ps = fma_v(ps, z, K.s[i]);
  double pc = fma_v(z, K.c[0], K.c[1]);
#pragma unroll
  for (int i = 2; i < 7; ++i) pc = fma_v(pc, z, K.c[i]);
  sincos_quadrant(r, z, ps, pc, k, sp, cp);
}

// The fast forms for every lane, then ocml's for the lanes outside their
// range (NaN included) behind one wave-uniform branch that is almost never
// taken: a lane's result depends on its own argument only. Each such branch
// ends a scheduling region, so the step evaluates its early transcendentals
// (wind angle, advance ratio, rudder: all known once the action is in) in
// one region (trig3), where the three chains interleave, and keeps the one
// late one (yaw) on its own.
// (ocml's functions stay inline: called out of line, to keep their tables
// and temporaries out of the step loop's registers, the step measured
// 0.12 us slower -- the call's register save and restore conventions)
struct SinCos {
  double s, c;
};
__device__ __forceinline__ double sin_ocml(double x) { return sin(x); }
__device__ __forceinline__ SinCos sincos_ocml(double x) {
  SinCos r;
  sincos(x, &r.s, &r.c);
  return r;
}

__device__ __forceinline__ void sincos_cw(double x, double* sp, double* cp, const TrigK& K) {
  sincos_fast(x, sp, cp, K);
  const bool ok = fabs(x) <= kCwBound;
  if (__builtin_expect(any_lane(!ok), 0)) {  // (unlikely: laid out off the step's fall-through path)
    if (!ok) {
      const SinCos r = sincos_ocml(x);
      *sp = r.s, *cp = r.c;
    }
  }
}

__device__ __forceinline__ void trig3(double j, double r, double w, double* sj, double* sr, double* sw,
                                      double* cw, const TrigK& K) {
  // the four Horner chains (sin j, sin r, and the sin and cos polynomials of w's
  // reduced argument) issued interleaved, their ends aligned: each FMA's
  // dependent predecessor is three instructions back, so the chains hide each
  // other's latency (written one after the other, the asm FMAs issued as two
  // serial 10-deep chains with a hazard nop between dependent pairs). The same
  // operations as sin_taylor / sincos_fast, so the same doubles.
  const double kw = rint(w * 0.6366197723675814);
  double rw = fma(-kw, 1.5707963267948966, w);
  rw = fma(-kw, 6.123233995736766e-17, rw);
  rw = fma(-kw, -1.4973849048591698e-33, rw);
  const double zj = j * j, zr = r * r, zw = rw * rw;
  double qj = fma_v(zj, K.s[0], K.s[1]);
  double qr = fma_v(zr, K.s[0], K.s[1]);
  double ps = 0.0, pc = 0.0;
#pragma unroll
  for (int i = 2; i < 10; ++i) {
    qj = fma_v(qj, zj, K.s[i]);
    qr = fma_v(qr, zr, K.s[i]);
    if (i == 3) ps = fma_v(zw, K.s[2], K.s[3]);
    if (i >= 4) ps = fma_v(ps, zw, K.s[i]);
    if (i == 4) pc = fma_v(zw, K.c[0], K.c[1]);
    if (i >= 5) pc = fma_v(pc, zw, K.c[i - 3]);
  }
  *sj = fma(j * zj, qj, j);
  *sr = fma(r * zr, qr, r);
  sincos_quadrant(rw, zw, ps, pc, kw, sw, cw);
  const bool okj = fabs(j) <= kSinBound, okr = fabs(r) <= kSinBound, okw = fabs(w) <= kCwBound;
  if (__builtin_expect(any_lane(!(okj && okr && okw)), 0)) {
    if (!okj) *sj = sin_ocml(j);
    if (!okr) *sr = sin_ocml(r);
    if (!okw) {
      const SinCos q = sincos_ocml(w);
      *sw = q.s, *cw = q.c;
    }
  }
}

// x / c for a per-launch constant c, from r = RN(1/c): Markstein's correction
// step returns the correctly rounded quotient, i.e. the same double as IEEE
// division, in 3 dependent FLOPs instead of the ~10 of a full fp64 divide.
// For finite x only: an infinite x gives NaN (err = fma(-inf, c, inf)) where
// IEEE division gives inf (the one x that can be infinite, the action, is handled
// by its caller).
__device__ __forceinline__ double div_c(double x, double c, double r) {
  const double q = x * r;
  const double err = fma(-q, c, x);
  return fma(err, r, q);
}

// ---------------------------------------------------------------- observation
// Boat.return_state / normalize (boat_env.py:308-326): (v - lo) / (hi - lo).
// Config-dependent spans divide exactly (div_c); the reference's literal
// spans are applied as reciprocals (the float32 observation is the output).
struct Obs {
  float v[SACENV_OBS_DIM];
};

struct ObsConst {  // per-launch reciprocals of the config-dependent spans
  double goal, two_w, fuel;
  // the literal spans' reciprocals (k[7]: the rudder offset pi/3), as VGPR
  // copies in the step loop (obs_const_v): as literals each use cost two s_mov
  double k[8];
};

__device__ __forceinline__ ObsConst obs_const(const Tail& T) {
  return ObsConst{T.r_goal, T.r_two_w, T.r_fuel,
                  {1.0 / 5.0, 1.0 / 0.025, 1.0 / 0.37, 1.0 / (2 * kPi), 1.0 / 8.5e-3, 1.0 / 1.4e-5,
                   1.0 / (kPi / 3 - (-kPi / 3)), kPi / 3}};
}
__device__ __forceinline__ ObsConst obs_const_v(const Tail& T) {
  ObsConst o = obs_const(T);
#pragma unroll
  for (int i = 0; i < 8; ++i) o.k[i] = vconst(o.k[i]);
  return o;
}

__device__ __forceinline__ Obs make_obs(const SacenvBoatParams& p, const ObsConst& oc, double s_x,
                                        double v_x, double a_x, double s_y, double v_y, double a_y,
                                        double s_r, double v_r, double a_r, double rudder,
                                        double fuel) {
  Obs o;
  o.v[0] = (float)div_c(s_x, p.goal_line, oc.goal);
  o.v[1] = (float)(v_x * oc.k[0]);
  o.v[2] = (float)(a_x * oc.k[1]);
  o.v[3] = (float)div_c(s_y + p.track_width, p.track_width + p.track_width, oc.two_w);
  o.v[4] = (float)(v_y * (1.0 / 2.0));
  o.v[5] = (float)(a_y * oc.k[2]);
  o.v[6] = (float)(s_r * oc.k[3]);
  o.v[7] = (float)(v_r * oc.k[4]);
  o.v[8] = (float)(a_r * oc.k[5]);
  o.v[9] = (float)((rudder + oc.k[7]) * oc.k[6]);
  o.v[10] = (float)div_c(fuel, (double)p.fuel0, oc.fuel);
  return o;
}

}  // namespace
