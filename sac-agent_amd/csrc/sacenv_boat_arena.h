// sacenv_boat_arena.h — the boat arena: the per-env units (U_*) and record columns (R_*), the
// layout (compute_layout), the device view (Arena), the host-built launch constants (Tail), and
// the rules host and device both read (n_curves, owner_curves, t_from_index).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sacenv.h"

namespace {
constexpr int kWave = 64;
}  // namespace

#include "mt19937.h"  // kMtN: the arena holds each env's two MT blocks

namespace {

constexpr int kMaxK = SACENV_MAX_KNOTS;
constexpr int kSlots = SACENV_SLOTS;
constexpr double kPi = 3.141592653589793;  // np.pi

// Per-env byte widths; a field's offset is (sum of widths before it) * n_pad.
// n_pad is a multiple of 64, so every array is 64-byte aligned.
// U_COEF / U_W0N / U_SYN are lane-coalesced copies of slot data the step
// reads every launch (see owner_wave): the active episode's spline piece
// (y0, y1, m0, m1 per curve) of the interval of this step's wind sample, and
// the next episode's curve values at grid index 0 and start y. Slots differ
// from env to env, so reading them from the slot ring itself would scatter
// every wave's loads over up to 33 rows. U_COEF follows the carried state
// directly: owner_wave loads both as 16-B pairs (U_PAIRED, below).
constexpr int U_SX = 0, U_SY = 8, U_SR = 16, U_VX = 24, U_VY = 32, U_VR = 40, U_RUD = 48,
              U_EP = 56, U_COEF = 64, U_W0N = 128, U_T = 144, U_IDX = 152,
              U_CONS = 156, U_FILL = 160, U_MTPOS = 164, U_SYN = 168, U_STARTY = 172,
              U_CNT = U_STARTY + 4 * kSlots,
              U_LIST = U_CNT + 4 * SACENV_N_COUNTERS, U_CSNAP = U_LIST + 12, U_LTERM = U_CSNAP + 4,
              U_WIND = U_LTERM + 4;
constexpr int U_MT_BYTES = 4 * kMtN;
// U_MTPOS holds the MT word index (bits 0..15, up to 2 x 624) and kMtNextOk:
// mt_next holds the block after mt_key (twisted ahead by the refill's fit
// launch), so a draw window may run past the block end without a twist; an
// index past 624 then reads mt_next, and the fit launch makes it current.
// Every other writer of the index (the wave-path draws, seeding, the host)
// stores it plain, which withdraws the pre-twisted block.
constexpr int kMtPosMask = 0xFFFF, kMtNextOk = 1 << 16;
// The f64 fields below U_PAIRED are stored as 16-B pairs per env, [n_pad][2]:
// (s_x, s_y) (s_r, v_x) (v_y, v_r) (rudder, ep_reward), the spline piece as
// (y0, m0) (y1, m1) per curve, and the two next-episode y0. A field's pair
// block starts at (u & ~15) * n_pad and it is element (u & 8) / 8 of each
// pair, so the step moves them with 16-B per-lane loads and stores.
constexpr int U_PAIRED = 144;
constexpr int64_t kWindUnits = 16LL * kSlots;  // f64 x 2 curves x slots, per knot

__host__ __device__ inline int64_t pad64(int64_t n) { return (n + 63) / 64 * 64; }
__host__ __device__ inline int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }

// The packed record's per-env byte columns (sacenv.h: what a step hands out, and
// what sacenv_boat_rollout writes per step), then the columns that follow the
// record in the arena: field f starts (record_unit + R_f) * n_pad bytes in.
constexpr int R_OBS = SACENV_REC_OBS, R_REWARD = SACENV_REC_REWARD, R_DONE = SACENV_REC_DONE,
              R_TERM = SACENV_REC_TERM, R_FIN = SACENV_RECORD_BYTES,  // final_obs: f32 [n_pad][11]
              R_FIN_EP = R_FIN + 4 * SACENV_OBS_DIM,                   // final_ep_reward: f64
              R_AX = R_FIN_EP + 8, R_AY = R_AX + 8, R_AR = R_AY + 8,   // accel: f64 [3][n_pad]
              R_REWARD64 = R_AR + 8, R_END = R_REWARD64 + 8;
static_assert(R_OBS == 0 && R_REWARD == 4 * SACENV_OBS_DIM && R_DONE == R_REWARD + 4 && R_TERM == R_DONE + 1 &&
                  SACENV_RECORD_BYTES == R_TERM + 1,
              "record: obs f32 x 11, reward f32, done u8, term u8");
static_assert(R_FIN == 50 && R_FIN_EP == 94 && R_AX == 102 && R_AY == 110 && R_AR == 118 && R_REWARD64 == 126 &&
                  R_END == 134,
              "the arena columns behind the record (SacenvBoatLayout, ABI 20)");
static_assert(R_FIN_EP % 2 == 0 && (R_AX - R_FIN_EP) % 8 == 0, "f64 columns stay 8-B aligned (n_pad % 64 == 0)");

// The record's unit offset (its byte offset / n_pad): behind the slot ring (with
// the raw knots when SACENV_OUT_KNOTS keeps them) and the two MT blocks.
__host__ __device__ inline int64_t record_unit(int nk, int rk) {
  return U_WIND + (2 + rk) * (kWindUnits * nk) + 2 * U_MT_BYTES;
}
// Byte offsets of what follows the per-env fields, each 256-B aligned: the refill
// masks (one 64-bit word per owner wave), the status words, the spline matrix and
// the shared wind table.
__host__ __device__ inline int64_t off_refill_mask(int64_t ur, int64_t np) { return align256((ur + R_END) * np); }
__host__ __device__ inline int64_t refill_mask_bytes(int64_t np) { return align256(8 * (int)(np / 64)); }
__host__ __device__ inline int64_t off_status(int64_t ur, int64_t np) {
  return off_refill_mask(ur, np) + refill_mask_bytes(np);
}
__host__ __device__ inline int64_t off_spline_g(int64_t ur, int64_t np) { return off_status(ur, np) + 256; }
__host__ __device__ inline int64_t off_wind_table(int64_t ur, int64_t np) {
  return off_spline_g(ur, np) + align256(8LL * kMaxK * kMaxK);
}

__host__ __device__ inline void compute_layout(int n, int nk, int L, int use_table, int raw_knots,
                                               SacenvBoatLayout* o) {
  const int64_t np = pad64(n);
  o->n_pad = np;
  // paired fields: the offset of env 0's element; consecutive envs are 16 B apart
  auto pair_off = [np](int u) { return (int64_t)(u & ~15) * np + (u & 8); };
  o->s_x = pair_off(U_SX);
  o->s_y = pair_off(U_SY);
  o->s_r = pair_off(U_SR);
  o->v_x = pair_off(U_VX);
  o->v_y = pair_off(U_VY);
  o->v_r = pair_off(U_VR);
  o->rudder = pair_off(U_RUD);
  o->t = U_T * np;
  o->ep_reward = pair_off(U_EP);
  o->wind_coef = U_COEF * np;
  o->wind0_next = U_W0N * np;
  o->start_y_next = U_SYN * np;
  o->index = U_IDX * np;
  o->cons = U_CONS * np;
  o->fill = U_FILL * np;
  o->mt_pos = U_MTPOS * np;
  o->start_y = U_STARTY * np;
  o->counters = U_CNT * np;
  o->refill_list = U_LIST * np;
  // the drawn knots (raw, before the fit) are kept per slot only when asked for
  // (SACENV_OUT_KNOTS); the refill's fit reads them from the slot's own y fields
  const int64_t uw = U_WIND, wk = kWindUnits * nk, rk = raw_knots ? 1 : 0;
  o->wind_knots = uw * np;
  o->knots_raw = raw_knots ? (uw + 2 * wk) * np : -1;
  o->mt_key = (uw + (2 + rk) * wk) * np;
  o->mt_next = o->mt_key + U_MT_BYTES * np;
  const int64_t ur = record_unit(nk, (int)rk);
  o->record = ur * np;
  o->obs = (ur + R_OBS) * np;
  o->reward = (ur + R_REWARD) * np;
  o->done = (ur + R_DONE) * np;
  o->term = (ur + R_TERM) * np;
  o->final_obs = (ur + R_FIN) * np;
  o->final_ep_reward = (ur + R_FIN_EP) * np;
  o->accel = (ur + R_AX) * np;
  o->reward64 = (ur + R_REWARD64) * np;
  o->refill_mask = off_refill_mask(ur, np);
  o->status = off_status(ur, np);
  o->spline_g = off_spline_g(ur, np);
  o->wind_table = off_wind_table(ur, np);
  o->total_bytes = o->wind_table + (use_table ? align256(16LL * L) : 0);
  o->last_term = U_LTERM * np;
}

// Device view: pointers are recomputed from (base, n_pad, n_knots) at use,
// which keeps the kernels' scalar-register footprint small.
struct Arena {
  char* b;
  int64_t np;
  int nk;
  int rk;  // 1: knots_raw is allocated (SACENV_OUT_KNOTS)
  template <class T>
  __device__ __forceinline__ T* at(int64_t units) const { return reinterpret_cast<T*>(b + units * np); }
  __device__ __forceinline__ int32_t* i32(int u) const { return at<int32_t>(u); }
  __device__ __forceinline__ int nwaves() const { return (int)(np / 64); }
  __device__ __forceinline__ int64_t wk() const { return kWindUnits * nk; }
  // episode-contiguous slot storage: [env][slot][curve][knot] (+ [y, m] pairs)
  __device__ __forceinline__ double* wind_knots() const { return at<double>(U_WIND); }
  __device__ __forceinline__ double* knots_raw() const { return at<double>(U_WIND + 2 * wk()); }
  __device__ __forceinline__ uint32_t* mt_key() const { return at<uint32_t>(U_WIND + (2 + rk) * wk()); }
  __device__ __forceinline__ uint32_t* mt_next() const { return mt_key() + kMtN * np; }
  __host__ __device__ __forceinline__ int64_t ur() const { return record_unit(nk, rk); }
  __device__ __forceinline__ float* obs() const { return at<float>(ur() + R_OBS); }
  __device__ __forceinline__ float* final_obs() const { return at<float>(ur() + R_FIN); }
  __device__ __forceinline__ double* accel() const { return at<double>(ur() + R_AX); }
  __device__ __forceinline__ double* reward64() const { return at<double>(ur() + R_REWARD64); }
  __device__ __forceinline__ char* tail() const { return b + off_refill_mask(ur(), np); }
  // envs of owner wave w that ended since the last refill
  __device__ __forceinline__ unsigned long long* refill_mask() const {
    return reinterpret_cast<unsigned long long*>(tail());
  }

  // per refill rank: the env's MT position as k_need_masks read it (its episode
  // counter goes to refill_list(2)): the refill tops the ring up from these
  // snapshots, so a step launch that runs concurrently with the refill (and
  // rewrites cons) cannot change what it draws
  __device__ __forceinline__ int32_t* cons_snap() const { return i32(U_CSNAP); }
  // [0] refills done, [1] SACENV_STATUS_* bits, [2] envs ranked by the last refill
  __device__ __forceinline__ int32_t* status() const {
    return reinterpret_cast<int32_t*>(tail() + refill_mask_bytes(np));  // (= b + off_status)
  }
  // refill rank -> [0] env, [1] first and [2] end episode number drawn
  __device__ __forceinline__ int32_t* refill_list(int k) const { return i32(U_LIST + 4 * k); }
  // element index of (env, slot, curve, knot) in knots_raw; x2 (+1) in wind_knots
  __device__ __forceinline__ int64_t wix(int slot, int c, int k, int e) const {
    return (((int64_t)e * kSlots + slot) * 2 + c) * nk + k;
  }
  // The slot ring of a wave's 64 envs is one contiguous block: its base is
  // uniform (64-bit, scalar registers) and a lane's (y, m) offset inside it
  // stays 32-bit (< 64 x 33 KB), so the step's gathers keep the SGPR-base
  // addressing mode at any env count.
  __device__ __forceinline__ const char* wk_wave(int e0) const {
    return reinterpret_cast<const char*>(wind_knots()) + (int64_t)e0 * (int64_t)kSlots * 32 * nk;
  }
  __device__ __forceinline__ uint32_t wko_l(int slot, int c, int k, int l) const {
    return ((((uint32_t)l * (uint32_t)kSlots + (uint32_t)slot) * 2u + (uint32_t)c) * (uint32_t)nk + (uint32_t)k) * 16u;
  }
  // the 32 contiguous bytes at byte offset off of the wave's ring block (wk_wave). owner_wave
  // gives its refreshing lanes their piece's offset and the others 0, the block's first line
  // (a fixed address: one cache line per wave), so the load needs no branch
  __device__ __forceinline__ void piece_at(const char* wbase, uint32_t off, double (&q)[4]) const {
    const char* base = wbase + off;
    const double2 a = *reinterpret_cast<const double2*>(base), b = *reinterpret_cast<const double2*>(base + 16);
    q[0] = a.x, q[1] = a.y, q[2] = b.x, q[3] = b.y;  // memory order: y0, m0, y1, m1
  }
  // (y, m) of knot k and k+1 of env e
  __device__ __forceinline__ void piece(int slot, int c, int k, int e, double (&q)[4]) const {
    piece_at(wk_wave(e & ~63), wko_l(slot, c, k, e & 63), q);
  }
  // Per-lane accesses as uniform base + 32-bit byte offset: the compiler then
  // uses the SGPR-base addressing mode (no 64-bit address arithmetic in VALU).
  // Offsets stay below 2^32 for n_envs <= 2^22 (check_params).
  template <class T>
  __device__ __forceinline__ T& at_e(int64_t unit, uint32_t off) const {
    return *reinterpret_cast<T*>(b + unit * np + off);
  }
  // the per-env fields below U_WIND: the whole byte offset in 32 bits (u < 724
  // and n_pad <= 2^22 by check_params), so each access is one VALU add
  // on the lane offset and an SGPR-base load/store
  template <class T>
  __device__ __forceinline__ T& at_s(int u, uint32_t off) const {
    return *reinterpret_cast<T*>(b + ((uint32_t)u * (uint32_t)np + off));
  }
  __device__ __forceinline__ double& f64e(int u, uint32_t eo) const {
    return u < U_PAIRED ? at_s<double>(u & ~15, 2u * eo + (uint32_t)(u & 8)) : at_s<double>(u, eo);
  }
  // the pair whose block starts at unit u (16-aligned, < U_PAIRED)
  __device__ __forceinline__ double2& f64p(int u, uint32_t eo) const { return at_s<double2>(u, 2u * eo); }
  __device__ __forceinline__ int32_t& i32e(int u, uint32_t eo4) const { return at_s<int32_t>(u, eo4); }
};

__host__ inline Arena make_arena(const SacenvBoatParams& p, void* base) {
  return Arena{static_cast<char*>(base), pad64(p.n_envs), p.n_knots, (p.out_flags & SACENV_OUT_KNOTS) ? 1 : 0};
}

// Launch constants built on the host: the small tables whose offsets depend
// on n_helpers / wind_len, and the reciprocals of the config divisors (IEEE
// 1/x on the host is the same double as on the device; computing them here
// keeps eight uniform fp64 divisions out of every lane).
struct Tail {
  const double* g;
  const double* table;
  double r_mx, r_my, r_iz, r_nd, r_w;  // 1/(m+m_x), 1/(m+m_y), 1/(I+I_z), 1/(n D), 1/width
  double r_goal, r_two_w, r_fuel;      // observation spans: 1/goal, 1/(2 width), 1/fuel
  // the force laws' constant factors, folded once per launch (make_tail): each
  // law is then (velocity^2) x one constant instead of a left-to-right chain of
  // four to six products (boat_env.py:213-281); ~30 fewer f64 multiplies a
  // step, rounding within ~2 ulp of the reference's order (state tolerance 1e-5)
  double k_front, k_thrust, k_side, k_rud_front, k_hull, k_rud_moment;
};

__host__ __device__ __forceinline__ int n_curves(int experiment) {
  return experiment == 6 ? 2 : (experiment == 4 || experiment == 5) ? 1 : 0;
}
// The spline curves a launch fits and evaluates: none when a recorded wind table
// overrides them (the draws still follow n_curves). owner_wave's kNc.
__host__ __device__ __forceinline__ int owner_curves(const SacenvBoatParams& p) {
  return p.use_wind_table ? 0 : n_curves(p.experiment);
}

// t += dt (boat_env.py:69) accumulates exactly when dt = m * 2^e with m < 2^22:
// every partial sum k*dt (k <= 2^31) is then a double, so t == index * dt
// bit for bit and t need not be carried in HBM (8 B read + 8 B write per
// env-step for the default dt = 0.25).
__host__ __device__ inline bool t_from_index(double dt) {
  uint64_t bits;
  memcpy(&bits, &dt, sizeof bits);
  return (bits & ((1ull << 30) - 1ull)) == 0ull;
}

}  // namespace
