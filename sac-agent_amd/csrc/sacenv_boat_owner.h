// sacenv_boat_owner.h — the owner wave, BoatEnv.step for 64 envs, one per lane: its output stores,
// its LDS, a multi-step launch's outputs and action hand-off (RollArgs, the flag helpers), the
// launch constants as VGPR copies, owner_wave and the multi-step launches' body (rollout_body).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sacenv.h"
#include "sacenv_boat_arena.h"
#include "sacenv_boat_math.h"
#include "sacenv_boat_wind.h"

#pragma clang fp contract(off)

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

// Cache policy of the step's output stores: write-through (sc1: the line
// leaves the XCD L2 as it issues, so the launch ends with no dirty lines to
// write back at its boundary; measured 0.21 us/step faster than plain stores,
// DESIGN.md §4). Scalars as agent-scope relaxed atomic stores; the 16-B pairs
// and obs rows (no 16-B sc1 atomic form) as write-through buffer stores (aux
// bit 4).
// kWT false: a plain (write-back) store, for the open-loop multi-step launch,
// whose record rows are rewritten every step in place: they stay in the XCD's
// L2 and are written back once, at the launch's end (measured: a write-through
// record made every step wait for the previous step's stores to reach memory,
// as the step's loads count behind them in vmcnt)
template <bool kWT = true, class T>
__device__ __forceinline__ void st_out(T& ref, T v) {
  if (kWT)
    __hip_atomic_store(&ref, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    ref = v;
}

// a 16-B pair of the paired state (block unit u), write-through
typedef unsigned int u4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st_pair(char* base, int u, uint32_t np, uint32_t eo, double a, double b) {
  const uint32_t off = (uint32_t)u * np + 2u * eo;
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7fffffff, 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, make_double2(a, b)), r, off, 0, 16);
}

__device__ __forceinline__ void store_obs(float* dst, const Obs& o) {
#pragma unroll
  for (int k = 0; k < SACENV_OBS_DIM; ++k) dst[k] = o.v[k];
}

// ---------------------------------------------------------------- owner wave

// The owner wave's paired state is loaded 16 B per lane, straight into
// registers. Outputs are stored per lane as soon as they are final
// (EARLY_STORE); the write-through obs rows go out through LDS as float4
// (64 rows x 44 B = 176 float4).
constexpr int kCoef = 8;  // wind_coef fields: 2 curves x (y0, y1, m0, m1)
constexpr int kMkWords = SACENV_REFILL_PERIOD / 32;  // 32-bit mark words per env (one bit per step)
struct OwnerLds {
  float obs[kWave * SACENV_OBS_DIM];  // the wave's obs rows, stored as float4
  // staged replay rows: bit (ks % 32) of mk[ks / 32][lane] marks lane's row of step ks
  // (word-major: the 64 lanes of one read hit 64 consecutive words, no bank conflict)
  uint32_t mk[kMkWords][kWave];
};

// Each dynamics field is stored as soon as it is final, so the write traffic
// drains while the wave still computes (measured: -0.15 us/step against
// staging every output for 16-B stores at the end).
#define EARLY_STORE(u, v)                      \
  do {                                         \
    if (!kRoll) st_out(A.f64e(u, eo), (v));    \
  } while (0)
#define EARLY_STORE2(u, v0, v1)                                     \
  do {                                                              \
    if (!kRoll) st_pair(A.b, (u), (uint32_t)A.np, eo, (v0), (v1));  \
  } while (0)

// (store_row with non-temporal stores: rows written once and not read back by the launch)
template <int ROW>
__device__ __forceinline__ void store_row_nt(float* row, const float* w) {
  typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
  typedef float f3u __attribute__((ext_vector_type(3), aligned(4)));
#pragma unroll
  for (int i = 0; i + 4 <= ROW; i += 4)
    __builtin_nontemporal_store(f4u{w[i], w[i + 1], w[i + 2], w[i + 3]}, reinterpret_cast<f4u*>(row + i));
  constexpr int t = ROW & ~3;
  static_assert(ROW - t == 3, "an obs row: 11 floats");
  __builtin_nontemporal_store(f3u{w[t], w[t + 1], w[t + 2]}, reinterpret_cast<f3u*>(row + t));
}

// one env's row of ROW floats (4-B aligned) from registers: dwordx4 stores,
// then the 1..3-float tail as one store
template <int ROW>
__device__ __forceinline__ void store_row(float* row, const float* w) {
  typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
  typedef float f3u __attribute__((ext_vector_type(3), aligned(4)));
  typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
#pragma unroll
  for (int i = 0; i + 4 <= ROW; i += 4) *reinterpret_cast<f4u*>(row + i) = f4u{w[i], w[i + 1], w[i + 2], w[i + 3]};
  constexpr int t = ROW & ~3;
  if (ROW - t == 3) *reinterpret_cast<f3u*>(row + t) = f3u{w[t], w[t + 1], w[t + 2]};
  if (ROW - t == 2) *reinterpret_cast<f2u*>(row + t) = f2u{w[t], w[t + 1]};
  if (ROW - t == 1) row[t] = w[t];
}

// 64 obs rows (2816 B) from LDS to a 16-B aligned row block: 3 float4 stores
template <int ROW = SACENV_OBS_DIM, bool kWT = true>  // floats per env row (11: obs; 9: the pooled row's s')
__device__ __forceinline__ void store_obs_block(const float* lds_rows, float* dst_rows, int lane) {
  const f4v* src = reinterpret_cast<const f4v*>(lds_rows);
  // write-through 16-B buffer stores (sc1, aux bit 4): 0.13 us/step faster than
  // nontemporal ones, which leave the rows dirty in L2 for the boundary
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(dst_rows, 0, 0x7fffffff, 0x00020000);
#pragma unroll
  for (int i = 0; i < (ROW * 16 + kWave - 1) / kWave; ++i) {
    const uint32_t q = (uint32_t)lane + kWave * i;
    if (q < kWave * ROW / 4)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, src[q]), r, q * 16u, 0, kWT ? 16 : 0);
  }
}

// Where a multi-step launch (kRoll: sacenv_boat_rollout, sacenv_boat_segment)
// puts step ks's outputs, and how it receives step ks's action.
struct RollArgs {
  char* rec;              // the 50-B/env record of step ks at rec + ks * rec_stride
  int64_t rec_stride;     // bytes; 0: every step into the same record (the arena's)
  float* fin;             // terminal obs of restarting envs at fin + ks * fin_stride (or null)
  int64_t fin_stride;     // floats
  char* trans;            // pooled transition row of step ks at trans + ks * trans_stride (or null)
  int64_t trans_stride;   // bytes
  // staged replay rows (kRows == 2): env e's 64-B row of step ks at stage + (e * K + ks) * 64
  // (K = n_steps: env-major, an env's rows of consecutive steps adjacent), written where bit
  // (ks % 64) of marks[e * ceil(K / 64) + ks / 64] is set (marks == null: every row)
  char* stage;
  unsigned long long* marks;  // (consumed: the launch clears the words it read)
  int64_t act_stride;     // floats between consecutive action rows
  // Action hand-off (sacenv_boat_segment): owner wave w steps ks only once
  // ready[w] >= seq0 + ks + 1, and publishes done[w] = seq0 + ks + 1 once step
  // ks's outputs are visible device-wide. ready == null: every row is ready.
  const uint32_t* ready;
  uint32_t* done;
  uint32_t seq0;
  int32_t* status;        // SACENV_STATUS_HANDOFF_TIMEOUT on a hand-off that never came
};

// A hand-off flag, read device-coherently (sc0 sc1: past the XCD's
// non-coherent L2) with a vector load. flag_issue returns the loaded VGPR
// without waiting for it; flag_value makes it uniform (and waits).
__device__ __forceinline__ uint32_t flag_issue(const uint32_t* f) {
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(f), 0, 4, 0x00020000);
  return __builtin_amdgcn_raw_buffer_load_b32(r, 0, 0, 17);
}
__device__ __forceinline__ uint32_t flag_value(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ uint32_t flag_load(const uint32_t* f) { return flag_value(flag_issue(f)); }
// an action value of an explicitly handed-off row: device-coherent like the flag
__device__ __forceinline__ float act_load(const char* row, uint32_t off) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(row), 0, 0x7fffffff,
                                                                     0x00020000);
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 17));
}
constexpr uint32_t kSpinLimit = 1u << 22;  // ~seconds of polling: then a launch gives up
// Spin until the flag reaches `want` (sequence numbers stay below 2^31). Returns
// the last value seen; on timeout flags the status and returns 0.
__device__ uint32_t wait_flag(const uint32_t* f, uint32_t want, uint32_t seen, int32_t* status, int lane) {
  for (uint32_t it = 0; seen < want; ++it) {
    if (it >= kSpinLimit) {
      if (lane == 0) atomicOr(status, SACENV_STATUS_HANDOFF_TIMEOUT);
      return 0u;
    }
    __builtin_amdgcn_s_sleep(2);
    seen = flag_load(f);
  }
  return seen;
}

// Uniform fp64 constants as VGPR copies: the step reads ~40 config doubles,
// more than the SGPR file holds next to the addresses, and SGPR spills
// (v_writelane/v_readlane pairs) cost more than VGPR operands; the owner
// wave has VGPRs to spare (LDS, not registers, bounds occupancy).
__device__ __forceinline__ SacenvBoatParams vreg_params(SacenvBoatParams q) {
  // (the force laws' factors are Tail's folded constants: not copied)
  q.dt = vconst(q.dt), q.t_max = vconst(q.t_max), q.goal_line = vconst(q.goal_line);
  q.oob_limit = vconst(q.oob_limit), q.track_width = vconst(q.track_width);
  q.m_plus_mx = vconst(q.m_plus_mx), q.m_plus_my = vconst(q.m_plus_my), q.i_plus_iz = vconst(q.i_plus_iz);
  q.one_minus_wf = vconst(q.one_minus_wf);
  q.n_times_d = vconst(q.n_times_d);
  q.reward_k = vconst(q.reward_k), q.reward_center = vconst(q.reward_center);
  q.knot_step = vconst(q.knot_step);
  return q;
}
__device__ __forceinline__ Tail vreg_tail(Tail t) {
  t.r_mx = vconst(t.r_mx), t.r_my = vconst(t.r_my), t.r_iz = vconst(t.r_iz), t.r_nd = vconst(t.r_nd);
  t.r_w = vconst(t.r_w), t.r_goal = vconst(t.r_goal), t.r_two_w = vconst(t.r_two_w), t.r_fuel = vconst(t.r_fuel);
  t.k_front = vconst(t.k_front), t.k_thrust = vconst(t.k_thrust), t.k_side = vconst(t.k_side);
  t.k_rud_front = vconst(t.k_rud_front), t.k_hull = vconst(t.k_hull), t.k_rud_moment = vconst(t.k_rud_moment);
  return t;
}

// One owner wave: BoatEnv.step for 64 consecutive envs, one per lane.
// kRoll: n_steps steps in one launch (sacenv_boat_rollout, sacenv_boat_segment)
// with the state in registers, step ks's outputs where RollArgs says; the
// state is loaded once and stored once.
// kNc: spline curves of the wind (0: constants or the shared table; 1: exp
// 4/5; 2: exp 6); kTIdx: t derived from the index (t_from_index). Both are
// launch constants; as template arguments the step carries no code (and no
// loads whose pending registers the waitcnt pass must respect) of the other
// wind kinds.
// kHand (kRoll only): rows published step by step and/or done flags (the
// closed loop); without it the loop carries no flag code at all (the launch
// checked that every row was already published).
// kLean (kRoll only): the launch's options as the persistent segment of a
// training loop has them, checked by the host dispatch (lean_launch): no
// optional outputs (out_flags == 0), autoreset on, experiment != 2,
// fuel0 != 0, and every step's record and terminal obs at the same address
// (rec_stride == fin_stride == 0). The step loop then carries no test of
// them and no code of the excluded cases.
template <bool kRoll, int kNc, bool kTIdx, bool kHand = false, int kRows = 1, bool kVc = kRoll, bool kLean = false>
__device__ __forceinline__ void owner_wave(const SacenvBoatParams& pin, const Arena& A, const Tail& Tin,
                                           const float* __restrict__ action, OwnerLds& l, int ob,
                                           int lane, int n_steps = 1, const RollArgs* ra = nullptr,
                                           char* trans1 = nullptr, uint32_t seen0 = 0u) {
#ifdef SACENV_STAMPS
  const uint64_t st_real0 = __builtin_amdgcn_s_memrealtime();
  uint64_t st_loaded = 0, st_computed = 0;
#define OWNER_STAMP(v)                                            \
  do {                                                            \
    if (!kRoll) { /* (multi-step launches: the PHASE clocks) */   \
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); \
      v = __builtin_amdgcn_s_memrealtime();                       \
    }                                                             \
  } while (0)
#else
#define OWNER_STAMP(v) \
  do {                 \
  } while (0)
#endif
  static_assert(!kLean || kRoll, "the lean options describe a multi-step launch");
  const bool autoreset = kLean || pin.autoreset != 0;
  const bool exp2 = !kLean && pin.experiment == 2;
  const bool no_fuel = !kLean && pin.fuel0 == 0;
  const uint32_t out_flags = kLean ? 0u : (uint32_t)pin.out_flags;
  const int e = ob * kWave + lane;
  const uint32_t eo = (uint32_t)e * 8u, eo4 = (uint32_t)e * 4u;  // per-lane byte offsets
  const char* const wbase = A.wk_wave(ob * kWave);  // the wave's slot-ring block (uniform)
  const bool active = e < pin.n_envs;
  // the (first) action, in flight with the state loads. A handed-off row
  // (sacenv_boat_segment) is read only after its flag says it is ready.
  // Padding lanes (e >= n_envs) read their wave's first env -- memory their own
  // wave's hand-off flag covers -- and step with action 0, so padding state
  // never depends on another wave's row.
  const char* const abase = reinterpret_cast<const char*>(action) + (active ? eo4 : (uint32_t)ob * 256u);
  // info['termination'] as the reference's info dict keeps it (main.py:83): the last
  // termination code 1..5, carried across steps and auto-resets
  uint32_t lt = (uint32_t)A.i32e(U_LTERM, eo4);
  const uint32_t* const rdy = kHand ? (ra->ready != nullptr ? ra->ready + ob : nullptr) : nullptr;
  const int64_t arow = kRoll ? ra->act_stride * 4 : 0;  // bytes between action rows
  // kHand: the latest value of this wave's ready flag (the launch waited for row 0)
  uint32_t seen = seen0;
  bool failed = false;      // a hand-off timed out: the launch stops stepping
  const bool per_step = kHand && rdy != nullptr && seen < ra->seq0 + (uint32_t)n_steps;
  float act_cur = *reinterpret_cast<const float*>(abase);
  constexpr bool t_idx = kTIdx;
  constexpr int nc = kNc;  // spline curves of the wind
  // per-lane 8-B loads straight into registers, coalesced over the wave's
  // 512-B rows; the wind piece and index first, as the wind is evaluated
  // first (measured 0.16 us/step faster than 16-B loads staged through LDS)
  int32_t index = A.i32e(U_IDX, eo4);
  int cons = autoreset ? A.i32e(U_CONS, eo4) : 0;  // (early: the refresh gathers' slot)
  double cf[kCoef];
#pragma unroll
  for (int k = 0; k < kCoef; ++k) cf[k] = 0.0;
  if (nc > 0) {  // two uniform branches, not one per field; 16-B pairs (y0, m0), (y1, m1)
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
      const double2 q = A.f64p(U_COEF + 8 * k, eo);
      cf[k] = q.x, cf[k + 1] = q.y;
    }
    if (nc > 1) {
#pragma unroll
      for (int k = 4; k < 8; k += 2) {
        const double2 q = A.f64p(U_COEF + 8 * k, eo);
        cf[k] = q.x, cf[k + 1] = q.y;
      }
    }
  }
  const double2 p_sxy = A.f64p(U_SX, eo), p_srvx = A.f64p(U_SR, eo), p_vyvr = A.f64p(U_VY, eo);
  const double2 p_rudep = A.f64p(U_RUD, eo);
  double s_x = p_sxy.x, s_y = p_sxy.y, s_r = p_srvx.x;
  double v_x = p_srvx.y, v_y = p_vyvr.x, v_r = p_vyvr.y;
  double rudder = p_rudep.x, t = t_idx ? 0.0 : A.f64e(U_T, eo), ep = p_rudep.y;
  // keep the whole load burst ahead of the first computation: the scheduler
  // would otherwise hoist the refresh-address math (index, cons) above the
  // state loads and wait for those two first
  __builtin_amdgcn_sched_barrier(0);
  // (the caller moved the fp64 constants to VGPRs ahead of the load burst:
  // measured 0.09 us/step faster than doing it here, behind the burst)
  const SacenvBoatParams& p = pin;
  const Tail& T = Tin;
  constexpr bool kWT = !kRoll || kHand;  // write-through outputs (st_out)
  // one-step launch: plain constants (the compiler places them; the VGPR copies
  // cost their moves in every launch: k_step 5.02 -> 5.36 us measured), the
  // multi-step loop: VGPR copies, moved once per launch
  const TrigK K = trig_k<kVc>();
  const ObsConst oc = kVc ? obs_const_v(T) : obs_const(T);
  // Wind.get_wind(index) (wind.py:20-24, IndexError guard) of this step. Curves:
  // from the lane's copy of its spline piece (wind_coef, loaded with the
  // state). The copy is refreshed from the active slot at the end of a step
  // whose successor enters the next knot interval, and in an episode's first
  // step (a new episode starts with y0 = y(0) in the piece, exact at t = 0
  // whatever the other fields hold): the few lanes that refresh issue their scattered slot
  // loads here and store the piece at the end.
  // rollout: the next pre-drawn episode's y(0) and start y, carried in registers
  double y0c[2] = {0.0, 0.0};
  int32_t syc = 0;
  if (kRoll && autoreset) {
#pragma unroll
    for (int c = 0; c < 2; ++c)
      if (c < nc) y0c[c] = A.f64e(U_W0N + 8 * c, eo);
    if (exp2) syc = A.i32e(U_SYN, eo4);
  }
#ifdef SACENV_STAMPS
  // per-phase shader-clock sums over a launch's steps (tools/phase_stamps.py):
  // issue-progress clocks, no waits added; sched barriers pin the phase edges
  uint64_t ph[4] = {0, 0, 0, 0}, ph_t = 0;
#define PHASE(i)                                         \
  do {                                                   \
    __builtin_amdgcn_sched_barrier(0);                   \
    const uint64_t ph_now = __builtin_amdgcn_s_memtime(); \
    if ((i) > 0) ph[(i) - 1] += ph_now - ph_t;           \
    ph_t = ph_now;                                       \
    __builtin_amdgcn_sched_barrier(0);                   \
  } while (0)
#else
#define PHASE(i) \
  do {           \
  } while (0)
#endif
  // carried between the steps of a multi-step launch (updated at each step's
  // end, not recomputed): the knot coordinate of this step's grid index, and
  // the lane's ring byte offsets of its current and next episode slots
  // (wko_l(slot, 0, 0, lane)): ~25 integer VALU a step less
  Knot kcur = knot_coord(p, index > p.wind_len - 1 ? p.wind_len - 1 : index);
  const uint32_t slot_bytes = 2u * 16u * (uint32_t)A.nk, lane_ring = A.wko_l(0, 0, 0, lane);
  const int slot0 = cons % kSlots;
  int nslot = slot0 + 1 == kSlots ? 0 : slot0 + 1;
  uint32_t so = lane_ring + (uint32_t)slot0 * slot_bytes, sno = lane_ring + (uint32_t)nslot * slot_bytes;
  // staged replay rows: each lane's mark bits of every step of the launch (its env's
  // ceil(n_steps / 64) words, env-major), staged in LDS once (a per-step global load
  // would sit in the loop's vmcnt accounting, and the step's first full wait would
  // expose its ~1-us latency every step)
  if (kRoll && kRows == 2) {
    // the launch consumes its marks: each env's words are read by its lane alone and
    // cleared, so the staged replay's next draws into this buffer start from zero (no
    // fill kernel). No marks: every row, all bits set (the loop reads mk[(ks / 32) % 8]
    // with no per-step branch on the pointer)
    static_assert((kMkWords & (kMkWords - 1)) == 0, "l.mk is indexed (ks / 32) % kMkWords");
    if (ra->marks != nullptr) {
      const int W = (n_steps + 63) / 64;  // (n_steps <= 256 with marks: sacenv_boat_segment)
      unsigned long long* const w = ra->marks + (int64_t)e * W;
      for (int q = 0; q < W; ++q) {
        const unsigned long long m = w[q];
        w[q] = 0ull;
        l.mk[2 * q][lane] = (uint32_t)m;
        l.mk[2 * q + 1][lane] = (uint32_t)(m >> 32);
      }
    } else {
#pragma unroll
      for (int q = 0; q < kMkWords; ++q) l.mk[q][lane] = ~0u;
    }
    wave_lds_sync();
  }
  // the staged rows: the wave's rows through one buffer resource (env-major: lane's row
  // of step ks at s_lane + ks * 64 from the wave's first env's), the step's offset in
  // the scalar offset
  const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(
      (kRoll && kRows == 2) ? ra->stage + (int64_t)ob * kWave * n_steps * 64 : nullptr, 0, 0x7fffffff, 0x00020000);
  const uint32_t s_lane = (kRoll && kRows == 2) ? (uint32_t)lane * (uint32_t)n_steps * 64u : 0u;
  uint32_t mkw = 0u;
  // every load of the launch's prologue has landed before the step loop: the waitcnt
  // pass then sees no load pending at the loop's entry, and the loop keeps no wait
  // for them -- such a wait, on later steps, also waits for the previous step's
  // stores (vmcnt counts both on gfx950)
  if (kRoll) __builtin_amdgcn_s_waitcnt(0);
  for (int ks = 0; ks < (kRoll ? n_steps : 1) && (!kHand || !failed); ++ks) {
  PHASE(0);
  const float act = active ? act_cur : 0.0f;
  // the next step's action, a step ahead: open-loop rows at once; a handed-off
  // row if its flag already said so, else after this step's outputs (below)
  bool act_next = false;
  uint32_t flag_now = 0u;
  if (kRoll && ks + 1 < n_steps) {
    if (!kHand || !per_step) {  // open loop, or every row of the launch already published
      act_cur = *reinterpret_cast<const float*>(abase + (int64_t)(ks + 1) * arow);
      act_next = true;
    } else {
      if (seen >= ra->seq0 + (uint32_t)ks + 2u) {
        act_cur = act_load(abase, (uint32_t)((ks + 1) * arow));
        act_next = true;
      }
      flag_now = flag_issue(rdy);  // in flight during the step, read at its end
    }
  }
  const int wi = index > p.wind_len - 1 ? p.wind_len - 1 : index;
  Knot knext = kcur;
  double wv = 0.0, wa = 0.0;
  bool refresh = false, any_refresh = false;
  int jn = 0;
  double rq[kCoef];  // refreshed piece (refresh lanes), stored at the end
  // autoreset: the next pre-drawn episode's curve values at grid index 0 and
  // start y. Lanes in an episode's first step gather them from the slot ring
  // and refresh their lane-coalesced copies; the others read the copies. The
  // one-step launch: one unconditional load per value from a per-lane address
  // (no divergent branch: see the refresh loads below; no select between two
  // loaded registers either).
  double y0n[2];
  int32_t syn = 0;
  const bool hdr_refresh = autoreset && index == 0;
#pragma unroll
  for (int c = 0; c < 2; ++c) y0n[c] = y0c[c];
  if (kRoll) syn = syc;
  const auto hdr_gather = [&]() {
    const int ns = nslot;  // (cons + 1) % kSlots
#pragma unroll
    for (int c = 0; c < 2; ++c)
      if (c < nc) {
        // (rollout: the copy is in registers; other lanes read the ring's first line)
        const double v = *(hdr_refresh ? reinterpret_cast<const double*>(wbase + sno + (uint32_t)(c * A.nk) * 16u)
                                       : (kRoll ? A.wind_knots() : &A.f64e(U_W0N + 8 * c, eo)));
        y0n[c] = kRoll && !hdr_refresh ? y0c[c] : v;
      }
    if (nc == 0 && exp2) {
      const int32_t v = *(hdr_refresh ? &A.i32e(U_STARTY + 4 * ns, eo4) : &A.i32e(U_SYN, eo4));
      syn = kRoll && !hdr_refresh ? syc : v;
    }
  };
  if (nc == 0) {
    wind_at(p, A, T.table, 0, e, wi, wv, wa);  // constants or the shared table
  } else {
    const double tt = kcur.t;  // = knot_coord(p, wi).t
    const double c0 = spline_piece(cf[0], cf[2], cf[1], cf[3], tt);  // cf: y0 m0 y1 m1
    if (nc == 2) {  // exp 6 (the only two-curve experiment)
      wv = c0;
      wa = spline_piece(cf[4], cf[6], cf[5], cf[7], tt);
    } else if (p.experiment == 4) {
      wv = c0;
      wa = p.wind_dir_rad;
    } else {  // 5: rectified angle (wind.py:92-99)
      wv = p.max_velocity;
      wa = ((c0 <= 0.5 / 2 ? 0.0 : 1.0) * kPi) + kPi / 2;
    }
    const int wn = index + 1 > p.wind_len - 1 ? p.wind_len - 1 : index + 1;
    knext = knot_coord(p, wn);
    jn = knext.j;
    refresh = index == 0 || jn != kcur.j;
    // (one wave-uniform branch: in ~3 of 4 steps no lane of the wave refreshes. It is the
    // multi-step loop's one rare-event test at the head of the step: its region, laid
    // out behind the loop, holds the header gathers, behind a uniform test of their own
    // -- a lane in its episode's first step is a refresh lane --, and the piece gathers.
    // The hint is a probability, not "never": with the plain unlikely hint the
    // register allocator spent 2-4 VGPRs more in some instantiations)
    any_refresh = any_lane(refresh);
    if (__builtin_expect_with_probability(any_refresh, 0, 0.9)) {
      // (multi-step loop: the header copies are in registers, and only a step with a
      // lane in its episode's first step -- the step after a restart -- gathers)
      if (kRoll && any_lane(hdr_refresh)) hdr_gather();
      // the piece of the next step's interval for refreshing lanes, stored at
      // the end (own registers, read only there). Unconditional loads, the
      // other lanes reading one fixed line: with no branch around them the
      // waitcnt pass can count the loads in flight (a load under a divergent
      // branch made the first use of every earlier load wait for all of them)
#pragma unroll
      for (int c = 0; c < 2; ++c)
        if (c < nc) {
          double q[4];
          A.piece_at(wbase, refresh ? so + (uint32_t)(c * A.nk + jn) * 16u : 0u, q);
          rq[4 * c] = q[0], rq[4 * c + 1] = q[1], rq[4 * c + 2] = q[2], rq[4 * c + 3] = q[3];
        }
    }
  }
  // (the one-step launch: unconditional; no curve: no refresh region, and the one
  // header value, exp 2's start y, behind its own test)
  if (!kRoll || (nc == 0 && exp2 && __builtin_expect(any_lane(hdr_refresh), 0))) hdr_gather();
  OWNER_STAMP(st_loaded);
  const double r_mx = T.r_mx, r_my = T.r_my, r_iz = T.r_iz, r_nd = T.r_nd, r_w = T.r_w;

  // BoatEnv.step :69-73
  t = t_idx ? (double)(index + 1) * p.dt : t + p.dt;  // boat_env.py:69
  const int32_t fuel = p.fuel0 - (index + 1);
  // action / 10. div_c's correction step turns an infinite quotient into NaN,
  // fma(-inf, 10, inf), where IEEE division keeps it (boat_env.py:73: the rudder is
  // infinite and breaks): a non-finite action passes through instead, inf / 10 = inf
  // and NaN / 10 = NaN, behind a wave-uniform branch that is almost never taken
  if (p.test_mode == 0) {
    double moved = rudder + div_c((double)act, 10.0, 0.1);
    if (__builtin_expect(any_lane(!__builtin_isfinite(act)), 0)) {
      if (!__builtin_isfinite(act)) moved = rudder + (double)act;
    }
    rudder = moved;
  }
  if (!t_idx) EARLY_STORE(U_T, t);
  const bool first = index == 0;  // integrator counter == 0 (control_blocks.py:21-22)
  const double v_x_w = v_x * p.one_minus_wf;
  const double J = p.n_rpm != 0.0 ? div_c(v_x_w, p.n_times_d, r_nd) : 0.0;  // :222-224
  double sin_J, sin_rud, swa, cwa;
  trig3(J, rudder, wa, &sin_J, &sin_rud, &swa, &cwa, K);
  PHASE(1);

  // eom_longitudinal :213-239
  const double F_R = (v_x * v_x) * T.k_front;
  const double F_T = sin_J * T.k_thrust;
  const double F_C = v_y * p.m_plus_my * v_r;
  // v^2 sign(v) as v |v| (|.| is a free operand modifier): one multiply instead
  // of a square, two compares, a convert and a multiply; the same double for
  // every v != 0 (multiplying by +-1 is exact, in any position)
  const double w2s = wv * fabs(wv);
  const double F_W = (w2s * T.k_front) * cwa;
  const double a_x = div_c(-F_R + F_T + F_C + F_W, p.m_plus_mx, r_mx);
  v_x = first ? 3.0 : a_x * p.dt + v_x;

  // eom_transverse :241-265 (new v_x)
  const double F_R2 = (v_y * fabs(v_y)) * T.k_side;
  const double vx2 = v_x * v_x;  // (the new v_x)
  const double F_RU = sin_rud * (vx2 * T.k_rud_front);
  const double F_C2 = v_x * p.m_plus_mx * v_r;
  const double F_W2 = (w2s * T.k_side) * swa;
  const double a_y = div_c(-F_R2 + F_RU + F_C2 + F_W2, p.m_plus_my, r_my);
  v_y = first ? 0.0 : a_y * p.dt + v_y;

  // eom_yawning :267-281
  const double M_hull = (v_r * fabs(v_r)) * T.k_hull;
  const double M_rud = ((v_x * fabs(v_x)) * T.k_rud_moment) * sin_rud;
  const double a_r = div_c(-M_hull + M_rud, p.i_plus_iz, r_iz);
  v_r = first ? 0.0 : a_r * p.dt + v_r;
  EARLY_STORE2(U_VY, v_y, v_r);

  // get_kinematics :283-306
  // drift = atan2(v_x, v_y) has sin = v_x / v, cos = v_y / v, so
  // sin(drift - s_r) v = v_x cos s_r - v_y sin s_r and
  // cos(drift - s_r) v = v_y cos s_r + v_x sin s_r: no atan2, sqrt or division
  // (122 fewer VALU; -0.26 us/step). Same parity class as the ocml/libm
  // differences: the increments agree to a few ulp of v dt.
  s_r = v_r * p.dt + s_r;
  double ssr, csr;
  sincos_cw(s_r, &ssr, &csr, K);
  s_x = (v_x * csr - v_y * ssr) * p.dt + s_x;
  s_y = (v_y * csr + v_x * ssr) * p.dt + s_y;
  index = index + 1;
  EARLY_STORE2(U_SX, s_x, s_y);
  EARLY_STORE2(U_SR, s_r, v_x);
  if (!kRoll) st_out(A.i32e(U_IDX, eo4), index);
  PHASE(2);

  Obs o = make_obs(p, oc, s_x, v_x, a_x, s_y, v_y, a_y, s_r, v_r, a_r, rudder, (double)fuel);

  // exponential_reward (reward_functions.py:42-57), f_x = 0
  const double ay = fabs(s_y);
  const double f_y = div_c(ay, p.track_width, r_w) / (1.0 + exp_v(p.reward_k * (ay - p.reward_center), K));
  double reward = 0.0 - f_y;

  // termination chain :84-105 (the first true condition wins), as selects: as an
  // if/else-if chain it compiled to nested exec-mask branches (~25 SALU a step)
  const bool goal = s_x >= p.goal_line;
  int tm = (rudder > kPi / 3) | (rudder < -kPi / 3) ? SACENV_TERM_RUDDER_BROKEN : SACENV_TERM_NONE;
  tm = p.t_max <= t ? SACENV_TERM_TIMEOUT : tm;
  tm = fuel < 0 ? SACENV_TERM_OUT_OF_FUEL : tm;
  tm = (fabs(s_y) > p.oob_limit) | (s_x < 0.0) ? SACENV_TERM_OUT_OF_BOUNDS : tm;
  tm = goal ? SACENV_TERM_REACHED_GOAL : tm;
  reward = goal ? reward + 1000.0 : reward;
  // penalties :107-111
  reward = ((rudder > kPi / 4) | (rudder < -kPi / 4)) ? reward - fabs(rudder) * 100.0 : reward;
  reward = fabs(s_r) > kPi / 2 ? reward - 1.0 : reward;
  ep = ep + reward;
  uint8_t term = active ? (uint8_t)tm : (uint8_t)SACENV_TERM_NONE;  // padding lanes never end

  // (the multi-step loop counts in its episode-end region, below)
  if (!kRoll && term != SACENV_TERM_NONE)  // no-return atomic: nothing on the critical path waits
    __hip_atomic_fetch_add(&A.at_e<uint32_t>(U_CNT + 4 * (term - 1), eo4), 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
  if (term == SACENV_TERM_NONE && active && p.max_episode_steps > 0 && index >= p.max_episode_steps)
    term = SACENV_TERM_TRUNCATED;
  lt = (uint32_t)term - 1u < 5u ? (uint32_t)term : lt;  // codes 1..5 overwrite it, 0 and 6 keep it
  const bool ended = term != SACENV_TERM_NONE;
  PHASE(3);

  OWNER_STAMP(st_computed);
  // this step's outputs: the arena's record, or the multi-step launch's
  // (kLean: both strides are 0, the addresses loop invariants)
  char* const R = kLean ? ra->rec : kRoll ? ra->rec + (int64_t)ks * ra->rec_stride : A.b + A.ur() * A.np;
  float* const fin = kLean   ? ra->fin
                     : kRoll ? (ra->fin != nullptr ? ra->fin + (int64_t)ks * ra->fin_stride : nullptr)
                             : A.final_obs();
  // (kRoll: kRows compiles the pooled row in or out; the step launch decides at run time)
  char* const trans = kRows != 1 ? nullptr
                              : kRoll ? (ra->trans != nullptr ? ra->trans + (int64_t)ks * ra->trans_stride : nullptr)
                                      : trans1;
  if (out_flags & SACENV_OUT_REWARD64) A.at_e<double>(A.ur() + R_REWARD64, eo) = reward;
  if (out_flags & SACENV_OUT_ACCEL) {
    A.at_e<double>(A.ur() + R_AX, eo) = a_x;
    A.at_e<double>(A.ur() + R_AY, eo) = a_y;
    A.at_e<double>(A.ur() + R_AR, eo) = a_r;
  }
  const bool restart = ended && autoreset;
  // terminal obs of the envs that auto-reset (main.py:72 reset, boat_env.py:121):
  // per-lane stores (measured 0.13 us/step cheaper than a 2.8-KB block store per
  // restarting wave with two extra barriers)
  if (!kRoll) {  // (the multi-step loop: in its episode-end region, below)
    if (ended) A.at_e<double>(A.ur() + R_FIN_EP, eo) = ep;
    if (restart && fin != nullptr) store_obs(fin + (int64_t)e * SACENV_OBS_DIM, o);
  }
  int cons_out = cons;
  // the record's obs row: this step's obs, or a restarting lane's first obs of
  // its next episode. The restart's ~45 per-lane selects (state, row, slot ring)
  // sit behind ONE wave-uniform branch: in most steps no lane of the wave ends
  // its episode (an episode runs up to 500 steps), and the selects are skipped.
  // the staged replay row of this step (sacenv_replay_sample_staged reads it), only
  // where a learn of this or the next segment samples it or its successor: one 64-B
  // line per row, s' (the pre-reset obs), reward, action, term | lt << 8, obs3_next
  // (written by a restarting lane below); stored before the restart selects, so the
  // pre-reset obs need not stay live across them
  bool staged = false;
  if (kRoll && kRows == 2) {
    // the lane's mark bits, one LDS read per 32 steps (a per-step read waited its
    // latency right before the test), consumed bit by bit
    if ((ks & 31) == 0) mkw = l.mk[(ks >> 5) & (kMkWords - 1)][lane];  // (n_steps <= 256 with marks)
    staged = (mkw & 1u) != 0u;
    mkw >>= 1;
    if (staged) {  // (write-through, as the record's stores: measured +70 us per launch here)
      const uint32_t so = (uint32_t)ks * 64u;
      __builtin_amdgcn_raw_buffer_store_b128(
          u4v{__float_as_uint(o.v[0]), __float_as_uint(o.v[1]), __float_as_uint(o.v[2]), __float_as_uint(o.v[3])},
          srs, s_lane, so, 0);
      __builtin_amdgcn_raw_buffer_store_b128(
          u4v{__float_as_uint(o.v[4]), __float_as_uint(o.v[5]), __float_as_uint(o.v[6]), __float_as_uint(o.v[7])},
          srs, s_lane + 16u, so, 0);
      __builtin_amdgcn_raw_buffer_store_b128(
          u4v{__float_as_uint(o.v[8]), __float_as_uint(o.v[9]), __float_as_uint(o.v[10]), __float_as_uint((float)reward)},
          srs, s_lane + 32u, so, 0);
      __builtin_amdgcn_raw_buffer_store_b128(u4v{__float_as_uint(act), (uint32_t)term | (lt << 8), 0u, 0u}, srs,
                                             s_lane + 48u, so, 0);
    }
  }
  float row[SACENV_OBS_DIM];
#pragma unroll
  for (int k = 0; k < SACENV_OBS_DIM; ++k) row[k] = o.v[k];
  float row3_new = 0.0f;  // (exp 2's pooled row: the new episode's obs[3])
  // The multi-step loop's episode-end region: everything a step does only for
  // lanes whose episode ended (the termination counter, ep_reward, the terminal
  // obs, the restart) behind ONE wave-uniform branch, the per-lane predicates
  // inside it. In ~3 of 4 steps no lane of the wave ends, and the step falls
  // through. (After the staged row's stores: a restarting lane's obs3_next
  // lands in the row just stored, and the later store wins.)
  // (the one-step launch: the restart's selects behind its own uniform branch, as before)
  if (kRoll ? __builtin_expect(any_lane(ended), 0) : __ballot(restart) != 0ull) {
    if (kRoll) {
      if ((uint32_t)term - 1u < 5u)  // codes 1..5 (no-return atomic: nothing waits for it)
        __hip_atomic_fetch_add(&A.at_e<uint32_t>(U_CNT + 4 * (term - 1), eo4), 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
      if (ended) A.at_e<double>(A.ur() + R_FIN_EP, eo) = ep;
      if (restart && fin != nullptr) store_obs(fin + (int64_t)e * SACENV_OBS_DIM, o);
    }
    if (restart) {  // next episode from its pre-drawn slot: a fresh Boat (boat_env.py:152-198)
      const double sy0 = exp2 ? (double)syn : 0.0;  // :166-169
      s_x = 0.0, s_y = sy0, s_r = 0.0, v_x = 0.0, v_y = 0.0, v_r = 0.0, rudder = 0.0;
      t = 0.0, ep = 0.0;  // :122
      index = 0;
      Obs fo;
      if (exp2 || no_fuel) {
        fo = make_obs(p, oc, 0.0, 0.0, 0.0, sy0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, (double)p.fuel0);
      } else {  // make_obs of the zero state, folded: (0+W)/(2W) = 0.5 and fuel0/fuel0 = 1 exactly
        constexpr float kRud0 = (float)((0.0 + kPi / 3) * (1.0 / (kPi / 3 - (-kPi / 3))));
#pragma unroll
        for (int k = 0; k < SACENV_OBS_DIM; ++k) fo.v[k] = 0.0f;
        fo.v[3] = 0.5f;
        fo.v[9] = kRud0;
        fo.v[10] = 1.0f;
      }
#pragma unroll
      for (int k = 0; k < SACENV_OBS_DIM; ++k) row[k] = fo.v[k];
      row3_new = fo.v[3];
      if (kRoll && kRows == 2 && exp2 && staged)  // the staged row's obs3_next
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(row3_new), srs, s_lane + 56u, (uint32_t)ks * 64u, 0);
      cons_out = cons + 1;
      if (kRoll) {  // the next slot becomes current; grid index 0 (registers: no store)
#pragma unroll
        for (int c = 0; c < 2; ++c)
          if (c < nc) cf[4 * c] = y0n[c];
        so = sno;
        nslot = nslot + 1 == kSlots ? 0 : nslot + 1;
        sno = nslot == 0 ? lane_ring : sno + slot_bytes;
        knext = knot_coord(p, 0);
      }
    }
  }
  // the dynamics' fields went out as they were computed; what is left: the
  // fresh state of restarting envs (same lane, same address: the later store
  // wins), ep_reward, the next wind, and the record
  if (!kRoll && restart) {
    EARLY_STORE2(U_SX, s_x, s_y);
    EARLY_STORE2(U_SR, s_r, v_x);
    EARLY_STORE2(U_VY, v_y, v_r);
    if (!t_idx) st_out(A.f64e(U_T, eo), t);
    st_out(A.i32e(U_IDX, eo4), index);
    st_out(A.i32e(U_CONS, eo4), cons_out);
  }
  if (!kRoll) {
    st_out(A.i32e(U_LTERM, eo4), (int32_t)lt);
    EARLY_STORE2(U_RUD, rudder, ep);
    if (restart && nc > 0) {  // the new episode's first wind: the piece's y0 = y(0); at
      // t = 0 the piece is exactly y0 whatever (finite) m0, y1, m1 it still holds
#pragma unroll
      for (int c = 0; c < 2; ++c)
        if (c < nc) st_out(A.f64e(U_COEF + 32 * c, eo), y0n[c]);
    } else if (refresh) {
#pragma unroll
      for (int k = 0; k < kCoef; k += 2)
        if (k < 4 * nc) EARLY_STORE2(U_COEF + 8 * k, rq[k], rq[k + 1]);
    }
    if (hdr_refresh) {
#pragma unroll
      for (int c = 0; c < 2; ++c)
        if (c < nc) st_out(A.f64e(U_W0N + 8 * c, eo), y0n[c]);
      if (exp2) st_out(A.i32e(U_SYN, eo4), syn);
    }
  } else {  // the same updates, in registers (each behind a wave-uniform branch)
    // (the saved result of the step's head test: a cold block behind the loop with its
    // register copies, no exec-mask skip on the fall-through path. One owner wave per
    // SIMD only: with the hint a two-waves-per-SIMD instantiation, exp 4/5's staged
    // rows, allocates a 20-B private segment it never touches)
    if (nc > 0 && (kVc ? __builtin_expect(any_refresh, 0) : any_refresh)) {
      if (refresh && !restart) {
#pragma unroll
        for (int k = 0; k < kCoef; ++k) cf[k] = rq[k];
      }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) y0c[c] = y0n[c];
    syc = syn;
    cons = cons_out;
    kcur = knext;  // (a restarting lane's: grid index 0, set in the episode-end region)
  }
  if (kRows == 3) {  // (fresh rows: streaming stores, as the obs row below)
    __builtin_nontemporal_store((float)reward, reinterpret_cast<float*>(R + R_REWARD * A.np + eo4));
    __builtin_nontemporal_store((uint8_t)(ended ? 1 : 0), reinterpret_cast<uint8_t*>(R + R_DONE * A.np + e));
    __builtin_nontemporal_store(term, reinterpret_cast<uint8_t*>(R + R_TERM * A.np + e));
  } else {
    st_out<kWT>(*reinterpret_cast<float*>(R + R_REWARD * A.np + eo4), (float)reward);
    st_out<kWT>(*reinterpret_cast<uint8_t*>(R + R_DONE * A.np + e), (uint8_t)(ended ? 1 : 0));
    st_out<kWT>(*reinterpret_cast<uint8_t*>(R + R_TERM * A.np + e), term);
  }
  // a restarting env's row is its new episode's first obs
  if (!kWT) {
    // write-back record (open-loop multi-step launch): each lane stores its own
    // 44-B row as 16 + 16 + 12 B (4-B aligned vector stores): 0.08 us/step
    // cheaper than the LDS-staged block below, whose LDS round trip and waits
    // sit on the step's path
    if (kRows == 3)  // every step's record to fresh rows (sacenv_boat_rollout): streaming stores
      store_row_nt<SACENV_OBS_DIM>(reinterpret_cast<float*>(R) + (int64_t)e * SACENV_OBS_DIM, row);
    else
      store_row<SACENV_OBS_DIM>(reinterpret_cast<float*>(R) + (int64_t)e * SACENV_OBS_DIM, row);
  } else {
    // obs rows through LDS, stored as write-through float4 (64 rows x 44 B = 176 float4)
#pragma unroll
    for (int k = 0; k < SACENV_OBS_DIM; ++k) l.obs[lane * SACENV_OBS_DIM + k] = row[k];
    wave_lds_sync();  // the rows are this wave's own LDS: no workgroup barrier
    const int64_t row0 = (int64_t)ob * kWave * SACENV_OBS_DIM;
    store_obs_block<SACENV_OBS_DIM, kWT>(l.obs, reinterpret_cast<float*>(R) + row0, lane);
    if (kRoll) {  // l.obs is rewritten by the next step
      wave_lds_sync();
    }
  }
  if (trans != nullptr) {  // the pooled transition row (sacenv_boat_step_pooled)
    // s' entries 0..8 = the pre-reset obs (entries 9 and 10, rudder and fuel, follow
    // on the receivers from the actions and the episode starts), reward, action,
    // term (done = term != 0) and, in experiment 2, the new episode's obs[3]
    if (!kWT) {  // per-lane rows, as the record's
      store_row<SACENV_TRANS_OBS>(reinterpret_cast<float*>(trans) + (int64_t)e * SACENV_TRANS_OBS, o.v);
    } else {
      wave_lds_sync();
#pragma unroll
      for (int k = 0; k < SACENV_TRANS_OBS; ++k) l.obs[lane * SACENV_TRANS_OBS + k] = o.v[k];
      wave_lds_sync();
      store_obs_block<SACENV_TRANS_OBS, kWT>(
          l.obs, reinterpret_cast<float*>(trans) + (int64_t)ob * kWave * SACENV_TRANS_OBS, lane);
    }
    constexpr int kOff = 4 * SACENV_TRANS_OBS;  // byte columns (x n_pad) after s'
    st_out<kWT>(*reinterpret_cast<float*>(trans + kOff * A.np + eo4), (float)reward);
    st_out<kWT>(*reinterpret_cast<float*>(trans + (kOff + 4) * A.np + eo4), act);
    st_out<kWT>(*reinterpret_cast<uint8_t*>(trans + (kOff + 8) * A.np + e), term);
    if (pin.experiment == 2)
      st_out<kWT>(*reinterpret_cast<float*>(trans + (kOff + 9) * A.np + eo4), row3_new);
    if (kRoll && kWT) {  // l.obs is rewritten by the next step
      wave_lds_sync();
    }
  }
  if (kHand && ra->done != nullptr) {
    // step ks's outputs visible device-wide (release: L2 write-back + wait for
    // the stores), then its done flag, write-through
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (lane == 0)
      __hip_atomic_store(ra->done + ob, ra->seq0 + (uint32_t)ks + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (kHand && per_step && ks + 1 < n_steps) {
    const uint32_t fv = flag_value(flag_now);
    seen = fv > seen ? fv : seen;
    failed = seen == SACENV_FLAG_ABORT;  // the producer gave up: so does this wave
    if (!act_next && !failed) {  // closed loop: the next action comes after these outputs
      seen = wait_flag(rdy, ra->seq0 + (uint32_t)ks + 2u, seen, ra->status, lane);
      failed = seen == 0u || seen == SACENV_FLAG_ABORT;
      act_cur = act_load(abase, (uint32_t)((ks + 1) * arow));
    }
  }
  PHASE(4);
  }  // steps
  if (kHand && failed && ra->done != nullptr && lane == 0)  // waiters on this wave must not hang
    __hip_atomic_store(ra->done + ob, SACENV_FLAG_ABORT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (kRoll) {  // the carried state, once
    A.f64e(U_SX, eo) = s_x, A.f64e(U_SY, eo) = s_y, A.f64e(U_SR, eo) = s_r;
    A.f64e(U_VX, eo) = v_x, A.f64e(U_VY, eo) = v_y, A.f64e(U_VR, eo) = v_r;
    A.f64e(U_RUD, eo) = rudder;
    if (!t_idx) A.f64e(U_T, eo) = t;
    A.f64e(U_EP, eo) = ep;
    A.i32e(U_IDX, eo4) = index;
    A.i32e(U_LTERM, eo4) = (int32_t)lt;
    if (autoreset) A.i32e(U_CONS, eo4) = cons;
#pragma unroll
    for (int k = 0; k < kCoef; ++k)
      if (k < 4 * nc) A.f64e(U_COEF + 8 * k, eo) = cf[k];
    if (autoreset) {
#pragma unroll
      for (int c = 0; c < 2; ++c)
        if (c < nc) A.f64e(U_W0N + 8 * c, eo) = y0c[c];
      if (exp2) A.i32e(U_SYN, eo4) = syc;
    }
  }

#ifdef SACENV_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (kRoll && lane == 0) {  // phase sums (shader clocks) of this launch
    double* d = A.accel() + (int64_t)ob * 8;
    for (int i = 0; i < 4; ++i) d[i] = (double)ph[i];
    d[4] = (double)n_steps;
  } else if (lane == 0) {
    double* d = A.accel() + (int64_t)ob * 4;
    d[0] = (double)st_real0;
    d[1] = (double)__builtin_amdgcn_s_memrealtime();
    d[2] = (double)st_loaded;
    d[3] = (double)st_computed;
  }
#endif
}

// n_steps BoatEnv.step launches fused, the state in registers between the
// steps: open-loop rollouts (records per step) and the segment
// launch (the arena's record every step, actions behind per-wave flags)
//
// kVc: the fp64 constants as VGPR copies (one owner wave per SIMD: k_rollout), or
// as literals and scalar registers (k_rollout_dense: 238 VGPRs, two owner waves
// per SIMD, for grids with more owner waves than SIMDs -- 131 072 envs: 48.5
// against 44.4 G env-steps/s; at one wave per SIMD the copies win, 1.34 against
// 2.04 us per step). The same arithmetic either way: results are bit-identical.
// kLean: the open loop with the launch's options compiled in (owner_wave); the
// hand-off loop stays general.
template <int kNc, bool kTIdx, int kRows, bool kVc, bool kLean>
__device__ __forceinline__ void rollout_body(const SacenvBoatParams& p, const Arena& A, const Tail& T,
                                             const float* __restrict__ action, int n_steps, const RollArgs& ra,
                                             OwnerLds& slds) {
  const int ob = blockIdx.x, lane = threadIdx.x;
  uint32_t seen = 0u;
  bool hand = ra.done != nullptr;
  if (ra.ready != nullptr || ra.done != nullptr) {
    // abort protocol (sacenv.h): after a hand-off timeout anywhere, a hand-off
    // launch steps nothing; a producer that gave up published SACENV_FLAG_ABORT
    const uint32_t* rdy = ra.ready != nullptr ? ra.ready + ob : nullptr;
    const uint32_t st = flag_issue(reinterpret_cast<const uint32_t*>(ra.status));
    const uint32_t f0 = rdy != nullptr ? flag_issue(rdy) : 0u;
    bool stop = (flag_value(st) & SACENV_STATUS_HANDOFF_TIMEOUT) != 0u;
    if (!stop && rdy != nullptr) {
      seen = wait_flag(rdy, ra.seq0 + 1u, flag_value(f0), ra.status, lane);
      stop = seen == 0u || seen == SACENV_FLAG_ABORT;  // row 0 never came: nothing steps
    }
    if (stop) {
      if (ra.done != nullptr && lane == 0)  // waiters on this wave must not hang either
        __hip_atomic_store(ra.done + ob, SACENV_FLAG_ABORT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
  }
  if (ra.ready != nullptr) {
    // the rows the flag covers were written before it (the producer's release):
    // drop any stale copy of them from this XCD's L2 once, then read them plainly;
    // rows published only later are read device-coherently, step by step
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    hand = hand || seen < ra.seq0 + (uint32_t)n_steps;
  }
  if (hand) {
    if (kVc)
      owner_wave<true, kNc, kTIdx, true, kRows, true>(vreg_params(p), A, vreg_tail(T), action, slds, ob, lane,
                                                       n_steps, &ra, nullptr, seen);
    else
      owner_wave<true, kNc, kTIdx, true, kRows, false>(p, A, T, action, slds, ob, lane, n_steps, &ra, nullptr, seen);
  } else {
    if (kVc)
      owner_wave<true, kNc, kTIdx, false, kRows, true, kLean>(vreg_params(p), A, vreg_tail(T), action, slds, ob,
                                                               lane, n_steps, &ra);
    else
      owner_wave<true, kNc, kTIdx, false, kRows, false, kLean>(p, A, T, action, slds, ob, lane, n_steps, &ra);
  }
}

}  // namespace
