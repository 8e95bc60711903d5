// sacenv_boat.hip — gfx950 kernels + C ABI for the vectorised boat env.
//
// The step launch (k_step) runs owner waves only: one lane per env, 64
// consecutive envs per wave, BoatEnv.step (boat_env.py:67-115) on float64
// SoA state. In autoreset mode an env that ends (terminated or truncated)
// starts its next episode at once from a PRE-DRAWN slot (SLOTS = 257 per env:
// the active episode + 256 ahead), so no RNG or spline work ever sits on the
// step's path, and the step keeps no refill bookkeeping beyond the episode
// counter `cons`.
// The refill launches (at least every 256 steps): k_need_masks marks the envs
// whose ring is short (fill < cons + SLOTS); k_refill ranks them from those
// masks (DPP scans, no atomics) and, one wave per env, draws
// the replacement episodes from the env's own numpy-legacy MT19937 stream
// (Boat.__init__ boat_env.py:144-201: randint, then the wind knots,
// wind.py:69-90), fits the not-a-knot spline, finds its exact grid-sample
// min/max from the critical points (instead of the reference's 10 000-sample
// scan, wind.py:80-89) and k_refill_fit stores the renormalised, scaled curve
// (wind.py:86-99). Kept out of the step launch, this work no longer shares
// SIMDs with the owners (measured: in-step helper waves cost 1.6 us/step).
//
// Floating-point order follows the reference expression by expression
// (left-to-right products, no FMA contraction: -ffp-contract=off); the only
// differences from the CPU step are the libm/ocml transcendentals.
//
// Here: the kernels, the host side and the C ABI. The device code they call is
// in the headers below, one per topic; none holds a kernel or an entry point.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sacenv.h"
#include "sacenv_boat_arena.h"  // units, layout, Arena, Tail, the host/device rules
#include "sacenv_boat_math.h"   // exp / sin / cos by hand, div_c, the observation
#include "sacenv_boat_wind.h"   // the spline piece, DPP helpers, grid extrema, the group fit
#include "sacenv_boat_draw.h"   // MT19937 episode draws, the wave fit, the twist ahead
#include "sacenv_toys.h"        // the toy envs
#include "sacenv_boat_owner.h"  // owner_wave and what it stores through

#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------- kernels

__global__ void k_spline_g(SacenvBoatParams p, double* __restrict__ g) {
  // (m/6) = G @ y for the not-a-knot cubic on uniform knots (knot coordinate):
  // rows 1..n-2: m[j-1] + 4 m[j] + m[j+1] = 6 (y[j-1] - 2 y[j] + y[j+1]);
  // rows 0, n-1: m[0] - 2 m[1] + m[2] = 0, m[n-3] - 2 m[n-2] + m[n-1] = 0.
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int n = p.n_knots;
  double a[kMaxK][kMaxK], r[kMaxK][kMaxK];
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) a[i][j] = r[i][j] = 0.0;
  a[0][0] = 1.0, a[0][1] = -2.0, a[0][2] = 1.0;
  a[n - 1][n - 3] = 1.0, a[n - 1][n - 2] = -2.0, a[n - 1][n - 1] = 1.0;
  for (int j = 1; j < n - 1; ++j) {
    a[j][j - 1] = 1.0, a[j][j] = 4.0, a[j][j + 1] = 1.0;
    r[j][j - 1] = 1.0, r[j][j] = -2.0, r[j][j + 1] = 1.0;  // (6 * rhs) / 6
  }
  for (int c = 0; c < n; ++c) {  // Gauss-Jordan, partial pivoting
    int piv = c;
    for (int i = c + 1; i < n; ++i)
      if (fabs(a[i][c]) > fabs(a[piv][c])) piv = i;
    for (int j = 0; j < n; ++j) {
      double t = a[c][j]; a[c][j] = a[piv][j]; a[piv][j] = t;
      t = r[c][j]; r[c][j] = r[piv][j]; r[piv][j] = t;
    }
    const double d = a[c][c];
    for (int j = 0; j < n; ++j) a[c][j] /= d, r[c][j] /= d;
    for (int i = 0; i < n; ++i) {
      if (i == c) continue;
      const double f = a[i][c];
      if (f == 0.0) continue;
      for (int j = 0; j < n; ++j) a[i][j] -= f * a[c][j], r[i][j] -= f * r[c][j];
    }
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) g[i * n + j] = r[i][j];
}

constexpr int kMaskThreads = 1024;

__global__ void __launch_bounds__(kWave) k_seed(SacenvBoatParams p, Arena A, const uint32_t* __restrict__ seeds) {
  const int e = blockIdx.x * kWave + threadIdx.x;
  // k_need_masks' look-back words (refill_mask): no stale epoch may match (the
  // caller's arena need not be zeroed; k_need_masks' workgroups <= owner waves <= envs)
  if (e < A.nwaves()) A.refill_mask()[e] = 0ull;
  if (e >= p.n_envs) return;
  // mt19937_seed (init_genrand), numpy RandomState._legacy_seeding(int)
  uint32_t x = seeds[e];
  uint32_t* key = A.mt_key() + (int64_t)e * kMtN;
  for (int i = 0; i < kMtN; ++i) {
    key[i] = x;
    x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)(i + 1);
  }
  A.i32(U_MTPOS)[e] = kMtN;  // (plain: mt_next not twisted yet)
  A.i32(U_CONS)[e] = 0;
  A.i32(U_FILL)[e] = 0;
}

// mode 0: first Boat (init). autoreset: slots 0..SLOTS-1 <- episodes 0..SLOTS-1.
// mode 1: reset listed envs. non-autoreset: slot 0 <- a new draw;
//         autoreset: start the next pre-drawn slot, then refill the freed one.
// mode 2: explicit draws (non-autoreset), slot 0.
// One Boat per listed env. ids == NULL: env = block index. dev_count != NULL:
// the list length is read on the device (ids[0 .. *dev_count), grid-stride),
// so a reset of the envs sacenv_compact_done found needs no host round trip.
__global__ void __launch_bounds__(kWave) k_draw(SacenvBoatParams p, Arena A, Tail T, int mode,
                                                const int32_t* __restrict__ ids,
                                                const int32_t* __restrict__ ex_start_y,
                                                const double* __restrict__ ex_knots,
                                                const int32_t* __restrict__ dev_count) {
  __shared__ DrawLds lds;
  const int lane = threadIdx.x;
  const int nq = dev_count != nullptr ? *dev_count : (int)gridDim.x;
  if ((int)blockIdx.x >= nq) return;
  load_g(p, T.g, lds, lane);
  for (int q = blockIdx.x; q < nq; q += gridDim.x) {
    const int e = ids != nullptr ? ids[q] : q;
    if (e < 0 || e >= p.n_envs) continue;  // uniform per block
    int32_t start_y;
    int slot = 0;
    if (mode == 2) {
      start_y = draw_episode_wave(p, A, lds, e, 0, lane, ex_start_y + q,
                                  ex_knots != nullptr ? ex_knots + (int64_t)q * 2 * p.n_knots : nullptr);
    } else if (!p.autoreset) {
      start_y = draw_episode_wave(p, A, lds, e, 0, lane, nullptr, nullptr);
    } else if (mode == 0) {
      // the first episode here; sacenv_boat_init's refill draws the next SLOTS-1 in
      // the env's order (all envs in parallel, the fits spread over lane groups:
      // seconds faster at 65 536 envs than SLOTS serial draw-and-fits per wave)
      start_y = draw_episode_wave(p, A, lds, e, 0, lane, nullptr, nullptr);
      if (lane == 0) {
        A.i32(U_CONS)[e] = 0;
        A.i32(U_FILL)[e] = 1;
      }
    } else {
      // start the next pre-drawn episode and draw one more behind the last
      // (per-env draw order: the refill continues from fill)
      const int c = A.i32(U_CONS)[e] + 1;
      const int f = A.i32(U_FILL)[e];
      if (c >= f && lane == 0) atomicOr(&A.status()[1], SACENV_STATUS_SLOT_UNDERFLOW);
      slot = c % kSlots;
      start_y = A.i32(U_STARTY)[(int64_t)slot * A.np + e];
      if (lane == 0) A.i32(U_CONS)[e] = c;
      draw_episode_wave(p, A, lds, e, f % kSlots, lane, nullptr, nullptr);
      if (lane == 0) A.i32(U_FILL)[e] = f + 1;
    }
    if (lane == 0) {
      const Obs o = fresh_state(p, A, T, e, start_y, slot);
      store_obs(A.obs() + (int64_t)e * SACENV_OBS_DIM, o);
    }
    __syncthreads();
  }
}

// Done-mask compaction (the reset list of BoatEnv.reset for the envs that
// ended): ids of the nonzero bytes of done[0..n), ascending,
// and their count. One workgroup of 1024 lanes, 64 bytes per lane per pass:
// per-lane counts -> DPP wave scan -> LDS scan of the 16 wave totals.
__global__ void __launch_bounds__(1024) k_compact(const uint8_t* __restrict__ done, int n, int aligned,
                                                  int32_t* __restrict__ ids, int32_t* __restrict__ count) {
  __shared__ int wsum[16];
  __shared__ int base_s;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (t == 0) base_s = 0;
  __syncthreads();
  for (int64_t c0 = 0; c0 < n; c0 += 1024 * 64) {
    const int64_t e0 = c0 + (int64_t)t * 64;
    uint64_t bits = 0;  // bit j: done[e0 + j] != 0
    if (aligned && e0 + 64 <= n) {
      const uint4* v = reinterpret_cast<const uint4*>(done + e0);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint4 x = v[k];
        const uint32_t wds[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
          for (int by = 0; by < 4; ++by)
            if ((wds[d] >> (8 * by)) & 0xffu) bits |= 1ull << (16 * k + 4 * d + by);
      }
    } else {
      for (int j = 0; j < 64 && e0 + j < n; ++j)
        if (done[e0 + j]) bits |= 1ull << j;
    }
    const int cnt = __popcll(bits);
    const int incl = wave_incl_scan(cnt);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int wbase = 0;
    for (int k = 0; k < w; ++k) wbase += wsum[k];
    int pos = base_s + wbase + incl - cnt;
    while (bits) {
      const int j = __ffsll((long long)bits) - 1;
      bits &= bits - 1ull;
      ids[pos++] = (int32_t)(e0 + j);
    }
    __syncthreads();
    if (t == 1023) base_s += wbase + incl;
    __syncthreads();
  }
  if (t == 0) *count = base_s;
}

// Non-serialising phase clocks of the refill (tools/refill_stamps.py; -DSACENV_STAMPS
// builds only): a stamp is taken once the value(s) it names are in registers
// (the empty asm consumes them), no other wait is added.
#ifdef SACENV_STAMPS
#define REFILL_STAMP(slot, ...)                                     \
  do {                                                              \
    asm volatile("" ::__VA_ARGS__);                                 \
    (slot) = __builtin_amdgcn_s_memrealtime();                      \
  } while (0)
constexpr int kRefillStamps = 24;  // per refill wave: start, total read, fast path done, 19 wave draws, end, draws
#else
#define REFILL_STAMP(slot, ...) \
  do {                          \
  } while (0)
#endif

// sacenv_boat_refill, launch 1: every listed env gets its slot ring topped up
// to SLOTS episodes (fill = cons + SLOTS), drawn in the env's order (start y
// and raw knots). A wave takes four consecutive ranks, one 16-lane group each.
// Fast path, one episode per group: the group loads the 16 + 2*nk*curves words
// at the env's MT position (when they lie inside the current 624-word block),
// tempers them, takes the first accepted randint word among the first 16
// (masked rejection, numpy legacy) and turns the following word pairs into the
// knots (genrand_res53), lane = (curve, knot): one wave instruction serves four
// envs, where the wave-per-env draw spent ~330 wave instructions on each (the
// refill was VALU-bound). A window that crosses the block end reads on in
// mt_next when the last fit launch twisted it ahead (kMtNextOk). The rest --
// a crossing without mt_next (a second one since the last refill), a randint
// rejected 16 times, more than 8 knots -- goes through the wave-per-env draw
// (draw_knots_wave), env by env. Block 0 counts the refill.
constexpr int kGroupLanes = 16;
constexpr int kGroups = kWave / kGroupLanes;
__global__ void __launch_bounds__(kWave) k_refill(SacenvBoatParams p, Arena A) {
  __shared__ RngLds lds;
  const int lane = threadIdx.x;
#ifdef SACENV_STAMPS
  uint64_t stm[kRefillStamps] = {};
  int n_st = 0;
#endif
  REFILL_STAMP(stm[0], "s"(lane));
  const int total = __builtin_amdgcn_readfirstlane(A.status()[2]);  // listed by k_need_masks
  REFILL_STAMP(stm[1], "s"(total));
  if (blockIdx.x == 0 && lane == 0) A.status()[0] += 1;
  const int G = (int)gridDim.x;
  const int g = lane / kGroupLanes, gl = lane % kGroupLanes;
  const int nk = p.n_knots;
  const int ndraw = n_curves(p.experiment);  // draws follow the reference even with a wind table
  const int ncurves = owner_curves(p);
  const int need = 2 * nk * ndraw;           // knot words after the randint word
  const int nwords = kGroupLanes + need;     // <= 48 on the fast path
  const bool grp_ok = nk <= 8;               // 16 lanes = 2 curves x 8 knots
  const uint32_t rng = (uint32_t)(2 * p.start_y_half - 1), mask = range_mask32(rng);
  // rank r's env, fill, cons snapshot and MT position (k_need_masks), loaded
  // with the count and not behind it: list rows below n_pad are always memory
  const int np_ = (int)A.np;
  int r0 = blockIdx.x * kGroups;
  int rq = r0 + g < np_ ? r0 + g : 0;
  int e_n = A.refill_list(0)[rq], f_n = A.refill_list(1)[rq], c_n = A.refill_list(2)[rq], p_n = A.cons_snap()[rq];
  for (; r0 < total; r0 += kGroups * G) {
    const int rr = r0 + g;
    const bool ok = rr < total;
    const int e = ok ? e_n : 0;
    const int c = ok ? c_n : 0;
    const int f0 = ok ? f_n : 0;
    const int pos = ok ? (p_n & kMtPosMask) : kMtN;
    const bool nx = ok && (p_n & kMtNextOk) != 0;  // mt_next holds the next block
    if (r0 + kGroups * G < total) {  // the next iteration's rank, in flight with this one
      rq = rr + kGroups * G < np_ ? rr + kGroups * G : 0;
      e_n = A.refill_list(0)[rq], f_n = A.refill_list(1)[rq], c_n = A.refill_list(2)[rq], p_n = A.cons_snap()[rq];
    }
    if (ok && c >= f0 && gl == 0) atomicOr(&A.status()[1], SACENV_STATUS_SLOT_UNDERFLOW);
    const int f_end = ok && f0 < c + kSlots ? c + kSlots : f0;
    // The group's episodes f0, f0+1, ... on the fast path, one per pass, while
    // each next window lies inside the current MT block (round 4: an env that
    // consumed several episodes drew only its first here, the rest wave by wave
    // at ~4 us each -- about half of a refill's draws)
    int f_next = f0, pos_next = pos;  // the next episode to draw and its MT position
    bool live = ok && f0 < f_end && grp_ok;
    uint32_t* const gw = lds.blk[0] + g * 3 * kGroupLanes;
#pragma unroll 1
    while (__ballot(live) != 0ull) {  // uniform: until every group left the fast path
      // (with the next block pre-twisted, a window may cross the block end)
      bool fast = live && pos_next + nwords <= (nx ? 2 * kMtN : kMtN);
      // the group's words pos_next .. pos_next + nwords - 1 (raw, key order), tempered;
      // index 624 on from mt_next
      const int64_t eo = (int64_t)e * kMtN;
      uint32_t w[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int i = pos_next + gl + kGroupLanes * q;
        const uint32_t* src = i < kMtN ? A.mt_key() + eo + i : A.mt_next() + eo + (i - kMtN);
        w[q] = fast && gl + kGroupLanes * q < nwords ? mt_temper(*src) : 0u;
      }
      wave_lds_sync();  // the last pass's reads of gw are done
#pragma unroll
      for (int q = 0; q < 3; ++q) gw[gl + kGroupLanes * q] = w[q];
      // np.random.randint (boat_env.py:147-150): the first accepted of the first 16 words
      const unsigned long long acc = __ballot(fast && (w[0] & mask) <= rng);
      const uint32_t gacc = (uint32_t)(acc >> (kGroupLanes * g)) & 0xFFFFu;
      fast = fast && gacc != 0u;
      const int k = fast ? __builtin_ctz(gacc) : 0;
      wave_lds_sync();  // the group's words, then reads
      REFILL_STAMP(stm[2], "v"(k));
      if (fast) {
        const int slot = f_next % kSlots;
        const int cc = gl / 8, jj = gl % 8;  // knot jj of curve cc (wind.py:78; velocity first)
        if (cc < ncurves && jj < nk) {
          const int src = k + 1 + cc * 2 * nk + 2 * jj;  // np.random.sample: res53 of two words
          const double kv = res53(gw[src], gw[src + 1]);
          A.wind_knots()[2 * A.wix(slot, cc, jj, e)] = kv;  // k_refill_fit's input, in the slot's y
          if (A.rk) A.knots_raw()[A.wix(slot, cc, jj, e)] = kv;
        }
        if (gl == 0) {
          A.i32(U_STARTY)[(int64_t)slot * A.np + e] = -p.start_y_half + (int32_t)(gw[k] & mask);
          A.i32(U_MTPOS)[e] = (pos_next + k + 1 + need) | (nx ? kMtNextOk : 0);
        }
        f_next = f_next + 1;
        pos_next = pos_next + k + 1 + need;
      }
      live = fast && f_next < f_end;
    }
    wave_lds_sync();  // LDS free for the wave draws
    // the rest, env by env, by the whole wave
#pragma unroll 1
    for (int j = 0; j < kGroups; ++j) {
      const int src = j * kGroupLanes;
      if (__builtin_amdgcn_readlane((int)ok, src) == 0) break;  // uniform; later groups too
      const int ej = __builtin_amdgcn_readlane(e, src);
      const int fe = __builtin_amdgcn_readlane(f_end, src);
      int f = __builtin_amdgcn_readlane(f_next, src);
      const int pj = __builtin_amdgcn_readlane(pos_next, src);
      bool first = true;
      for (; f < fe; ++f) {
        const int32_t start_y = draw_knots_wave(p, A, lds, ej, lane, nullptr, nullptr, first ? pj : -1);
#ifdef SACENV_STAMPS
        const int sb = 3 + (n_st < 18 ? n_st : 18);  // the end of each wave draw (first 19)
        ++n_st;
#endif
        REFILL_STAMP(stm[sb], "v"(start_y));
        first = false;
        __syncthreads();
        store_draw(p, A, lds, ej, f % kSlots, start_y, lane, true);
        __syncthreads();
      }
      if (lane == 0) {
        A.i32(U_FILL)[ej] = fe;
        A.refill_list(1)[r0 + j] = __builtin_amdgcn_readlane(f0, src);
        A.refill_list(2)[r0 + j] = fe;
      }
    }
  }
#ifdef SACENV_STAMPS
  stm[22] = __builtin_amdgcn_s_memrealtime();
  stm[23] = (uint64_t)n_st;
  if (lane == 0 && (int64_t)(blockIdx.x + 1) * kRefillStamps * 8 <= 24 * A.np) {
    uint64_t* d = reinterpret_cast<uint64_t*>(A.accel()) + (int64_t)blockIdx.x * kRefillStamps;
    for (int i = 0; i < kRefillStamps; ++i) d[i] = stm[i];
  }
#endif
}

// sacenv_boat_refill, launch 2: the twist-ahead workgroups (mt_ahead), then the
// spline fits of the episodes launch 1 drew (fit_group), grid-stride over the groups.
// GS lanes per (env, curve): 8 for up to 8 knots, else 16; one instantiation
// per width, so the 8-knot launch carries no 16-knot registers
template <int GS, bool kFull>
__global__ void __launch_bounds__(kWave) k_refill_fit(SacenvBoatParams p, Arena A, Tail T) {
  const int lane = threadIdx.x;
  const int ahead = (int)(A.np / kAheadEnvs);
  if ((int)blockIdx.x < ahead) {
    mt_ahead(p, A, (int)blockIdx.x, lane);
    return;
  }
  const int fb = (int)blockIdx.x - ahead, fgrid = (int)gridDim.x - ahead;
  // (owner_curves(p), spelled out: through the call the scheduler swaps two scalar
  // instructions of this kernel, and a refactor leaves every kernel as it was)
  const int nc = p.use_wind_table ? 0 : n_curves(p.experiment);
  const int nk = kFull ? GS : p.n_knots;
  const int items = A.status()[2] * nc;  // (env, curve) groups
#ifdef SACENV_STAMPS
  const uint64_t st0 = __builtin_amdgcn_s_memrealtime();
  uint64_t* const fst = reinterpret_cast<uint64_t*>(A.reward64()) + 2 * (int64_t)blockIdx.x;
  const bool fst_ok = lane == 0 && (int64_t)(blockIdx.x + 1) * 16 <= 8 * A.np;
  if (fst_ok) fst[0] = st0, fst[1] = 0;
#endif
  if (items == 0 || fb * (kWave / GS) >= items) return;  // uniform
  const int j = lane & (GS - 1);
  const int jj = j < nk ? j : nk - 1, j1 = jj + 1 < nk ? jj + 1 : jj;
  double gr[GS];
#pragma unroll
  for (int k = 0; k < GS; ++k) gr[k] = kFull || k < nk ? T.g[jj * nk + k] : 0.0;
  IvGrid ig = interval_grid(p, j < nk - 1 ? j : 0);
  ig.valid = ig.valid && j < nk - 1;
  const int per = kWave / GS;
  for (int base = fb * per; base < items; base += fgrid * per) {
    const int item = base + lane / GS;
    if (item >= items) break;
    fit_group<GS, kFull>(p, A, gr, ig, item, j, jj, j1, nc);
  }
#ifdef SACENV_STAMPS
  __syncthreads();
  if (fst_ok) fst[1] = __builtin_amdgcn_s_memrealtime();
#endif
}

// sacenv_boat_refill, launch 0: which envs consumed pre-drawn episodes since
// their ring was last topped up (fill < cons + SLOTS), listed for launch 1 in
// env order. Derived from the episode counters, so the step launch keeps no
// flags of its own (measured: owner-side flag words cost 0.25-0.4 us/step).
// 16 owner waves' envs per workgroup (one wave each). A workgroup counts its
// flagged envs (ballots, a scan of the 16 popcounts), publishes the count as
// its look-back word (refill_mask[b] = (epoch, count); epoch = refills done + 1,
// so no word of an earlier refill matches and nothing is reset), sums the words
// of workgroups 0..b-1 -- one vector load of up to 64 words per pass, polled
// until every one carries this epoch -- and stores each flagged env's id at its
// rank in refill_list(0), one coalesced store per wave; the last workgroup
// stores the total in status[2]. k_refill then finds its envs with one load
// each. The ranks are those of a serial scan over the envs (the lists, and so
// the arenas, are the same at every run). Round 2's design had the last
// workgroup to take a ticket rank all 1 024 masks: 14.7 us a refill.
__device__ __forceinline__ unsigned long long lookback_load(const unsigned long long* w) {
  return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ void __launch_bounds__(kMaskThreads) k_need_masks(SacenvBoatParams p, Arena A) {
  __shared__ int wcnt[kMaskThreads / kWave];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t >> 6;
  const int nw = A.nwaves(), b = (int)blockIdx.x;
  const int w = b * (kMaskThreads / kWave) + wv, e = w * kWave + lane;
  const uint32_t epoch = (uint32_t)A.status()[0] + 1u;
  bool need = false;
  int c = 0, fl = 0, mp = 0;
  if (w < nw && e < p.n_envs) {
    c = A.i32(U_CONS)[e];
    fl = A.i32(U_FILL)[e];
    mp = A.i32(U_MTPOS)[e];
    need = fl < c + kSlots;
  }
  const unsigned long long m = __ballot(need);
  if (lane == 0) wcnt[wv] = __popcll(m);
  __syncthreads();
  if (t < kWave) {  // wave 0: the workgroup's count, its look-back, each wave's base
    unsigned long long* const look = A.refill_mask();
    const int cnt = t < kMaskThreads / kWave ? wcnt[t] : 0;
    const int incl = wave_incl_scan(cnt);
    const int total = __builtin_amdgcn_readlane(incl, kMaskThreads / kWave - 1);
    if (t == 0)
      __hip_atomic_store(look + b, ((unsigned long long)epoch << 32) | (uint32_t)total, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    int before = 0;
    for (int q0 = 0; q0 < b; q0 += kWave) {
      const int q = q0 + t;
      unsigned long long x = q < b ? lookback_load(look + q) : ((unsigned long long)epoch << 32);
      for (uint32_t it = 0; __ballot((uint32_t)(x >> 32) != epoch) != 0ull; ++it) {
        if (it >= kSpinLimit) {  // a predecessor that never publishes: flag it, rank as if it listed none
          if (t == 0) atomicOr(&A.status()[1], SACENV_STATUS_LIST_TIMEOUT);
          break;
        }
        __builtin_amdgcn_s_sleep(1);
        if ((uint32_t)(x >> 32) != epoch) x = lookback_load(look + q);
      }
      int v = (uint32_t)(x >> 32) == epoch ? (int)(uint32_t)x : 0;
      v += __shfl_xor(v, 32);
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 8);
      v += __shfl_xor(v, 4);
      v += __shfl_xor(v, 2);
      v += __shfl_xor(v, 1);
      before += v;
    }
    if (t < kMaskThreads / kWave) wcnt[t] = before + incl - cnt;
    if (t == 0 && b == (int)gridDim.x - 1) A.status()[2] = before + total;
  }
  __syncthreads();
  if (need) {  // rank r: the env and its counters as of now, one load each for k_refill
    const int r = wcnt[wv] + __popcll(m & ((1ull << lane) - 1ull));
    A.refill_list(0)[r] = e;
    A.refill_list(1)[r] = fl;
    A.refill_list(2)[r] = c;  // the cons snapshot (k_refill then stores the end episode here)
    A.cons_snap()[r] = mp;
  }
}

// The step launch. Grid: nb_boat owner waves, then (kMixed) the waves of
// each toy arena: heterogeneous workgroups of one launch, selected by
// uniform block-index ranges. One wave per workgroup (measured against 2 and
// 4 waves, with or without LDS padding to one workgroup per CU: 6.04-6.29 us
// against 5.33-5.35).
template <bool kMixed, int kNc, bool kTIdx>
__global__ void __launch_bounds__(kWave) k_step(SacenvBoatParams p, Arena A, Tail T,
                                                const float* __restrict__ action, int nb_boat,
                                                MixedToys M, char* __restrict__ trans) {
  __shared__ OwnerLds slds;
  const int lane = threadIdx.x;
  int b = (int)blockIdx.x;
  if (!kMixed || b < nb_boat) {
    // (the parameters stay in SGPRs: VGPR copies ahead of the load burst delay it in
    // every launch, measured k_step 5.79 -> 5.37 us without them)
    owner_wave<false, kNc, kTIdx>(p, A, T, action, slds, b, lane, 1, nullptr,
                                  trans);
    return;
  }
  b -= nb_boat;
  if (b < M.nb[0]) {
    toy_wave(M.p[0], M.a[0], b, lane);
  } else if (M.n > 1) {
    toy_wave(M.p[1], M.a[1], b - M.nb[0], lane);
  }
}

// The multi-step launches (rollout_body): one owner wave per SIMD with the fp64
// constants as VGPR copies (k_rollout), or two with them as literals (k_rollout_dense)
template <int kNc, bool kTIdx, int kRows, bool kLean = false>
__global__ void __launch_bounds__(kWave) k_rollout(SacenvBoatParams p, Arena A, Tail T,
                                                   const float* __restrict__ action, int n_steps, RollArgs ra) {
  __shared__ OwnerLds slds;
  rollout_body<kNc, kTIdx, kRows, true, kLean>(p, A, T, action, n_steps, ra, slds);
}
template <int kNc, bool kTIdx, int kRows, bool kLean = false>
__global__ void __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_rollout_dense(SacenvBoatParams p, Arena A, Tail T, const float* __restrict__ action, int n_steps, RollArgs ra) {
  __shared__ OwnerLds slds;
  rollout_body<kNc, kTIdx, kRows, false, kLean>(p, A, T, action, n_steps, ra, slds);
}

// sacenv_mixed_segment (BASELINE configs[4] as one persistent launch): the
// boat's owner waves (k_rollout's open loop) and each toy arena's waves,
// heterogeneous workgroups selected by uniform block-index ranges
template <int kNc, bool kTIdx, bool kLean = false>
__global__ void __launch_bounds__(kWave) k_rollout_mixed(SacenvBoatParams p, Arena A, Tail T,
                                                         const float* __restrict__ action, int n_steps, RollArgs ra,
                                                         int nb_boat, MixedToys M) {
  __shared__ OwnerLds slds;
  const int lane = threadIdx.x;
  int b = (int)blockIdx.x;
  if (b < nb_boat) {
    owner_wave<true, kNc, kTIdx, false, 0, true, kLean>(vreg_params(p), A, vreg_tail(T), action, slds, b, lane,
                                                         n_steps, &ra);
    return;
  }
  b -= nb_boat;
  if (b < M.nb[0]) {
    toy_roll_wave(M.p[0], M.a[0], b, lane, n_steps);
  } else if (M.n > 1) {
    toy_roll_wave(M.p[1], M.a[1], b - M.nb[0], lane, n_steps);
  }
}

__global__ void __launch_bounds__(kWave) k_toy_init(SacenvToyParams p, ToyArena T, const int32_t* __restrict__ ids,
                                                    int n, int zero_counters) {
  const int q = blockIdx.x * kWave + threadIdx.x;
  if (q >= n) return;
  const int e = ids != nullptr ? ids[q] : q;
  if (e < 0 || e >= p.n_envs) return;
  double f[5];
  float obs[2];
  toy_initial(p, f, obs);
  for (int k = 0; k < 5; ++k) T.f(k)[e] = f[k];
  T.count()[e] = 0;
  if (zero_counters)
    for (int k = 0; k < 3; ++k) T.ctr(k)[e] = 0u;
  reinterpret_cast<float2*>(T.obs())[e] = make_float2(obs[0], obs[1]);
  T.reward()[e] = 0.0f;
  T.done()[e] = 0;
  T.term()[e] = 0;
}

__global__ void __launch_bounds__(kWave) k_toy_step(SacenvToyParams p, ToyArena T) {
  toy_wave(p, T, blockIdx.x, threadIdx.x);
}

__global__ void __launch_bounds__(256) k_wind_eval(SacenvBoatParams p, Arena A, Tail T,
                                                   const int32_t* __restrict__ env_ids,
                                                   const int32_t* __restrict__ idx, int n,
                                                   double* __restrict__ out_v, double* __restrict__ out_a) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const int e = env_ids[q];
  if (e < 0 || e >= p.n_envs) return;
  const int slot = p.autoreset ? A.i32(U_CONS)[e] % kSlots : 0;
  double wv, wa;
  wind_at(p, A, T.table, slot, e, idx[q], wv, wa);
  out_v[q] = wv;
  out_a[q] = wa;
}

// ---------------------------------------------------------------- host side

int check_params(const SacenvBoatParams* p) {
  if (p == nullptr) return SACENV_E_NULL;
  if (p->experiment < 1 || p->experiment > 6) return SACENV_E_EXPERIMENT;
  if (p->n_envs <= 0 || p->n_envs > (1 << 22) || p->wind_len <= 0) return SACENV_E_SIZE;  // 32-bit offsets
  if (n_curves(p->experiment) > 0 && (p->n_knots < 4 || p->n_knots > kMaxK)) return SACENV_E_KNOTS;
  if (p->n_knots < 2 || p->n_knots > kMaxK) return SACENV_E_KNOTS;
  if (n_curves(p->experiment) > 0 && !p->use_wind_table && p->wind_len < 2) return SACENV_E_SIZE;
  if (p->start_y_half < 1) return SACENV_E_RANGE;
  if (p->autoreset && (p->n_helpers < 1 || p->n_helpers > 65536)) return SACENV_E_SIZE;
  return SACENV_OK;
}

Tail make_tail(const SacenvBoatParams& p, void* arena) {
  const Arena A = make_arena(p, arena);
  Tail T;
  T.g = reinterpret_cast<const double*>(A.b + off_spline_g(A.ur(), A.np));
  T.table = reinterpret_cast<const double*>(A.b + off_wind_table(A.ur(), A.np));
  T.r_mx = 1.0 / p.m_plus_mx;
  T.r_my = 1.0 / p.m_plus_my;
  T.r_iz = 1.0 / p.i_plus_iz;
  T.r_nd = 1.0 / p.n_times_d;
  T.r_w = 1.0 / p.track_width;
  T.r_goal = 1.0 / p.goal_line;
  T.r_two_w = 1.0 / (p.track_width + p.track_width);
  T.r_fuel = 1.0 / (double)p.fuel0;
  T.k_front = p.c_r_front * 0.5 * p.rho * p.boat_area_front;                  // F_R, F_W
  T.k_thrust = p.n_squared * p.rho * p.d_pow4 * p.one_minus_td;               // F_T / KT
  T.k_side = p.c_r_side * 0.5 * p.rho * p.boat_area_side;                     // F_R (transverse), F_W
  T.k_rud_front = p.c_r_front * 0.5 * p.rho * p.rudder_area;                  // F_RU
  T.k_hull = p.c_r_side * 0.5 * p.rho * p.boat_area_side * p.boat_l * 5.0;    // M_hull
  T.k_rud_moment = p.c_r_side * 0.5 * p.rho * p.rudder_area * (p.boat_b / 2);  // M_rudder
  return T;
}

int launch_status() {
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? SACENV_OK : (int)err;
}

inline int blocks_for(int n, int per) { return (n + per - 1) / per; }
// owner waves of a launch: one per 64 envs, the last one padded
inline int owner_waves(const SacenvBoatParams& p) { return (int)(pad64(p.n_envs) / kWave); }

int check_toy(const SacenvToyParams* p) {
  if (p == nullptr) return SACENV_E_NULL;
  if (p->kind != SACENV_TOY_PARACHUTE && p->kind != SACENV_TOY_CAR) return SACENV_E_EXPERIMENT;
  if (p->n_envs <= 0) return SACENV_E_SIZE;
  return SACENV_OK;
}

ToyArena make_toy_arena(const SacenvToyParams& p, void* base) {
  return ToyArena{static_cast<char*>(base), pad64(p.n_envs)};
}

// ---- kernel choice: every family's instantiation for a launch is picked here,
// once; the entry points launch (or ask the runtime about) the pointer they get.
using StepKernel = void (*)(SacenvBoatParams, Arena, Tail, const float*, int, MixedToys, char*);
using RolloutKernel = void (*)(SacenvBoatParams, Arena, Tail, const float*, int, RollArgs);
using MixedRolloutKernel = void (*)(SacenvBoatParams, Arena, Tail, const float*, int, RollArgs, int, MixedToys);
using FitKernel = void (*)(SacenvBoatParams, Arena, Tail);

// The step kernels' wind kind and t rule (owner_wave's template arguments): the
// one switch over them; f gets them as Owner<kNc, kTIdx>.
template <int kNc, bool kTIdx>
struct Owner {
  static constexpr int nc = kNc;
  static constexpr bool ti = kTIdx;
};
template <class F>
auto owner_dispatch(const SacenvBoatParams& p, F f) {
  switch (owner_curves(p) * 2 + (t_from_index(p.dt) ? 1 : 0)) {
    case 0: return f(Owner<0, false>{});
    case 1: return f(Owner<0, true>{});
    case 2: return f(Owner<1, false>{});
    case 3: return f(Owner<1, true>{});
    case 4: return f(Owner<2, false>{});
    default: return f(Owner<2, true>{});
  }
}

StepKernel step_kernel(const SacenvBoatParams& p, bool mixed) {
  return owner_dispatch(p, [mixed](auto o) -> StepKernel {
    using O = decltype(o);
    return mixed ? k_step<true, O::nc, O::ti> : k_step<false, O::nc, O::ti>;
  });
}

// More owner waves than the device has SIMDs: the two-waves-per-SIMD
// instantiation (k_rollout_dense), which keeps every owner wave resident.
bool dense_grid(int nb_boat) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return false;
  return nb_boat > 4 * cus;
}

// The lean instantiation's conditions (owner_wave's kLean), all of them: the
// persistent segment of a training loop. Any other launch takes the general one.
bool lean_launch(const SacenvBoatParams& p, const RollArgs& ra) {
  return p.out_flags == 0 && p.autoreset != 0 && p.experiment != 2 && p.fuel0 != 0 && ra.rec_stride == 0 &&
         ra.fin_stride == 0;
}

// The rows a multi-step launch writes besides the record (owner_wave's kRows):
// 2 staged replay rows, 1 pooled rows, 3 a fresh record per step, 0 none.
int rollout_rows(const RollArgs& ra) {
  return ra.stage != nullptr ? 2 : ra.trans != nullptr ? 1 : ra.rec_stride != 0 ? 3 : 0;
}

template <int kNc, bool kTIdx, int kRows, bool kLean = false>
RolloutKernel rollout_one(bool dense) {
  return dense ? k_rollout_dense<kNc, kTIdx, kRows, kLean> : k_rollout<kNc, kTIdx, kRows, kLean>;
}
// k_rollout / k_rollout_dense for the launch: 6 owners x 6 (rows, lean) x 2. Lean
// exists for the staged rows and the plain record in place (rows 2 and 0); the
// pooled rows and the fresh rows of sacenv_boat_rollout stay general.
RolloutKernel rollout_kernel(const SacenvBoatParams& p, int rows, bool lean, bool dense) {
  return owner_dispatch(p, [=](auto o) -> RolloutKernel {
    constexpr int nc = decltype(o)::nc;
    constexpr bool ti = decltype(o)::ti;
    switch (rows) {
      case 0: return lean ? rollout_one<nc, ti, 0, true>(dense) : rollout_one<nc, ti, 0>(dense);
      case 1: return rollout_one<nc, ti, 1>(dense);
      case 2: return lean ? rollout_one<nc, ti, 2, true>(dense) : rollout_one<nc, ti, 2>(dense);
      default: return rollout_one<nc, ti, 3>(dense);
    }
  });
}

MixedRolloutKernel rollout_mixed_kernel(const SacenvBoatParams& p, bool lean) {
  return owner_dispatch(p, [lean](auto o) -> MixedRolloutKernel {
    using O = decltype(o);
    return lean ? k_rollout_mixed<O::nc, O::ti, true> : k_rollout_mixed<O::nc, O::ti>;
  });
}

// the refill's fit: 8 or 16 knots per group, kFull when every one is used
FitKernel refill_fit_kernel(int n_knots) {
  return n_knots == 8   ? k_refill_fit<8, true>
         : n_knots < 8  ? k_refill_fit<8, false>
         : n_knots == 16 ? k_refill_fit<16, true>
                         : k_refill_fit<16, false>;
}

// The RollArgs of a launch that writes the arena's own record every step: the
// record, the terminal obs behind it (strides 0) and the hand-off status word.
RollArgs arena_roll_args(const Arena& A) {
  RollArgs ra{};
  ra.rec = A.b + A.ur() * A.np;
  ra.fin = reinterpret_cast<float*>(ra.rec + R_FIN * A.np);
  ra.status = reinterpret_cast<int32_t*>(A.b + off_status(A.ur(), A.np)) + 1;
  return ra;
}

int launch_multi(const SacenvBoatParams& p, void* arena, const float* actions, int n_steps, const RollArgs& ra,
                 void* stream) {
  const int nb_boat = owner_waves(p);
  const RolloutKernel k = rollout_kernel(p, rollout_rows(ra), lean_launch(p, ra), dense_grid(nb_boat));
  hipLaunchKernelGGL(k, dim3(nb_boat), dim3(kWave), 0, (hipStream_t)stream, p, make_arena(p, arena),
                     make_tail(p, arena), actions, n_steps, ra);
  return launch_status();
}

// A mixed launch's workgroups: the boat's owner waves (if any) first, then each
// toy arena's waves.
struct MixedLaunch {
  MixedToys M{};
  SacenvBoatParams p{};  // (no boat: zeroed, and no owner wave runs)
  Arena A{};
  Tail T{};
  int nb_boat = 0, nb = 0;
};
int mixed_setup(const SacenvBoatParams* bp, void* boat_arena, const float* boat_actions,
                const SacenvToyParams* toy_params, void* const* toy_arenas, int32_t n_toys, int32_t n_steps,
                MixedLaunch* L) {
  int rc;
  if (n_toys < 0 || n_toys > 2) return SACENV_E_SIZE;
  if (n_toys > 0 && (toy_params == nullptr || toy_arenas == nullptr)) return SACENV_E_NULL;
  if (n_steps < 1) return SACENV_E_SIZE;
  L->M.n = n_toys;
  for (int t = 0; t < n_toys; ++t) {
    if ((rc = check_toy(&toy_params[t]))) return rc;
    if (toy_arenas[t] == nullptr) return SACENV_E_NULL;
    L->M.p[t] = toy_params[t];
    L->M.a[t] = make_toy_arena(toy_params[t], toy_arenas[t]);
    L->M.nb[t] = blocks_for(toy_params[t].n_envs, kWave);
    L->nb += L->M.nb[t];
  }
  if (bp != nullptr) {
    if ((rc = check_params(bp))) return rc;
    if (boat_arena == nullptr || boat_actions == nullptr) return SACENV_E_NULL;
    L->p = *bp;
    L->A = make_arena(*bp, boat_arena);
    L->T = make_tail(*bp, boat_arena);
    L->nb_boat = owner_waves(*bp);
    L->nb += L->nb_boat;
  }
  return SACENV_OK;
}

}  // namespace

extern "C" {

int sacenv_abi_version(void) { return SACENV_ABI_VERSION; }

int sacenv_stream_create_exclusive(void** stream) {
  if (stream == nullptr) return SACENV_E_NULL;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, dev);
  if (e != hipSuccess) return (int)e;
  uint32_t mask[64];
  const int words = (prop.multiProcessorCount + 31) / 32;
  if (words > 64) return SACENV_E_SIZE;
  for (int i = 0; i < words; ++i) mask[i] = 0xFFFFFFFFu;  // every CU (extra bits are ignored)
  hipStream_t s = nullptr;
  e = hipExtStreamCreateWithCUMask(&s, (uint32_t)words, mask);
  if (e != hipSuccess) return (int)e;
  *stream = s;
  return SACENV_OK;
}

int sacenv_stream_destroy(void* stream) {
  if (stream == nullptr) return SACENV_E_NULL;
  return (int)hipStreamDestroy((hipStream_t)stream);
}

const char* sacenv_error_string(int code) {
  switch (code) {
    case SACENV_OK: return "ok";
    case SACENV_E_NULL: return "required pointer is NULL";
    case SACENV_E_EXPERIMENT: return "Well someone tried to use an experiment that doesnt exist!";
    case SACENV_E_KNOTS:
      return "Please select at least 4 fixed_points in your config. The interpolation doesn't work "
             "otherwise! (max 16)";
    case SACENV_E_SIZE: return "size out of range";
    case SACENV_E_RANGE: return "low >= high: int(0.8*track_width) must be >= 1";
    case SACENV_E_MODE: return "call not valid in this autoreset mode";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown sacenv error";
  }
}

int sacenv_boat_layout(const SacenvBoatParams* p, SacenvBoatLayout* out) {
  const int rc = check_params(p);
  if (rc) return rc;
  if (out == nullptr) return SACENV_E_NULL;
  compute_layout(p->n_envs, p->n_knots, p->wind_len, p->use_wind_table, (p->out_flags & SACENV_OUT_KNOTS) != 0, out);
  return SACENV_OK;
}

int sacenv_boat_init(const SacenvBoatParams* p, void* arena, const uint32_t* seeds, void* stream) {
  int rc = check_params(p);
  if (rc) return rc;
  if (arena == nullptr || seeds == nullptr) return SACENV_E_NULL;
  const hipStream_t s = (hipStream_t)stream;
  const Arena A = make_arena(*p, arena);
  const Tail T = make_tail(*p, arena);
  hipLaunchKernelGGL(k_spline_g, dim3(1), dim3(1), 0, s, *p, const_cast<double*>(T.g));
  if ((rc = launch_status())) return rc;
  hipLaunchKernelGGL(k_seed, dim3(blocks_for(p->n_envs, kWave)), dim3(kWave), 0, s, *p, A, seeds);
  if ((rc = launch_status())) return rc;
  hipLaunchKernelGGL(k_draw, dim3(p->n_envs), dim3(kWave), 0, s, *p, A, T, 0, (const int32_t*)nullptr,
                     (const int32_t*)nullptr, (const double*)nullptr, (const int32_t*)nullptr);
  if ((rc = launch_status())) return rc;
  return p->autoreset ? sacenv_boat_refill(p, arena, stream) : SACENV_OK;  // episodes 1 .. SLOTS-1
}

int sacenv_boat_reset(const SacenvBoatParams* p, void* arena, const int32_t* ids, int32_t n_ids,
                      void* stream) {
  int rc = check_params(p);
  if (rc) return rc;
  if (arena == nullptr) return SACENV_E_NULL;
  const int nb = ids != nullptr ? n_ids : p->n_envs;
  if (nb < 0) return SACENV_E_SIZE;
  if (nb == 0) return SACENV_OK;
  const hipStream_t s = (hipStream_t)stream;
  const Arena A = make_arena(*p, arena);
  const Tail T = make_tail(*p, arena);
  hipLaunchKernelGGL(k_draw, dim3(nb), dim3(kWave), 0, s, *p, A, T, 1, ids, (const int32_t*)nullptr,
                     (const double*)nullptr, (const int32_t*)nullptr);
  return launch_status();
}

int sacenv_compact_done(const uint8_t* done, int32_t n, int32_t* ids, int32_t* count, void* stream) {
  if (n < 0) return SACENV_E_SIZE;
  if (count == nullptr || (n > 0 && (done == nullptr || ids == nullptr))) return SACENV_E_NULL;
  const int aligned = (reinterpret_cast<uintptr_t>(done) & 15u) == 0;
  hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, (hipStream_t)stream, done, n, aligned, ids, count);
  return launch_status();
}

int sacenv_boat_reset_list(const SacenvBoatParams* p, void* arena, const int32_t* ids, const int32_t* count,
                           void* stream) {
  int rc = check_params(p);
  if (rc) return rc;
  if (arena == nullptr || ids == nullptr || count == nullptr) return SACENV_E_NULL;
  const hipStream_t s = (hipStream_t)stream;
  const Arena A = make_arena(*p, arena);
  const Tail T = make_tail(*p, arena);
  // at most one workgroup per CU-slot; each loops over its share of the device-side list
  const int grid = p->n_envs < 1024 ? p->n_envs : 1024;
  hipLaunchKernelGGL(k_draw, dim3(grid), dim3(kWave), 0, s, *p, A, T, 1, ids, (const int32_t*)nullptr,
                     (const double*)nullptr, count);
  return launch_status();
}

int sacenv_boat_reset_explicit(const SacenvBoatParams* p, void* arena, const int32_t* ids, int32_t n_ids,
                               const int32_t* start_y, const double* knots, void* stream) {
  int rc = check_params(p);
  if (rc) return rc;
  if (p->autoreset) return SACENV_E_MODE;
  if (arena == nullptr || ids == nullptr || start_y == nullptr) return SACENV_E_NULL;
  if (n_curves(p->experiment) > 0 && !p->use_wind_table && knots == nullptr) return SACENV_E_NULL;
  if (n_ids < 0) return SACENV_E_SIZE;
  if (n_ids == 0) return SACENV_OK;
  hipLaunchKernelGGL(k_draw, dim3(n_ids), dim3(kWave), 0, (hipStream_t)stream, *p, make_arena(*p, arena),
                     make_tail(*p, arena), 2, ids, start_y, knots, (const int32_t*)nullptr);
  return launch_status();
}

static int boat_step(const SacenvBoatParams* p, void* arena, const float* action, char* trans, void* stream) {
  int rc = check_params(p);
  if (rc) return rc;
  if (arena == nullptr || action == nullptr) return SACENV_E_NULL;
  const int nb_boat = owner_waves(*p);
  hipLaunchKernelGGL(step_kernel(*p, false), dim3(nb_boat), dim3(kWave), 0, (hipStream_t)stream, *p,
                     make_arena(*p, arena), make_tail(*p, arena), action, nb_boat, MixedToys{}, trans);
  return launch_status();
}

int sacenv_boat_step(const SacenvBoatParams* p, void* arena, const float* action, void* stream) {
  return boat_step(p, arena, action, nullptr, stream);
}

int sacenv_boat_step_pooled(const SacenvBoatParams* p, void* arena, const float* action, void* trans,
                            void* stream) {
  if (trans == nullptr) return SACENV_E_NULL;
  if ((reinterpret_cast<uintptr_t>(trans) & 15u) != 0u) return SACENV_E_RANGE;  // float4 row stores
  return boat_step(p, arena, action, static_cast<char*>(trans), stream);
}

int sacenv_boat_rollout(const SacenvBoatParams* p, void* arena, const float* actions, int32_t n_steps,
                        void* records, float* final_obs, void* stream) {
  int rc = check_params(p);
  if (rc) return rc;
  if (arena == nullptr || actions == nullptr || records == nullptr) return SACENV_E_NULL;
  if (n_steps < 1 || (p->autoreset && n_steps > SACENV_REFILL_PERIOD)) return SACENV_E_SIZE;
  const int64_t np = pad64(p->n_envs);
  RollArgs ra{};
  ra.rec = static_cast<char*>(records);
  ra.rec_stride = SACENV_RECORD_BYTES * np;
  ra.fin = final_obs;
  ra.fin_stride = np * SACENV_OBS_DIM;
  ra.act_stride = p->n_envs;
  return launch_multi(*p, arena, actions, n_steps, ra, stream);
}

int sacenv_boat_segment(const SacenvBoatParams* p, void* arena, const float* actions, int64_t action_stride,
                        int32_t n_steps, const uint32_t* act_ready, uint32_t* step_done, uint32_t seq0,
                        void* trans, int64_t trans_stride, void* stage, uint64_t* stage_marks,
                        void* stream) {
  int rc = check_params(p);
  if (rc) return rc;
  if (arena == nullptr || actions == nullptr) return SACENV_E_NULL;
  if (n_steps < 1 || (p->autoreset && n_steps > SACENV_REFILL_PERIOD)) return SACENV_E_SIZE;
  if (action_stride < p->n_envs ||
      ((act_ready != nullptr || step_done != nullptr) && (uint64_t)seq0 + (uint64_t)n_steps >= 0x80000000ull))
    return SACENV_E_RANGE;
  if (trans != nullptr && ((reinterpret_cast<uintptr_t>(trans) & 15u) != 0u || (trans_stride & 15) != 0))
    return SACENV_E_RANGE;  // float4 row stores
  if (stage != nullptr && (trans != nullptr || (reinterpret_cast<uintptr_t>(stage) & 15u) != 0u))
    return SACENV_E_RANGE;  // one kind of rows per launch; float4 stores
  // the marks are staged into the wave's LDS (OwnerLds::mk: one word per step, REFILL_PERIOD
  // entries), whatever the autoreset setting
  if (stage_marks != nullptr && n_steps > SACENV_REFILL_PERIOD) return SACENV_E_SIZE;
  RollArgs ra = arena_roll_args(make_arena(*p, arena));
  ra.trans = static_cast<char*>(trans);
  ra.trans_stride = trans_stride;
  ra.stage = static_cast<char*>(stage);
  ra.marks = reinterpret_cast<unsigned long long*>(stage_marks);
  ra.act_stride = action_stride;
  ra.ready = act_ready;
  ra.done = step_done;
  ra.seq0 = seq0;
  return launch_multi(*p, arena, actions, n_steps, ra, stream);
}

// The segment launch's kernel resources for these params, for the closed
// loop's co-residency plan (sacenv.h): resident one-wave workgroups per CU
// (hipOccupancyMaxActiveBlocksPerMultiprocessor), the grid, VGPRs per lane as
// allocated and LDS bytes per workgroup (hipFuncGetAttributes).
int sacenv_boat_segment_occupancy(const SacenvBoatParams* p, int32_t with_trans, int32_t* blocks_per_cu,
                                  int32_t* grid, int32_t* vgprs, int32_t* lds_bytes) {
  int rc = check_params(p);
  if (rc) return rc;
  if (blocks_per_cu == nullptr || grid == nullptr || vgprs == nullptr || lds_bytes == nullptr) return SACENV_E_NULL;
  // the kernel launch_multi picks for a segment (strides 0) with these rows
  const int nb_boat = owner_waves(*p);
  const int rows = with_trans == 2 ? 2 : with_trans ? 1 : 0;
  const RolloutKernel k = rollout_kernel(*p, rows, lean_launch(*p, RollArgs{}), dense_grid(nb_boat));
  int nb = 0;
  hipFuncAttributes fa{};
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, kWave, 0);
  if (e == hipSuccess) e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k));
  if (e != hipSuccess) return (int)e;
  *blocks_per_cu = nb;
  *grid = nb_boat;
  *vgprs = fa.numRegs;
  *lds_bytes = (int32_t)fa.sharedSizeBytes;
  return SACENV_OK;
}

int sacenv_boat_refill(const SacenvBoatParams* p, void* arena, void* stream) {
  int rc = check_params(p);
  if (rc) return rc;
  if (arena == nullptr) return SACENV_E_NULL;
  if (!p->autoreset) return SACENV_E_MODE;
  const Arena A = make_arena(*p, arena);
  const unsigned mask_blocks = (unsigned)((A.np / kWave + kMaskThreads / kWave - 1) / (kMaskThreads / kWave));
  hipLaunchKernelGGL(k_need_masks, dim3(mask_blocks), dim3(kMaskThreads), 0, (hipStream_t)stream, *p, A);
  if ((rc = launch_status())) return rc;
  hipLaunchKernelGGL(k_refill, dim3(p->n_helpers), dim3(kWave), 0, (hipStream_t)stream, *p, A);
  if ((rc = launch_status())) return rc;
  // the fit's item count (episodes drawn x curves) is on the device: a grid
  // that covers a typical refill in one pass (8 groups per block: 65 536
  // (episode, curve) items), grid-stride beyond it; blocks past the count exit
  // at once. Measured 0.12 us/step better than one block per owner wave.
  // (+ the twist-ahead workgroups first, np / kAheadEnvs: measured ahead of
  // twisting in the fit blocks, before or after their fits)
  const int fit_blocks = 8192 + (int)(A.np / kAheadEnvs);
  hipLaunchKernelGGL(refill_fit_kernel(p->n_knots), dim3(fit_blocks), dim3(kWave), 0, (hipStream_t)stream, *p, A,
                     make_tail(*p, arena));
  return launch_status();
}

int sacenv_toy_layout(const SacenvToyParams* p, SacenvToyLayout* out) {
  const int rc = check_toy(p);
  if (rc) return rc;
  if (out == nullptr) return SACENV_E_NULL;
  toy_layout(p->n_envs, out);
  return SACENV_OK;
}

int sacenv_toy_init(const SacenvToyParams* p, void* arena, void* stream) {
  const int rc = check_toy(p);
  if (rc) return rc;
  if (arena == nullptr) return SACENV_E_NULL;
  hipLaunchKernelGGL(k_toy_init, dim3(blocks_for(p->n_envs, kWave)), dim3(kWave), 0, (hipStream_t)stream, *p,
                     make_toy_arena(*p, arena), (const int32_t*)nullptr, p->n_envs, 1);
  return launch_status();
}

int sacenv_toy_reset(const SacenvToyParams* p, void* arena, const int32_t* ids, int32_t n_ids, void* stream) {
  const int rc = check_toy(p);
  if (rc) return rc;
  if (arena == nullptr) return SACENV_E_NULL;
  const int n = ids != nullptr ? n_ids : p->n_envs;
  if (n < 0) return SACENV_E_SIZE;
  if (n == 0) return SACENV_OK;
  hipLaunchKernelGGL(k_toy_init, dim3(blocks_for(n, kWave)), dim3(kWave), 0, (hipStream_t)stream, *p,
                     make_toy_arena(*p, arena), ids, n, 0);
  return launch_status();
}

int sacenv_toy_step(const SacenvToyParams* p, void* arena, void* stream) {
  const int rc = check_toy(p);
  if (rc) return rc;
  if (arena == nullptr) return SACENV_E_NULL;
  hipLaunchKernelGGL(k_toy_step, dim3(blocks_for(p->n_envs, kWave)), dim3(kWave), 0, (hipStream_t)stream, *p,
                     make_toy_arena(*p, arena));
  return launch_status();
}

static int mixed_step(const SacenvBoatParams* bp, void* boat_arena, const float* boat_action,
                      const SacenvToyParams* toy_params, void* const* toy_arenas, int32_t n_toys,
                      char* trans, void* stream) {
  MixedLaunch L;
  const int rc = mixed_setup(bp, boat_arena, boat_action, toy_params, toy_arenas, n_toys, 1, &L);
  if (rc) return rc;
  if (L.nb == 0) return SACENV_OK;
  hipLaunchKernelGGL(step_kernel(L.p, true), dim3(L.nb), dim3(kWave), 0, (hipStream_t)stream, L.p, L.A, L.T,
                     boat_action, L.nb_boat, L.M, trans);
  return launch_status();
}

int sacenv_mixed_step(const SacenvBoatParams* bp, void* boat_arena, const float* boat_action,
                      const SacenvToyParams* toy_params, void* const* toy_arenas, int32_t n_toys,
                      void* stream) {
  return mixed_step(bp, boat_arena, boat_action, toy_params, toy_arenas, n_toys, nullptr, stream);
}

int sacenv_mixed_step_pooled(const SacenvBoatParams* bp, void* boat_arena, const float* boat_action,
                             const SacenvToyParams* toy_params, void* const* toy_arenas, int32_t n_toys,
                             void* trans, void* stream) {
  if (bp == nullptr || trans == nullptr) return SACENV_E_NULL;
  if ((reinterpret_cast<uintptr_t>(trans) & 15u) != 0u) return SACENV_E_RANGE;
  return mixed_step(bp, boat_arena, boat_action, toy_params, toy_arenas, n_toys, static_cast<char*>(trans),
                    stream);
}

int sacenv_mixed_segment(const SacenvBoatParams* bp, void* boat_arena, const float* boat_actions,
                         int64_t action_stride, int32_t n_steps, const SacenvToyParams* toy_params,
                         void* const* toy_arenas, int32_t n_toys, void* stream) {
  MixedLaunch L;
  const int rc = mixed_setup(bp, boat_arena, boat_actions, toy_params, toy_arenas, n_toys, n_steps, &L);
  if (rc) return rc;
  RollArgs ra{};
  if (bp != nullptr) {
    if (bp->autoreset && n_steps > SACENV_REFILL_PERIOD) return SACENV_E_SIZE;
    if (action_stride < bp->n_envs) return SACENV_E_RANGE;
    ra = arena_roll_args(L.A);
    ra.act_stride = action_stride;
  }
  if (L.nb == 0) return SACENV_OK;
  // (no boat: p is zeroed and no owner wave runs; the general instantiation)
  hipLaunchKernelGGL(rollout_mixed_kernel(L.p, lean_launch(L.p, ra)), dim3(L.nb), dim3(kWave), 0,
                     (hipStream_t)stream, L.p, L.A, L.T, boat_actions, n_steps, ra, L.nb_boat, L.M);
  return launch_status();
}

int sacenv_boat_wind_eval(const SacenvBoatParams* p, const void* arena, const int32_t* env_ids,
                          const int32_t* idx, int32_t n, double* out_velocity, double* out_angle,
                          void* stream) {
  int rc = check_params(p);
  if (rc) return rc;
  if (!arena || !env_ids || !idx || !out_velocity || !out_angle) return SACENV_E_NULL;
  if (n < 0) return SACENV_E_SIZE;
  if (n == 0) return SACENV_OK;
  void* a = const_cast<void*>(arena);
  hipLaunchKernelGGL(k_wind_eval, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, *p,
                     make_arena(*p, a), make_tail(*p, a), env_ids, idx, n, out_velocity, out_angle);
  return launch_status();
}

}  // extern "C"
