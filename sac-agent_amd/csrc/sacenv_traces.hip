// sacenv_traces.hip — gfx950 episode traces (include/sacenv_traces.h): the rows of each
// member's best episode, kept on the device from the step records.
//
// The working store holds the last S = max_steps + call_steps steps of every env, one slot
// per step (global step u lives in slot (u - (step0 - 1)) mod S):
//     obs f32 [n_pad][11] | action f32 [n_pad] | reward f32 [n_pad]
// which is what the step wrote, as it lies: a wave appends a step with thirteen 256-B row
// copies (eleven of its 2 816 obs bytes, one action row, one reward row). No row per lane at a
// per-env position: 64 lanes storing to 64 different rows run at about 1/17 of that rate, and
// the append is the per-step path. Reading ONE env's values back out of the slots is the rare
// path (a new best) and is left to the pick launch.
//
// Two launches per update, one lane per env, one wave per 64 envs:
//   k_tr_walk  walks the K steps with the carry in registers, as k_ep_emit of
//              sacenv_episodes.hip does (the same f64 add per step from the same f32 record,
//              so the same scores, bit for bit; the two statements are restated here, the
//              rest of that kernel's step is the log's position arithmetic), kTrUnroll steps'
//              loads in flight, all unconditional. It copies every step into its slot. Each
//              lane keeps its env's candidate -- an env's endings come in step order, so
//              `score > candidate` keeps the first greatest -- and the wave reduces the 64
//              candidates once, at the end, under the total order (score descending, end_step,
//              env): one candidate per wave. At a step with an ending in the wave (a wave-
//              uniform branch, rarely taken) the wave also reduces the ending scores to their
//              maximum; lane 0 stores that, or NaN for "none", per (step, wave).
//   k_tr_pick  one workgroup per member: the first greatest of its waves' candidates; the
//              count of steps at which the per-step maxima beat the running best (`replaced`,
//              the same however the steps are split into calls); and only if the candidate
//              beats the stored score, the episode's rows out of the slots, the last row from
//              final_obs, the header last. Members without a winner touch nothing.
//
// The ordering hazard. Within one call an env can end more than once, and the winner may be
// the earlier ending; the walk has then long since appended the later episode's steps. That
// is safe because a slot belongs to a STEP, not to an episode: nothing an episode's later
// steps write can land on its earlier ones, except by a wrap of the store. A call of K <=
// call_steps steps starting at global step s writes steps s .. s + K - 1; the oldest step a
// winner that ended at t >= s can need is t - max_steps >= s - max_steps (row 0 or, of a
// longer episode, row L - max_steps). Step u overwrites step u - S, so nothing needed is
// overwritten while s + K - 1 - S < s - max_steps, i.e. S >= max_steps + K: hence
// "append everything, then copy" with S = max_steps + call_steps, and hence n_steps >
// call_steps is an error.
// No atomics: the member buffer's bytes are the same from run to run.

#include "sacenv_traces.h"
#include "sacenv_wave_core.h"
#include "sacenv_traces_frames.h"   // the episode frames' kernels (include/sacenv_frames.h); their entry points are below

namespace {

constexpr int kObs = SACENV_OBS_DIM;
constexpr int kTrUnroll = 4;        // steps whose loads (15 per lane and step) are in flight together
constexpr int kPickThreads = 256;
constexpr int kPickWaves = kPickThreads / kWave;
constexpr int kCandBytes = 32;      // one wave's candidate: i64 end_step | f64 score | i32 env | i32 length | u32 term | 0
constexpr int kRowWords = SACENV_TRACE_ROW_BYTES / 4;
static_assert(SACENV_TRACE_STEP_BYTES == 4 * (kObs + 2), "a slot holds the obs block and two columns");
static_assert(sizeof(SacenvTraceHeader) == SACENV_TRACE_HEADER_BYTES, "the member buffer's header");

// the working store: candidates [n_waves] | step maxima f64 [call_steps][n_waves] | carry score
// f64 [n_pad] | carry length i32 [n_pad] | S slots
struct Store {
  int64_t cand, cell, carry_score, carry_len, slots, slot_bytes, total;
  int32_t S;
};

__host__ __device__ inline Store store_layout(const int32_t n_pad, const int32_t max_steps, const int32_t call_steps) {
  Store l;
  const int64_t n_waves = n_pad / kWave;
  l.S = max_steps + call_steps;
  l.cand = 0;
  l.cell = l.cand + kCandBytes * n_waves;
  l.carry_score = l.cell + (8 * (int64_t)call_steps * n_waves + 15) / 16 * 16;
  l.carry_len = l.carry_score + 8 * (int64_t)n_pad;
  l.slots = l.carry_len + 4 * (int64_t)n_pad;
  l.slot_bytes = (int64_t)SACENV_TRACE_STEP_BYTES * n_pad;
  l.total = l.slots + l.slot_bytes * l.S;
  return l;
}

inline int64_t member_stride(const int32_t max_steps) {
  return SACENV_TRACE_HEADER_BYTES + (int64_t)SACENV_TRACE_ROW_BYTES * ((int64_t)max_steps + 1);
}

// what the kernels need of the two descriptors, the columns as pointers to env 0 of step 0
struct Tr {
  const char* obs;
  const char* reward;
  const uint8_t* done;
  const uint8_t* term;
  const float* actions;
  const char* final_obs;
  char* members;
  char* store;
  int64_t stride, final_stride;
  int64_t step;        // global number of the call's first step
  int64_t attach;      // step0 of the descriptor
  int64_t member_bytes;
  int32_t slot0;       // the slot of the call's first step
  int32_t n_envs, n_pad, n_waves, n_steps, owned, epm, env_base, R, call_steps;
};

__device__ __forceinline__ bool cand_better(const double xs, const int64_t xt, const int32_t xe, const double ys,
                                            const int64_t yt, const int32_t ye) {
  // x, y: candidates; env < 0 = none. Scores of candidates are never NaN.
  if (xe < 0) return false;
  if (ye < 0) return true;
  return xs > ys || (xs == ys && (xt < yt || (xt == yt && xe < ye)));
}

struct Lane {
  double score;        // the carry
  int32_t len;
  double best;         // the lane's candidate
  int64_t best_step;
  int32_t best_len, best_env;   // best_env < 0: none
  uint32_t best_term;
};

// One step of the walk for one lane: the f64 add and the length as in sacenv_episodes.hip;
// where the wave has an ending, the lane's candidate and the wave's maximum of the step.
__device__ __forceinline__ double tr_step(Lane& s, const int64_t step, const int32_t e, const float r,
                                          const bool ended, const uint32_t term) {
  s.score = s.score + (double)r;
  ++s.len;
  double vmax = __builtin_nan("");
  if (__ballot(ended) != 0ull) {
    if (ended) {
      if (s.score == s.score) {                       // a NaN score never wins
        vmax = s.score;
        if (s.best_env < 0 || s.score > s.best) {
          s.best = s.score;
          s.best_step = step;
          s.best_len = s.len;
          s.best_env = e;
          s.best_term = term;
        }
      }
      s.score = 0.0;
      s.len = 0;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) vmax = fmax(vmax, __shfl_xor(vmax, o));   // (fmax drops a NaN operand)
  }
  return vmax;
}

__global__ __launch_bounds__(kWave) void k_tr_walk(const Tr a) {
  const int lane = threadIdx.x;
  const int w = blockIdx.x;
  const int e = w * kWave + lane;
  const bool owned = e < a.owned;
  const int el = min(e, a.n_envs - 1);
  const Store l = store_layout(a.n_pad, a.R, a.call_steps);
  double* __restrict__ carry_score = reinterpret_cast<double*>(a.store + l.carry_score);
  int32_t* __restrict__ carry_len = reinterpret_cast<int32_t*>(a.store + l.carry_len);
  double* __restrict__ cell = reinterpret_cast<double*>(a.store + l.cell) + w;
  Lane s;
  s.score = carry_score[el];
  s.len = carry_len[el];
  s.best = 0.0;
  s.best_step = 0;
  s.best_len = 0;
  s.best_env = -1;
  s.best_term = 0u;
  // the wave's obs block is dwords [704 w, 704 w + 704) of the record's obs: lane + 64 j
  int64_t od[kObs], odc[kObs];
  const int64_t last = (int64_t)a.n_envs * kObs - 1;
#pragma unroll
  for (int j = 0; j < kObs; ++j) {
    od[j] = (int64_t)w * (kWave * kObs) + lane + kWave * j;
    odc[j] = od[j] < last ? od[j] : last;               // columns of envs >= n_envs are never read
  }
  const char* __restrict__ rp = a.reward + 4 * (int64_t)el;
  const uint8_t* __restrict__ dp = a.done + el;
  const uint8_t* __restrict__ tp = a.term + el;
  const float* __restrict__ ap = a.actions + el;
  int32_t slot = a.slot0;
  int k = 0;
  for (; k + kTrUnroll <= a.n_steps; k += kTrUnroll) {
    float o[kTrUnroll][kObs], r[kTrUnroll], ac[kTrUnroll];
    uint8_t d[kTrUnroll], tm[kTrUnroll];
#pragma unroll
    for (int u = 0; u < kTrUnroll; ++u) {
      const int64_t off = (int64_t)(k + u) * a.stride;
      const float* __restrict__ op = reinterpret_cast<const float*>(a.obs + off);
#pragma unroll
      for (int j = 0; j < kObs; ++j) o[u][j] = op[odc[j]];
      r[u] = *reinterpret_cast<const float*>(rp + off);
      ac[u] = ap[(int64_t)(k + u) * a.n_envs];
      d[u] = dp[off];
      tm[u] = tp[off];
    }
#pragma unroll
    for (int u = 0; u < kTrUnroll; ++u) {
      float* __restrict__ sp = reinterpret_cast<float*>(a.store + l.slots + l.slot_bytes * slot);
#pragma unroll
      for (int j = 0; j < kObs; ++j) sp[od[j]] = o[u][j];
      sp[(int64_t)kObs * a.n_pad + e] = ac[u];
      sp[(int64_t)(kObs + 1) * a.n_pad + e] = r[u];
      const double v = tr_step(s, a.step + k + u, e, r[u], owned && d[u] != 0, tm[u]);
      if (lane == 0) cell[(int64_t)(k + u) * a.n_waves] = v;
      slot = slot + 1 == l.S ? 0 : slot + 1;
    }
  }
  for (; k < a.n_steps; ++k) {  // the last K mod kTrUnroll steps
    const int64_t off = (int64_t)k * a.stride;
    const float* __restrict__ op = reinterpret_cast<const float*>(a.obs + off);
    float* __restrict__ sp = reinterpret_cast<float*>(a.store + l.slots + l.slot_bytes * slot);
    float o[kObs];
#pragma unroll
    for (int j = 0; j < kObs; ++j) o[j] = op[odc[j]];
    const float r = *reinterpret_cast<const float*>(rp + off);
    const float ac = ap[(int64_t)k * a.n_envs];
    const uint8_t d = dp[off], tm = tp[off];
#pragma unroll
    for (int j = 0; j < kObs; ++j) sp[od[j]] = o[j];
    sp[(int64_t)kObs * a.n_pad + e] = ac;
    sp[(int64_t)(kObs + 1) * a.n_pad + e] = r;
    const double v = tr_step(s, a.step + k, e, r, owned && d != 0, tm);
    if (lane == 0) cell[(int64_t)k * a.n_waves] = v;
    slot = slot + 1 == l.S ? 0 : slot + 1;
  }
  if (e < a.n_envs) {
    carry_score[e] = s.score;
    carry_len[e] = s.len;
  }
  // the wave's candidate: the first greatest of the lanes'
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const double os = __shfl_xor(s.best, o);
    const int64_t ot = __shfl_xor((long long)s.best_step, o);
    const int32_t ol = __shfl_xor(s.best_len, o), oe = __shfl_xor(s.best_env, o);
    const uint32_t om = __shfl_xor(s.best_term, o);
    if (cand_better(os, ot, oe, s.best, s.best_step, s.best_env)) {
      s.best = os;
      s.best_step = ot;
      s.best_len = ol;
      s.best_env = oe;
      s.best_term = om;
    }
  }
  if (lane == 0) {
    char* c = a.store + l.cand + (int64_t)kCandBytes * w;
    store16(c, (uint64_t)s.best_step, (uint64_t)__double_as_longlong(s.best));
    store16(c + 16, pack32(s.best_env, s.best_len), s.best_term);
  }
}

__global__ __launch_bounds__(kPickThreads) void k_tr_pick(const Tr a) {
  __shared__ double w_score[kPickWaves], stepmax[kPickThreads];
  __shared__ int64_t w_step[kPickWaves];
  __shared__ int32_t w_env[kPickWaves], w_len[kPickWaves];
  __shared__ uint32_t w_term[kPickWaves];
  __shared__ int64_t s_replaced;

  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  const int m = blockIdx.x;
  const Store l = store_layout(a.n_pad, a.R, a.call_steps);
  const int w0 = (int)((int64_t)m * a.epm / kWave);
  const int nw = min((a.epm + kWave - 1) / kWave, a.n_waves - w0);
  SacenvTraceHeader* __restrict__ hdr = reinterpret_cast<SacenvTraceHeader*>(a.members + (int64_t)m * a.member_bytes);
  const bool empty = hdr->rows == 0;
  const double stored = hdr->score;

  // the first greatest of the member's waves' candidates
  double bs = 0.0;
  int64_t bt = 0;
  int32_t be = -1, bl = 0;
  uint32_t bm = 0u;
  for (int i = t; i < nw; i += kPickThreads) {
    const char* c = a.store + l.cand + (int64_t)kCandBytes * (w0 + i);
    const ulong2 c0 = *reinterpret_cast<const ulong2*>(c), c1 = *reinterpret_cast<const ulong2*>(c + 16);
    const double xs = __longlong_as_double((long long)c0.y);
    const int64_t xt = (int64_t)c0.x;
    const int32_t xe = (int32_t)(uint32_t)c1.x, xl = (int32_t)(uint32_t)(c1.x >> 32);
    if (cand_better(xs, xt, xe, bs, bt, be)) {
      bs = xs;
      bt = xt;
      be = xe;
      bl = xl;
      bm = (uint32_t)c1.y;
    }
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const double os = __shfl_xor(bs, o);
    const int64_t ot = __shfl_xor((long long)bt, o);
    const int32_t oe = __shfl_xor(be, o), ol = __shfl_xor(bl, o);
    const uint32_t om = __shfl_xor(bm, o);
    if (cand_better(os, ot, oe, bs, bt, be)) {
      bs = os;
      bt = ot;
      be = oe;
      bl = ol;
      bm = om;
    }
  }
  if (lane == 0) {
    w_score[wv] = bs;
    w_step[wv] = bt;
    w_env[wv] = be;
    w_len[wv] = bl;
    w_term[wv] = bm;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPickWaves; ++j) {   // every thread: the same winner
    if (cand_better(w_score[j], w_step[j], w_env[j], bs, bt, be)) {
      bs = w_score[j];
      bt = w_step[j];
      be = w_env[j];
      bl = w_len[j];
      bm = w_term[j];
    }
  }
  const bool win = be >= 0 && (empty || bs > stored);
  if (!win) return;   // (uniform over the workgroup)

  // `replaced`: the steps whose maximum beat the running best, kPickThreads steps at a time;
  // wave wv reduces the steps wv, wv + 4, .. of a chunk over the member's waves
  const double* __restrict__ cell = reinterpret_cast<const double*>(a.store + l.cell) + w0;
  if (t == 0) s_replaced = 0;
  double run = stored;
  bool none = empty;
  for (int k0 = 0; k0 < a.n_steps; k0 += kPickThreads) {
    const int n = min(kPickThreads, a.n_steps - k0);
    for (int k = wv; k < n; k += kPickWaves) {
      double v = __builtin_nan("");
      for (int i = lane; i < nw; i += kWave) v = fmax(v, cell[(int64_t)(k0 + k) * a.n_waves + i]);
#pragma unroll
      for (int o = kWave / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
      if (lane == 0) stepmax[k] = v;
    }
    __syncthreads();
    if (t == 0) {
      int64_t c = 0;
      for (int k = 0; k < n; ++k) {
        const double v = stepmax[k];
        if (v == v && (none || v > run)) {
          run = v;
          none = false;
          ++c;
        }
      }
      s_replaced += c;
    }
    __syncthreads();
  }

  // the rows: first_row .. L of the episode that ended at step bt with length bl
  const int64_t L = bl;
  int64_t first = L > a.R ? L - a.R : 0;
  const int64_t q = a.attach - (bt - L);   // steps before the first one the keeper saw, + 1
  if (q > 1 && q > first) first = q;
  const int32_t rows = (int32_t)(L - first + 1);
  uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(hdr) + SACENV_TRACE_HEADER_BYTES);
  for (int i = t; i < (a.R + 1) * kRowWords; i += kPickThreads) {
    if (i >= rows * kRowWords) {   // nothing of an earlier, longer best stays behind
      out[i] = 0u;
      continue;
    }
    const int word = i % kRowWords;
    const int64_t jr = first + i / kRowWords;
    const int64_t u = bt - L + jr;                           // the row's global step, >= attach - 1
    const uint32_t* __restrict__ sp =
        reinterpret_cast<const uint32_t*>(a.store + l.slots + l.slot_bytes * ((u - (a.attach - 1)) % l.S));
    uint32_t v = 0u;
    if (word < kObs) {
      if (jr == L)
        v = reinterpret_cast<const uint32_t*>(a.final_obs + (bt - a.step) * a.final_stride)[(int64_t)be * kObs + word];
      else
        v = sp[(int64_t)be * kObs + word];
    } else if (word < kObs + 2 && jr != 0) {
      v = sp[(int64_t)(word) * a.n_pad + be];               // action at 11 n_pad, reward at 12 n_pad
    }
    out[i] = v;
  }
  __syncthreads();
  if (t == 0) {   // the header last
    const int64_t replaced = hdr->replaced + s_replaced;
    store16(&hdr->end_step, (uint64_t)bt, (uint64_t)__double_as_longlong(bs));
    store16(&hdr->env, pack32(a.env_base + be, bl), pack32((int32_t)bm, rows));
    store16(&hdr->first_row, pack32((int32_t)first, 0), (uint64_t)replaced);
  }
}

// the empty state: headers and zeroed rows, the carry, and the slot before step0 (slot 0)
__global__ __launch_bounds__(256) void k_tr_init(const Tr a, const float* __restrict__ obs,
                                                 const double* __restrict__ carry_score,
                                                 const int32_t* __restrict__ carry_len, const int32_t members) {
  const Store l = store_layout(a.n_pad, a.R, a.call_steps);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t mwords = a.member_bytes / 8;
  uint64_t* __restrict__ mb = reinterpret_cast<uint64_t*>(a.members);
  for (int64_t i = first; i < mwords * members; i += stride) {
    const int64_t f = i % mwords;
    uint64_t v = 0;
    if (f == 0) v = ~0ull;                                                     // end_step = -1
    if (f == 1) v = (uint64_t)__double_as_longlong(-__builtin_inf());          // score
    if (f == 2) v = pack32(-1, 0);                                             // env = -1, length = 0
    mb[i] = v;
  }
  double* __restrict__ cs = reinterpret_cast<double*>(a.store + l.carry_score);
  int32_t* __restrict__ cl = reinterpret_cast<int32_t*>(a.store + l.carry_len);
  float* __restrict__ sp = reinterpret_cast<float*>(a.store + l.slots);
  for (int64_t i = first; i < a.n_pad; i += stride) {
    const bool in = i < a.n_envs;
    cs[i] = in && carry_score != nullptr ? carry_score[i] : 0.0;
    cl[i] = in && carry_len != nullptr ? carry_len[i] : 0;
    sp[(int64_t)kObs * a.n_pad + i] = 0.0f;
    sp[(int64_t)(kObs + 1) * a.n_pad + i] = 0.0f;
  }
  for (int64_t i = first; i < (int64_t)a.n_pad * kObs; i += stride)
    sp[i] = obs != nullptr && i < (int64_t)a.n_envs * kObs ? obs[i] : 0.0f;
}

int check_traces(const SacenvTraces* t) {
  if (t == nullptr) return SACENV_E_NULL;
  if (t->n_envs < 1 || t->n_pad < t->n_envs || t->n_pad % kWave != 0 || t->env_base < 0 ||
      (int64_t)t->env_base + t->n_envs > INT32_MAX || t->members < 1 || t->members > SACENV_TRACES_MAX_MEMBERS ||
      t->envs_per_member < 1 || t->max_steps < 1 || t->max_steps > SACENV_TRACES_MAX_STEPS || t->call_steps < 1 ||
      t->call_steps > SACENV_TRACES_MAX_STEPS || t->step0 < 0)
    return SACENV_E_SIZE;
  if (t->members > 1 && t->envs_per_member % kWave != 0) return SACENV_E_SIZE;
  if ((int64_t)t->members * t->envs_per_member > t->n_envs) return SACENV_E_SIZE;
  return SACENV_OK;
}

Tr make_tr(const SacenvTraces* t, void* member_buf, void* store) {
  Tr a = {};
  a.members = static_cast<char*>(member_buf);
  a.store = static_cast<char*>(store);
  a.attach = t->step0;
  a.member_bytes = member_stride(t->max_steps);
  a.n_envs = t->n_envs;
  a.n_pad = t->n_pad;
  a.n_waves = t->n_pad / kWave;
  const int64_t owned = (int64_t)t->members * t->envs_per_member;
  a.owned = (int32_t)(owned < t->n_envs ? owned : t->n_envs);
  a.epm = t->envs_per_member;
  a.env_base = t->env_base;
  a.R = t->max_steps;
  a.call_steps = t->call_steps;
  return a;
}

// ---- the episode frames (include/sacenv_frames.h; the kernels are in sacenv_traces_frames.h)

inline bool fr_finite(const float v) { return v - v == 0.0f; }

int check_frames(const SacenvFrames* f) {
  if (f == nullptr) return SACENV_E_NULL;
  if (f->width < SACENV_FRAMES_MIN_DIM || f->width > SACENV_FRAMES_MAX_DIM || f->width % 4 != 0 ||
      f->height < SACENV_FRAMES_MIN_DIM || f->height > SACENV_FRAMES_MAX_DIM || f->strip < 2 ||
      f->height - f->strip < 8 || f->members < 1 || f->members > SACENV_TRACES_MAX_MEMBERS || f->max_steps < 1 ||
      f->max_steps > SACENV_TRACES_MAX_STEPS || f->rad < 1 || f->rad > SACENV_FRAMES_MAX_RAD || f->boat_len < 1 ||
      f->boat_len > SACENV_FRAMES_MAX_BOAT || f->boat_half < 1 || f->boat_half > SACENV_FRAMES_MAX_BOAT)
    return SACENV_E_SIZE;
  if (!fr_finite(f->x0) || !fr_finite(f->y0) || !fr_finite(f->scale_x) || !fr_finite(f->scale_y) || !(f->scale_x > 0.0f) ||
      !(f->scale_y > 0.0f) || !fr_finite(f->goal_line) || !fr_finite(f->track_width))
    return SACENV_E_RANGE;
  return SACENV_OK;
}

}  // namespace

extern "C" {

int sacenv_traces_bytes(const SacenvTraces* t, int64_t* member_bytes, int64_t* store_bytes) {
  const int rc = check_traces(t);
  if (rc) return rc;
  if (member_bytes == nullptr || store_bytes == nullptr) return SACENV_E_NULL;
  *member_bytes = member_stride(t->max_steps) * t->members;
  *store_bytes = store_layout(t->n_pad, t->max_steps, t->call_steps).total;
  return SACENV_OK;
}

int sacenv_traces_init(const SacenvTraces* t, const float* obs, const double* carry_score, const int32_t* carry_length,
                       void* member_buf, void* store, void* stream) {
  const int rc = check_traces(t);
  if (rc) return rc;
  if (member_buf == nullptr || store == nullptr) return SACENV_E_NULL;
  if ((uintptr_t)member_buf % 16 != 0 || (uintptr_t)store % 16 != 0 || (uintptr_t)obs % 4 != 0 ||
      (uintptr_t)carry_score % 8 != 0 || (uintptr_t)carry_length % 4 != 0)
    return SACENV_E_RANGE;
  const Tr a = make_tr(t, member_buf, store);
  const int64_t items = (int64_t)t->n_pad * kObs;
  const int64_t blocks = (items + 255) / 256;
  hipLaunchKernelGGL(k_tr_init, dim3((uint32_t)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, (hipStream_t)stream, a,
                     obs, carry_score, carry_length, t->members);
  return status();
}

int sacenv_traces_update(const SacenvTraces* t, const SacenvTraceSteps* s, const void* records, const float* actions,
                         const void* final_obs, void* member_buf, void* store, void* stream) {
  const int rc = check_traces(t);
  if (rc) return rc;
  if (s == nullptr || records == nullptr || actions == nullptr || final_obs == nullptr || member_buf == nullptr ||
      store == nullptr)
    return SACENV_E_NULL;
  if (s->n_steps < 1 || s->n_steps > t->call_steps) return SACENV_E_SIZE;
  if (s->obs_off < 0 || s->reward_off < 0 || s->done_off < 0 || s->term_off < 0 || s->rec_stride < 0 ||
      s->final_stride < 0 || s->step < t->step0 || s->obs_off % 4 != 0 || s->reward_off % 4 != 0)
    return SACENV_E_RANGE;
  if (s->n_steps > 1 && (s->rec_stride == 0 || s->rec_stride % 4 != 0 || s->final_stride == 0 || s->final_stride % 4 != 0))
    return SACENV_E_RANGE;
  if ((uintptr_t)records % 4 != 0 || (uintptr_t)actions % 4 != 0 || (uintptr_t)final_obs % 4 != 0 ||
      (uintptr_t)member_buf % 16 != 0 || (uintptr_t)store % 16 != 0)
    return SACENV_E_RANGE;
  Tr a = make_tr(t, member_buf, store);
  const char* rec = static_cast<const char*>(records);
  a.obs = rec + s->obs_off;
  a.reward = rec + s->reward_off;
  a.done = reinterpret_cast<const uint8_t*>(rec + s->done_off);
  a.term = reinterpret_cast<const uint8_t*>(rec + s->term_off);
  a.actions = actions;
  a.final_obs = static_cast<const char*>(final_obs);
  a.stride = s->rec_stride;
  a.final_stride = s->final_stride;
  a.step = s->step;
  a.n_steps = s->n_steps;
  a.slot0 = (int32_t)((s->step - (t->step0 - 1)) % ((int64_t)t->max_steps + t->call_steps));
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_tr_walk, dim3((uint32_t)a.n_waves), dim3(kWave), 0, st, a);
  hipLaunchKernelGGL(k_tr_pick, dim3((uint32_t)t->members), dim3(kPickThreads), 0, st, a);
  return status();
}

int sacenv_frames_bytes(const SacenvFrames* f, int64_t* scratch_bytes, int64_t* frame_bytes) {
  const int rc = check_frames(f);
  if (rc) return rc;
  if (scratch_bytes == nullptr || frame_bytes == nullptr) return SACENV_E_NULL;
  *scratch_bytes = fr_map_off(f->max_steps, f->width) + 4 * (int64_t)f->width * (f->height - f->strip);
  *frame_bytes = (int64_t)f->width * f->height;
  return SACENV_OK;
}

int sacenv_frames_render(const SacenvFrames* f, const void* member_buf, int32_t member, int64_t first_frame,
                         int32_t every, int32_t n_frames, void* out, void* scratch, void* stream) {
  const int rc = check_frames(f);
  if (rc) return rc;
  if (member_buf == nullptr || out == nullptr || scratch == nullptr) return SACENV_E_NULL;
  if (member < 0 || member >= f->members || every < 1 || n_frames < 1 || n_frames > SACENV_FRAMES_MAX_FRAMES)
    return SACENV_E_SIZE;
  if (first_frame < 0 || first_frame > ((int64_t)1 << 62) || (uintptr_t)member_buf % 16 != 0 ||
      (uintptr_t)scratch % 16 != 0 || (uintptr_t)out % 4 != 0)
    return SACENV_E_RANGE;
  Fr a = {};
  a.member = static_cast<const char*>(member_buf) + member_stride(f->max_steps) * member;
  a.scratch = static_cast<char*>(scratch);
  a.out = static_cast<uint8_t*>(out);
  a.first_frame = first_frame;
  a.W = f->width;
  a.H = f->height;
  a.S = f->strip;
  a.HP = f->height - f->strip;
  a.R = f->max_steps;
  a.rad = f->rad;
  a.rad2 = f->rad * f->rad;
  a.boat_len = f->boat_len;
  a.boat_half = f->boat_half;
  a.every = every;
  a.n_frames = n_frames;
  a.blocks_per_frame = (a.H * (a.W / 4) + 255) / 256;   // <= 1024, times n_frames <= 2^20: a grid.x below 2^31
  a.inv_wq = fr_inverse((uint32_t)(a.W / 4));
  a.inv_hp = fr_inverse((uint32_t)a.HP);
  a.x0 = f->x0;
  a.y0 = f->y0;
  a.sx = f->scale_x;
  a.sy = f->scale_y;
  a.goal_line = f->goal_line;
  a.track_width = f->track_width;
  FrDir dir;
  static_assert(sizeof(dir.v) == sizeof(f->dir), "the direction table goes to the points launch by value");
  memcpy(dir.v, f->dir, sizeof(dir.v));
  const hipStream_t st = (hipStream_t)stream;
  const int32_t items = a.R + 1 > a.W ? a.R + 1 : a.W;   // a thread per row and per strip column
  hipLaunchKernelGGL(k_fr_points, dim3((uint32_t)((items + 255) / 256)), dim3(256), 0, st, a, dir);
  hipLaunchKernelGGL(k_fr_cover, dim3((uint32_t)((a.W + kFrTile - 1) / kFrTile), (uint32_t)((a.HP + kFrTile - 1) / kFrTile)),
                     dim3(kFrThreads), 0, st, a);
  hipLaunchKernelGGL(k_fr_compose, dim3((uint32_t)a.blocks_per_frame * (uint32_t)n_frames), dim3(256), 0, st, a);
  return status();
}

}  // extern "C"
