// sacenv_toys.h — the toy envs (parachute, car): their arena layout and device view, one
// loop iteration per step (toy_advance), the one-step and the persistent wave, and the toy
// arenas a mixed launch steps next to the boat (MixedToys).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sacenv.h"
#include "sacenv_boat_arena.h"  // kWave, pad64, align256

#pragma clang fp contract(off)

namespace {

// environment/toy_parachute.py:7-41 and environment/toy_car.py:5-33, one
// env per lane, as vectorised envs: one step = one iteration of the
// script's loop, obs = the signals the script records. The integrators
// (control_blocks.py:5-36) keep their STORED output (clamped to the limits,
// :27-32) but return the unclamped value (:36); the first call returns the
// initial value (:21-22).

constexpr int UT_CNT = 40, UT_CTR = 44, UT_OBS = 56, UT_REW = 64, UT_DONE = 68, UT_TERM = 69,
              UT_FOBS = 70, UT_TOTAL = 78;  // per-env bytes after the 5 f64 state fields

__host__ __device__ inline void toy_layout(int n, SacenvToyLayout* o) {
  const int64_t np = pad64(n);
  o->n_pad = np;
  o->state = 0;
  o->count = UT_CNT * np;
  o->counters = UT_CTR * np;
  o->record = UT_OBS * np;
  o->obs = UT_OBS * np;
  o->reward = UT_REW * np;
  o->done = UT_DONE * np;
  o->term = UT_TERM * np;
  o->final_obs = UT_FOBS * np;
  o->total_bytes = align256(UT_TOTAL * np);
}

struct ToyArena {
  char* b;
  int64_t np;
  __device__ __forceinline__ double* f(int k) const { return reinterpret_cast<double*>(b + 8LL * k * np); }
  __device__ __forceinline__ int32_t* count() const { return reinterpret_cast<int32_t*>(b + UT_CNT * np); }
  __device__ __forceinline__ uint32_t* ctr(int k) const {
    return reinterpret_cast<uint32_t*>(b + UT_CTR * np) + (int64_t)k * np;
  }
  __device__ __forceinline__ float* obs() const { return reinterpret_cast<float*>(b + UT_OBS * np); }
  __device__ __forceinline__ float* reward() const { return reinterpret_cast<float*>(b + UT_REW * np); }
  __device__ __forceinline__ uint8_t* done() const { return reinterpret_cast<uint8_t*>(b + UT_DONE * np); }
  __device__ __forceinline__ uint8_t* term() const { return reinterpret_cast<uint8_t*>(b + UT_TERM * np); }
  __device__ __forceinline__ float* final_obs() const { return reinterpret_cast<float*>(b + UT_FOBS * np); }
};

// the scripts' variables before the loop, and the signals they stand for
__device__ __forceinline__ void toy_initial(const SacenvToyParams& p, double f[5], float obs[2]) {
  for (int k = 0; k < 5; ++k) f[k] = 0.0;
  if (p.kind == SACENV_TOY_PARACHUTE) {
    f[1] = p.h0;  // v_integrator = Integrator(initial_value=h_0) (:21)
    obs[0] = (float)p.h0;
    obs[1] = 0.0f;
  } else {
    obs[0] = 0.0f;
    obs[1] = 0.0f;
  }
}

// one loop iteration; returns the termination code (0: the loop goes on)
__device__ __forceinline__ uint8_t toy_advance(const SacenvToyParams& p, double f[5], int& count,
                                               float obs[2]) {
  const bool first = count == 0;
  uint8_t term = SACENV_TERM_NONE;
  ++count;
  if (p.kind == SACENV_TOY_PARACHUTE) {
    // f = (a_integrator stored output = v, v_integrator stored output = s, total_a, t)
    double total_a = f[2] - p.g;                               // :24
    const double v = first ? 0.0 : total_a * p.integ_dt + f[0];  // :25
    const double s = first ? p.h0 : v * p.integ_dt + f[1];       // :26
    f[0] = v;
    f[1] = s;
    obs[0] = (float)s;
    obs[1] = (float)v;
    if (s < 0.0) {  // :29-30 ground reached: the script breaks
      term = SACENV_TOY_TERM_GROUND;
    } else {
      const double area = s < p.h1 ? p.area_open : p.area_closed;  // :33-36
      const double F_w = v * v * 0.5 * p.rho * p.c_w * area;
      total_a = F_w / p.mass;  // :38
      f[3] = f[3] + p.dt;      // :40
      if (!(f[3] <= p.t_max)) term = SACENV_TERM_TIMEOUT;  // :23
    }
    f[2] = total_a;
  } else {
    // f = (car_angle, a_integrator stored output, v_x / v_y integrator stored outputs, t)
    const double angle = f[0] + p.car_dangle;                          // :24
    const double v = first ? 0.0 : p.car_accel * p.integ_dt + f[1];   // :25
    const double vx = v * cos(angle), vy = v * sin(angle);            // :27-28
    const double sx = first ? 0.0 : vx * p.integ_dt + f[2];           // :30
    const double sy = first ? 0.0 : vy * p.integ_dt + f[3];           // :31
    f[0] = angle;
    f[1] = v >= p.car_v_max ? p.car_v_max : v;  // stored clamp (upper_limit=10, :12)
    f[2] = sx;
    f[3] = sy;
    f[4] = f[4] + p.dt;  // :33
    obs[0] = (float)sx;
    obs[1] = (float)sy;
    if (!(f[4] <= p.t_max)) term = SACENV_TERM_TIMEOUT;  // :22
  }
  return term;
}

// one toy wave: 64 envs, one per lane
__device__ __forceinline__ void toy_wave(const SacenvToyParams& p, const ToyArena& T, int ob, int lane) {
  const int e = ob * kWave + lane;
  if (e >= p.n_envs) return;
  double f[5];
  for (int k = 0; k < 5; ++k) f[k] = T.f(k)[e];
  int count = T.count()[e];
  float obs[2];
  uint8_t term = toy_advance(p, f, count, obs);
  if (term == SACENV_TERM_NONE && p.max_episode_steps > 0 && count >= p.max_episode_steps)
    term = SACENV_TERM_TRUNCATED;
  if (term != SACENV_TERM_NONE) {
    const int c = term == SACENV_TOY_TERM_GROUND ? 0 : term == SACENV_TERM_TIMEOUT ? 1 : 2;
    T.ctr(c)[e] += 1u;
    if (p.autoreset) {
      T.final_obs()[2 * e] = obs[0];
      T.final_obs()[2 * e + 1] = obs[1];
      toy_initial(p, f, obs);
      count = 0;
    }
  }
  for (int k = 0; k < 5; ++k) T.f(k)[e] = f[k];
  T.count()[e] = count;
  reinterpret_cast<float2*>(T.obs())[e] = make_float2(obs[0], obs[1]);
  T.reward()[e] = 0.0f;
  T.done()[e] = term != SACENV_TERM_NONE ? 1 : 0;
  T.term()[e] = term;
}

// n_steps iterations of one toy wave in a persistent launch (sacenv_mixed_segment):
// the state and the iteration count in registers, each step's record (obs,
// reward, done, term) and a restarting lane's terminal obs stored as
// toy_wave stores them, the counters added once at the end. Results equal
// n_steps toy_wave launches bit for bit (the same toy_advance arithmetic).
__device__ __forceinline__ void toy_roll_wave(const SacenvToyParams& p, const ToyArena& T, int ob, int lane,
                                              int n_steps) {
  const int e = ob * kWave + lane;
  if (e >= p.n_envs) return;
  double f[5];
  for (int k = 0; k < 5; ++k) f[k] = T.f(k)[e];
  int count = T.count()[e];
  uint32_t ends[3] = {0u, 0u, 0u};
  for (int ks = 0; ks < n_steps; ++ks) {
    float obs[2];
    uint8_t term = toy_advance(p, f, count, obs);
    if (term == SACENV_TERM_NONE && p.max_episode_steps > 0 && count >= p.max_episode_steps)
      term = SACENV_TERM_TRUNCATED;
    if (term != SACENV_TERM_NONE) {
      ++ends[term == SACENV_TOY_TERM_GROUND ? 0 : term == SACENV_TERM_TIMEOUT ? 1 : 2];
      if (p.autoreset) {
        reinterpret_cast<float2*>(T.final_obs())[e] = make_float2(obs[0], obs[1]);
        toy_initial(p, f, obs);
        count = 0;
      }
    }
    reinterpret_cast<float2*>(T.obs())[e] = make_float2(obs[0], obs[1]);
    T.reward()[e] = 0.0f;
    T.done()[e] = term != SACENV_TERM_NONE ? 1 : 0;
    T.term()[e] = term;
  }
  for (int k = 0; k < 5; ++k) T.f(k)[e] = f[k];
  T.count()[e] = count;
  for (int c = 0; c < 3; ++c)
    if (ends[c] != 0u) T.ctr(c)[e] += ends[c];
}

// toy arenas stepped inside a mixed launch
struct MixedToys {
  SacenvToyParams p[2];
  ToyArena a[2];
  int nb[2];
  int n;
};

}  // namespace
