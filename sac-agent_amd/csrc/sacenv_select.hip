// sacenv_select.hip — gfx950 population selection (include/sacenv_selection.h): the worst q
// ready members of a search become copies of the best q, with perturbed values.
//
// Two launches:
//   k_select_decide  one wave, lane m for member m (P <= 64). Each lane reads its member's
//                    episodes and look-back mean from the board and its record from the state;
//                    the ranks come from a 64-step loop in which step j compares every lane's
//                    mean with lane j's (a wave-shared value: one lane read per step, no LDS).
//                    Losers draw their source with one Philox block, take its values from LDS
//                    (every lane's values as they stood before the call) and write their
//                    record; lane 0 commits the header.
//   k_select_copy    grid (chunks, P): the workgroups of a member whose source_now is < 0 exit
//                    at once; the others copy the source's slab over the member's, 16 B per lane
//                    and access, as k_board_finish (sacenv_board.hip) copies a snapshot.
// No atomics: the state's and the slabs' bytes are the same from run to run.

#include <math.h>

#include "sacenv_board_core.h"
#include "sacenv_philox.h"
#include "sacenv_selection.h"
#include "sacenv_wave_core.h"

namespace {

constexpr int kMaxP = SACENV_SELECT_MAX_MEMBERS;
constexpr int kCopyThreads = SACENV_SELECT_COPY_THREADS;
constexpr int kCopyChunks = SACENV_SELECT_COPY_CHUNKS;

static_assert(kMaxP == kWave, "one lane per member");
static_assert(SACENV_SELECT_COPY_UNROLL == kSlabLoads, "the header's grid rule is slab_copy's");
static_assert(kMaxP <= SACENV_BOARD_MAX_MEMBERS, "the board holds every member");
static_assert(sizeof(SacenvSelectMember) == SACENV_SELECT_MEMBER_BYTES, "the member record is 64 B");
static_assert(SACENV_SELECT_HEADER_BYTES % 16 == 0 && SACENV_SELECT_MEMBER_BYTES % 16 == 0, "16-B records");
static_assert(sizeof(SacenvSelect) == 120, "SacenvSelect is 120 B");

// what the decision needs of SacenvSelect (kernel argument)
struct Decide {
  const char* board;
  char* state;
  int64_t min_episodes;
  uint64_t seed;
  double factor[2], lo[4], hi[4];
  int32_t members, quantile;
};

// the initial values of every member (kernel argument, 2 KB)
struct Initial {
  double hp[kMaxP][4];
};

__device__ __forceinline__ SacenvSelectMember* select_member(char* state, const int m) {
  return reinterpret_cast<SacenvSelectMember*>(state + SACENV_SELECT_HEADER_BYTES) + m;
}

// lane j's value for every lane (j the same in all lanes: two v_readlane, no LDS)
__device__ __forceinline__ double lane_value(const double x, const int j) {
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, j);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), j);
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

__global__ __launch_bounds__(kWave) void k_select_decide(const Decide a) {
  __shared__ double hp_before[kMaxP][4];   // every member's values as they stood before the call
  __shared__ int32_t by_rank[kMaxP];       // the ready member of each rank

  const int m = threadIdx.x;
  const bool member = m < a.members;
  const int mc = member ? m : a.members - 1;   // lanes past P read the last member's and write nothing
  const SacenvBoardMember* __restrict__ brec =
      reinterpret_cast<const SacenvBoardMember*>(a.board + SACENV_BOARD_HEADER_BYTES) + mc;
  SacenvSelectMember* __restrict__ rec = select_member(a.state, mc);
  int64_t* __restrict__ hdr = reinterpret_cast<int64_t*>(a.state);

  const int64_t round = hdr[0], replaced_total = hdr[1];
  const int64_t episodes = brec->episodes;
  const double avg = brec->avg;
  const int64_t since = rec->since, replaced = rec->replaced;
  const int32_t parent = rec->parent;
  double hp[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) hp_before[m][k] = hp[k] = rec->hp[k];

  // 1: ready
  const bool ready = member && episodes - since >= a.min_episodes && avg == avg;
  const uint64_t ready_mask = __ballot(ready);
  const int R = __popcll(ready_mask);

  // 2: rank = the ready members ahead of this one. Step j holds every lane's mean against lane
  // j's, a wave-shared value
  int32_t rank = 0;
#pragma unroll 8
  for (int j = 0; j < kWave; ++j) {
    const double aj = lane_value(avg, j);
    const bool rj = (ready_mask >> j) & 1ull;
    rank += (rj && (aj > avg || (aj == avg && j < m))) ? 1 : 0;
  }
  if (ready) by_rank[rank] = m;
  __syncthreads();

  // 3: with R >= 2 q the last q ranks lose to the first q
  const int q = a.quantile;
  const bool loser = ready && R >= 2 * q && rank >= R - q;
  const uint64_t loser_mask = __ballot(loser);

  int32_t source = -1;
  if (loser) {
    // 4: the source
    uint64_t w[4] = {(uint64_t)m, (uint64_t)round, 0ull, 0ull};
    philox4x64_10(w, a.seed, SACENV_SELECT_KEY1);
    const uint64_t j = ((w[0] >> 32) * (uint64_t)q) >> 32;
    source = by_rank[j];
    // 5: its values, each times one of the two factors, clipped
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double v = hp_before[source][k] * a.factor[(w[1] >> k) & 1ull];
      if (v < a.lo[k]) v = a.lo[k];
      if (v > a.hi[k]) v = a.hi[k];
      hp[k] = v;
    }
  }

  // 6: the record, four 16-B stores
  if (member) {
    char* out = reinterpret_cast<char*>(rec);
    store16(out, (uint64_t)(loser ? episodes : since), (uint64_t)(replaced + (loser ? 1 : 0)));
    store16(out + 16, pack32(source, ready ? rank : -1), pack32(loser ? source : parent, 0));
    store16(out + 32, (uint64_t)__double_as_longlong(hp[0]), (uint64_t)__double_as_longlong(hp[1]));
    store16(out + 48, (uint64_t)__double_as_longlong(hp[2]), (uint64_t)__double_as_longlong(hp[3]));
  }
  if (m == 0) {
    store16(hdr, (uint64_t)(round + 1), (uint64_t)(replaced_total + __popcll(loser_mask)));
    store16(hdr + 2, 0ull, 0ull);
  }
}

// 7: the copy. A source is a winner and a destination a loser, and with 2 q <= R no member is
// both (sacenv_selection.h, rule 3): the slabs this launch reads are not written by it and the
// slabs it writes are not read, so the order of its workgroups cannot show.
__global__ __launch_bounds__(kCopyThreads) void k_select_copy(const char* __restrict__ state,
                                                              float4* __restrict__ weights, const int64_t vecs) {
  const int m = blockIdx.y;
  const int32_t s =
      (reinterpret_cast<const SacenvSelectMember*>(state + SACENV_SELECT_HEADER_BYTES) + m)->source_now;
  if (s < 0 || s >= (int)gridDim.y || s == m) return;   // (a state of garbage moves nothing out of bounds)
  slab_copy<kCopyThreads>(weights + (int64_t)s * vecs, weights + (int64_t)m * vecs, vecs);
}

// the empty state: lane m writes member m's record, lane 0 the header too
__global__ __launch_bounds__(kWave) void k_select_init(char* __restrict__ state, const int32_t members,
                                                       const Initial init) {
  const int m = threadIdx.x;
  if (m == 0) {
    store16(state, 0ull, 0ull);
    store16(state + 16, 0ull, 0ull);
  }
  if (m >= members) return;
  char* out = reinterpret_cast<char*>(select_member(state, m));
  store16(out, 0ull, 0ull);
  store16(out + 16, pack32(-1, -1), pack32(-1, 0));
  store16(out + 32, (uint64_t)__double_as_longlong(init.hp[m][0]), (uint64_t)__double_as_longlong(init.hp[m][1]));
  store16(out + 48, (uint64_t)__double_as_longlong(init.hp[m][2]), (uint64_t)__double_as_longlong(init.hp[m][3]));
}

int check_select(const SacenvSelect* s) {
  if (s == nullptr) return SACENV_E_NULL;
  if (s->members < 2 || s->members > kMaxP || s->quantile < 1 || 2 * (int64_t)s->quantile > s->members ||
      s->lookback < 1 || s->lookback > SACENV_BOARD_MAX_LOOKBACK || s->min_episodes < 1 || s->member_floats < 1 ||
      s->member_floats % 4 != 0)
    return SACENV_E_SIZE;
  for (int i = 0; i < 2; ++i)
    if (!isfinite(s->factor[i]) || !(s->factor[i] > 0.0)) return SACENV_E_RANGE;
  for (int k = 0; k < 4; ++k)
    if (!isfinite(s->lo[k]) || !isfinite(s->hi[k]) || s->lo[k] > s->hi[k]) return SACENV_E_RANGE;
  return SACENV_OK;
}

}  // namespace

extern "C" {

int sacenv_select_bytes(const SacenvSelect* s, int64_t* bytes) {
  const int rc = check_select(s);
  if (rc) return rc;
  if (bytes == nullptr) return SACENV_E_NULL;
  *bytes = SACENV_SELECT_HEADER_BYTES + (int64_t)SACENV_SELECT_MEMBER_BYTES * s->members;
  return SACENV_OK;
}

int sacenv_select_init(const SacenvSelect* s, const SacenvSacMember* hp0, void* state, void* stream) {
  const int rc = check_select(s);
  if (rc) return rc;
  if (hp0 == nullptr || state == nullptr) return SACENV_E_NULL;
  if ((uintptr_t)state % 16 != 0) return SACENV_E_RANGE;
  Initial init = {};
  for (int m = 0; m < s->members; ++m) {
    const double v[4] = {hp0[m].lr_actor, hp0[m].lr_critic, hp0[m].gamma, hp0[m].tau};
    for (int k = 0; k < 4; ++k) {
      if (!isfinite(v[k])) return SACENV_E_RANGE;
      init.hp[m][k] = v[k];
    }
  }
  hipLaunchKernelGGL(k_select_init, dim3(1), dim3(kWave), 0, (hipStream_t)stream, static_cast<char*>(state),
                     s->members, init);
  return status();
}

int sacenv_select_step(const SacenvSelect* s, const void* board, void* state, float* weights, void* stream) {
  const int rc = check_select(s);
  if (rc) return rc;
  if (board == nullptr || state == nullptr || weights == nullptr) return SACENV_E_NULL;
  if ((uintptr_t)board % 16 != 0 || (uintptr_t)state % 16 != 0 || (uintptr_t)weights % 16 != 0) return SACENV_E_RANGE;
  Decide a;
  a.board = static_cast<const char*>(board);
  a.state = static_cast<char*>(state);
  a.min_episodes = s->min_episodes;
  a.seed = s->seed;
  for (int i = 0; i < 2; ++i) a.factor[i] = s->factor[i];
  for (int k = 0; k < 4; ++k) {
    a.lo[k] = s->lo[k];
    a.hi[k] = s->hi[k];
  }
  a.members = s->members;
  a.quantile = s->quantile;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_select_decide, dim3(1), dim3(kWave), 0, st, a);
  const int64_t vecs = s->member_floats / 4;
  const int64_t chunks = slab_chunks(vecs, kCopyThreads, kCopyChunks);
  hipLaunchKernelGGL(k_select_copy, dim3((uint32_t)chunks, (uint32_t)s->members), dim3(kCopyThreads), 0, st,
                     static_cast<const char*>(state), reinterpret_cast<float4*>(weights), vecs);
  return status();
}

}  // extern "C"
