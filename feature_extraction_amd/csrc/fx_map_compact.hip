// fx_map_compact.hip — the persistent map's landmarks renumbered without the dead ones: the fragments fx_map_merge absorbed, and
// the short old landmarks the caller's options let go (include/fx.h fx_map_compact).
//
// Every decision is an integer: a flag a landmark, its exclusive prefix (fx_device.h's wg_scan2 / wg_scan2_blocks) and 32-bit sums,
// which commute.  No floating-point operation occurs: records and sums move as 16-byte vectors, 3 + 4 a landmark.  The same bytes
// from run to run and with any number of contexts in flight.  Counts come from the map's header on the device; the grids are sized
// by the map's max_landmarks and exit early.
//
// The move.  new id <= old id, and the two may lie in different workgroups: landmark 300 may go to slot 40 while landmark 40, of
// another workgroup that has not run yet, still has to be read.  A move in place races, and there is no second set of map buffers to
// swap in, because fx_map_get's and fx_map_get_alias's addresses are promised stable.  So the kept landmarks are gathered into the
// context's scratch (k_mc_stage reads the map, writes the scratch) and copied back by the launch after the next (k_mc_finish reads the
// scratch, writes the map): within one launch nothing is both read and written, and stream order separates the launches.  The
// alias table is read until k_mc_remap (a root's new id is looked up through it) and filled with -1 only by k_mc_finish.
//
// Launches, in stream order (FXMC_WG = 256 landmarks, carry rows or 16-byte vectors a workgroup; N = the header's n_landmarks):
//   (a memset: the marks and the state words to 0)
//   k_mc_mark    a thread a carry row: mark[the resolved root of carry[j]] = 1 (the next update continues it)
//   k_mc_flag    a thread a landmark: kept or not, the workgroup's exclusive prefix of (kept, n_obs of a dropped live one), the
//                block's totals; the absorbed ones are counted
//   k_mc_top     one workgroup: the exclusive prefix of the blocks' totals; st[0] = K, st[1] = the dropped live landmarks' n_obs
//   k_mc_stage   a thread a 16-byte vector of a landmark: a kept one's vector to its new id's place in the scratch
//   k_mc_remap   a thread a landmark / carry row: remap[], and every carry word >= 0 to its root's new id
//   k_mc_finish  a thread a vector: the scratch back into the map; alias[i] = -1; one lane: the header and the result
//
// fx_map_retire (include/fx.h) is this compaction with a rule: A.expected / A.seen given, k_mc_flag also drops the live landmarks the
// counters condemn (unless a carry row holds them) and writes the byte mask; two more launches move the counters with the landmarks,
// staged like the records (k_mc_stage_counters behind k_mc_top, k_mc_finish_counters last).  A dry run launches the mark, the flags,
// the prefix, the remap without its carry half and one lane of the finish.  Without a rule (fx_map_compact) every branch on it is a
// uniform scalar test and nothing else runs.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_scan_query.h"
#include "fx_launch.h"
#include "../../include/fx.h"

#define FXMC_WG 256
#define FXMC_NWAVE (FXMC_WG / 64)
#define FXMC_REC_V 3u  // 16-byte vectors of an fx_map_landmark
#define FXMC_ACC_V 4u  // ... of a landmark's FX_MAP_ACC doubles
#define FXMC_V (FXMC_REC_V + FXMC_ACC_V)

static_assert(sizeof(fx_map_landmark) == FXMC_REC_V * 16 && FX_MAP_ACC * sizeof(double) == FXMC_ACC_V * 16 && sizeof(fx_map_header) == 88 &&
                  sizeof(fx_map_compact_result) == 16 && sizeof(fx_map_retire_result) == 32 && sizeof(fx_map_retire_options) == 24,
              "include/fx.h");

namespace {
__device__ __forceinline__ const fx_map_header *header(const FxMapCompactArgs &A) { return reinterpret_cast<const fx_map_header *>(A.header); }
__device__ __forceinline__ uint32_t n_landmarks(const FxMapCompactArgs &A) { return min(header(A)->n_landmarks, A.cap); }
__device__ __forceinline__ uint32_t n_carry(const FxMapCompactArgs &A) { return min(header(A)->carry_rows, A.max_carry); }
// the landmark that holds id's observations: its root when it was absorbed (alias entries are fully resolved); id < N
__device__ __forceinline__ uint32_t root_of(const FxMapCompactArgs &A, uint32_t id, uint32_t N) {
  const int32_t a = A.alias[id];
  return a >= 0 && (uint32_t)a < N ? (uint32_t)a : id;
}
// the new id of landmark i < N after k_mc_top, -1: dropped
__device__ __forceinline__ int32_t new_id(const FxMapCompactArgs &A, uint32_t i) {
  const int32_t local = A.local[i];
  return local >= 0 ? (int32_t)(A.bsum[i / FXMC_WG] + (uint32_t)local) : -1;
}
// fx_map_retire's result (one lane, behind k_mc_top)
__device__ __forceinline__ void write_retire_result(const FxMapCompactArgs &A, uint32_t N, uint32_t K) {
  A.result[0] = N, A.result[1] = K, A.result[2] = A.st[2], A.result[3] = A.st[3], A.result[4] = A.st[4], A.result[5] = A.st[5];
  A.result[6] = A.result[7] = 0u;
}
}  // namespace

extern "C" __global__ __launch_bounds__(FXMC_WG) void k_mc_mark(FxMapCompactArgs A) {
  const uint32_t j = blockIdx.x * FXMC_WG + threadIdx.x;
  const uint32_t N = n_landmarks(A);
  if (j >= n_carry(A)) return;
  const int32_t c = A.carry[j];
  if (c >= 0 && (uint32_t)c < N) A.mark[root_of(A, (uint32_t)c, N)] = 1u;  // (every writer writes 1)
}

extern "C" __global__ __launch_bounds__(FXMC_WG) void k_mc_flag(FxMapCompactArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXMC_NWAVE];
  const uint32_t i = blockIdx.x * FXMC_WG + threadIdx.x;
  const uint32_t N = n_landmarks(A);
  uint32_t kept = 0u, lost_obs = 0u;
  bool absorbed = false, retired = false, held = false;
  if (i < N) {
    const fx_map_landmark *R = reinterpret_cast<const fx_map_landmark *>(A.records) + i;
    absorbed = A.alias[i] != -1;
    const uint32_t n_obs = R->n_obs, age = (header(A)->scans - 1u) - R->last_scan;
    kept = !absorbed && (n_obs >= A.min_obs || age < A.min_age || A.mark[i] != 0u) ? 1u : 0u;
    if (A.expected && !absorbed) {  // fx_map_retire's rule: expected often enough, seen too rarely, and no carry row holds it
      const uint32_t e = A.expected[i], sn = A.seen[i];
      const bool condemned = e >= A.min_expected && (unsigned long long)sn * A.seen_den < (unsigned long long)e * A.seen_num;
      retired = condemned && A.mark[i] == 0u, held = condemned && A.mark[i] != 0u;
      if (retired) kept = 0u, atomicAdd(&A.st[4], n_obs);
    }
    lost_obs = !absorbed && !kept ? n_obs : 0u;
  }
  if (A.expected) {
    if (A.retired && i < A.cap) A.retired[i] = retired ? 1u : 0u;
    count_wave(retired, &A.st[3]);
    count_wave(held, &A.st[5]);
  }
  uint32_t ea, eb, ta, tb;
  wg_scan2<FXMC_NWAVE>(kept, lost_obs, s_w, ea, eb, ta, tb);
  if (i < A.cap) A.local[i] = kept ? (int32_t)ea : -1;
  if (threadIdx.x == 0u) A.bsum[blockIdx.x] = ta, A.bsum[n_blocks + blockIdx.x] = tb;
  count_wave(absorbed, &A.st[2]);
}

extern "C" __global__ __launch_bounds__(FXMC_WG) void k_mc_top(FxMapCompactArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXMC_NWAVE];
  uint32_t tot_a, tot_b;
  wg_scan2_blocks<FXMC_NWAVE>(A.bsum, n_blocks, s_w, tot_a, tot_b);
  if (threadIdx.x == 0u) A.st[0] = tot_a, A.st[1] = tot_b;
}

extern "C" __global__ __launch_bounds__(FXMC_WG) void k_mc_stage(FxMapCompactArgs A) {
  const size_t t = (size_t)blockIdx.x * FXMC_WG + threadIdx.x;
  const size_t i = t / FXMC_V;
  const uint32_t v = (uint32_t)(t - i * FXMC_V);
  if (i >= n_landmarks(A)) return;
  const int32_t id = new_id(A, (uint32_t)i);
  if (id < 0) return;  // (id <= i < cap: inside the scratch)
  if (v < FXMC_REC_V)
    A.stage_rec[(size_t)id * FXMC_REC_V + v] = reinterpret_cast<const uint4 *>(A.records)[i * FXMC_REC_V + v];
  else
    A.stage_acc[(size_t)id * FXMC_ACC_V + (v - FXMC_REC_V)] = reinterpret_cast<const uint4 *>(A.acc)[i * FXMC_ACC_V + (v - FXMC_REC_V)];
}

extern "C" __global__ __launch_bounds__(FXMC_WG) void k_mc_remap(FxMapCompactArgs A) {
  const uint32_t i = blockIdx.x * FXMC_WG + threadIdx.x;
  const uint32_t N = n_landmarks(A);
  if (A.remap && i < A.cap) A.remap[i] = i < N ? new_id(A, root_of(A, i, N)) : -1;  // (a dropped live one is its own root: -1)
  if (i < n_carry(A) && !A.dry_run) {
    const int32_t c = A.carry[i];
    if (c >= 0) A.carry[i] = (uint32_t)c < N ? new_id(A, root_of(A, (uint32_t)c, N)) : -1;
  }
}

extern "C" __global__ __launch_bounds__(FXMC_WG) void k_mc_finish(FxMapCompactArgs A) {
  const size_t t = (size_t)blockIdx.x * FXMC_WG + threadIdx.x;
  const uint32_t K = min(A.st[0], A.cap);
  if (A.dry_run) {  // (fx_map_retire alone: one workgroup, and only the result is written)
    if (!t && A.result) write_retire_result(A, n_landmarks(A), K);
    return;
  }
  if (t < (size_t)K * FXMC_REC_V) reinterpret_cast<uint4 *>(A.records)[t] = A.stage_rec[t];
  if (t < (size_t)K * FXMC_ACC_V) reinterpret_cast<uint4 *>(A.acc)[t] = A.stage_acc[t];
  if (t < A.cap) A.alias[t] = -1;
  if (t) return;
  // (no other thread of this launch reads the header)
  fx_map_header *H = reinterpret_cast<fx_map_header *>(A.header);
  const uint32_t N = min(H->n_landmarks, A.cap);
  H->n_landmarks = H->n_needed = K;
  H->n_obs -= A.st[1];
  if (A.result && !A.expected) A.result[0] = N, A.result[1] = K, A.result[2] = A.st[2], A.result[3] = N - K - A.st[2];
  if (A.result && A.expected) write_retire_result(A, N, K);
}

// fx_map_retire: a thread a landmark, a kept one's two counters to its new id's place in the scratch
extern "C" __global__ __launch_bounds__(FXMC_WG) void k_mc_stage_counters(FxMapCompactArgs A) {
  const uint32_t i = blockIdx.x * FXMC_WG + threadIdx.x;
  if (i >= n_landmarks(A)) return;
  const int32_t id = new_id(A, i);
  if (id < 0) return;  // (id <= i < cap: inside the scratch)
  A.stage_cnt[id] = A.expected[i], A.stage_cnt[(size_t)A.cap + (uint32_t)id] = A.seen[i];
}

// fx_map_retire: a thread a word of each counter array: the staged counters back, 0 from K on
extern "C" __global__ __launch_bounds__(FXMC_WG) void k_mc_finish_counters(FxMapCompactArgs A) {
  const uint32_t t = blockIdx.x * FXMC_WG + threadIdx.x;
  const uint32_t K = min(A.st[0], A.cap);
  if (t >= A.cap) return;
  A.expected[t] = t < K ? A.stage_cnt[t] : 0u;
  A.seen[t] = t < K ? A.stage_cnt[(size_t)A.cap + t] : 0u;
}

extern "C" hipError_t fxk_map_compact(hipStream_t s, const FxMapCompactArgs &A) {
  const dim3 wg(FXMC_WG);
  const uint32_t nl = (A.cap + FXMC_WG - 1u) / FXMC_WG;
  const uint32_t nc = (A.max_carry + FXMC_WG - 1u) / FXMC_WG;
  const uint32_t nr = ((A.cap > A.max_carry ? A.cap : A.max_carry) + FXMC_WG - 1u) / FXMC_WG;
  const uint32_t nv = (uint32_t)(((size_t)A.cap * FXMC_V + FXMC_WG - 1u) / FXMC_WG);
  const uint32_t nf = (uint32_t)(((size_t)A.cap * FXMC_ACC_V + FXMC_WG - 1u) / FXMC_WG);
  // the marks and the state words behind them are one region of the scratch (fxk_map_compact_scratch)
  const hipError_t e = hipMemsetAsync(A.mark, 0, ((size_t)A.cap + FX_MAP_COMPACT_ST_WORDS) * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  if (nc) hipLaunchKernelGGL(k_mc_mark, dim3(nc), wg, 0, s, A);
  hipLaunchKernelGGL(k_mc_flag, dim3(nl), wg, 0, s, A, nl);
  hipLaunchKernelGGL(k_mc_top, dim3(1), wg, 0, s, A, nl);
  if (A.dry_run) {  // (fx_map_retire alone)
    hipLaunchKernelGGL(k_mc_remap, dim3(nl), wg, 0, s, A);
    hipLaunchKernelGGL(k_mc_finish, dim3(1), wg, 0, s, A);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_mc_stage, dim3(nv), wg, 0, s, A);
  if (A.expected) hipLaunchKernelGGL(k_mc_stage_counters, dim3(nl), wg, 0, s, A);
  hipLaunchKernelGGL(k_mc_remap, dim3(nr), wg, 0, s, A);
  hipLaunchKernelGGL(k_mc_finish, dim3(nf), wg, 0, s, A);
  if (A.expected) hipLaunchKernelGGL(k_mc_finish_counters, dim3(nl), wg, 0, s, A);
  return hipGetLastError();
}

// bytes of the context's scratch for a map of `cap` landmarks, and the pointers carved out of it
extern "C" size_t fxk_map_compact_scratch(FxMapCompactArgs *A, uint8_t *base) {
  const size_t cap = A->cap, nb = (cap + FXMC_WG - 1u) / FXMC_WG;
  FxCarve C{base, 0};
  A->stage_rec = C.take<uint4>(cap * FXMC_REC_V);
  A->stage_acc = C.take<uint4>(cap * FXMC_ACC_V);
  A->mark = C.take<uint32_t>(cap + FX_MAP_COMPACT_ST_WORDS);
  A->st = base ? A->mark + cap : (uint32_t *)nullptr;
  A->local = C.take<int32_t>(cap);
  A->bsum = C.take<uint32_t>(2u * nb);
  A->stage_cnt = A->expected ? C.take<uint32_t>(2u * cap) : (uint32_t *)nullptr;
  return C.o;
}
