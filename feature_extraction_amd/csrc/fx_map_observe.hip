// fx_map_observe.hip — the inlier rows of localised scans folded into the landmarks they were matched to (include/fx.h
// fx_map_observe): the re-estimation fx_map_localize leaves to its caller.
//
// The (row, landmark) table is given, so no grid is built.  Every decision is an integer or a minimum over a total order: a row's
// verdict, 32-bit integer atomics (counts and cursors: sums, which commute), an exclusive prefix (fx_device.h's wg_scan2 /
// wg_scan2_blocks), a rank among distinct rows.  The scatter's order is arbitrary and never shows: k_obs_rank puts every list in
// ascending row before anything is added.  Every fp64 sum is an ordered chain on one lane (the build's -ffp-contract=off): the same
// bytes from run to run and with any number of contexts in flight.  The gate reads the records as they are when the call starts:
// the only launch that writes them, k_obs_fold, runs behind every reader, and a lane of it touches its own landmark only.
//
// Launches, in stream order (FXO_WG = 256 rows, landmarks or list entries a workgroup; N = the header's n_landmarks):
//   (a memset: the lists' counts, the cursors and the state words to 0)
//   k_obs_classify  a thread a row r < q_max_rows: the row's scan, whether the scan is used, the proposal, its target through the
//                   alias table (fx_scan_query.h: scan_of_row, scan_used, named_landmark), stale or not, the world point
//                   (world_point) and the gate.  Writes tgt[r], d2[r], observed_id_of_row[r] = -1; counts the row in its
//                   landmark's list
//   k_obs_count     a thread a landmark: the list lengths' exclusive prefix within the block, the block's total; gained[i] = 0
//   k_obs_top       one workgroup: the exclusive prefix of the blocks' totals, the entries of all lists, the used scans
//   k_obs_scatter   a thread a row with a target: its (row, scan, d2 bits) entry to the next free slot of its landmark's list
//   k_obs_rank      a thread an entry: its rank among its list's rows (they are distinct), the entry to that place of `sorted`
//   k_obs_fold      a thread an entry, the one at the head of a list works: the list in ascending row, which is ascending scan; of
//                   a scan's entries the lowest (d2 bits, row) is kept and added to the sums, one chain; the record from the sums
//   k_obs_finish    one lane: the result and the header's n_obs
// A dry run (FX_OBS_DRY_RUN) runs all of it and skips the stores into the map.  No LDS beyond the scan's [2][4] words.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_scan_query.h"
#include "fx_launch.h"
#include "../../include/fx.h"

#define FXO_WG 256
#define FXO_NWAVE (FXO_WG / 64)

static_assert(sizeof(fx_localization) == 112 && sizeof(fx_map_observe_options) == 16 && sizeof(fx_map_observe_result) == 32 &&
                  sizeof(fx_map_landmark) == 48 && sizeof(fx_map_header) == 88,
              "include/fx.h");

namespace {
// landmarks that take part
__device__ __forceinline__ uint32_t obs_landmarks(const FxMapObserveArgs &A) {
  return min(reinterpret_cast<const fx_map_header *>(A.header)->n_landmarks, A.cap);
}
// the first slot of landmark g's list (after k_obs_top)
__device__ __forceinline__ uint32_t list_start(const FxMapObserveArgs &A, uint32_t g) { return A.bsum[g / FXO_WG] + A.local[g]; }
// an entry's d2 bits
__device__ __forceinline__ unsigned long long entry_d2(uint4 e) { return ((unsigned long long)e.w << 32) | e.z; }
}  // namespace

extern "C" __global__ __launch_bounds__(FXO_WG) void k_obs_classify(FxMapObserveArgs A) {
  const uint32_t r = blockIdx.x * FXO_WG + threadIdx.x;
  const KpView V = query_view(A.K);
  const uint32_t N = obs_landmarks(A);
  int32_t g = -1;
  unsigned long long d2 = 0ull;
  bool proposed = false, stale = false, gated = false;
  uint32_t b;
  if (r < V.rows && V.S && scan_of_row(V.off, V.S, r, b) && scan_used(A.loc, b, A.require_flags)) {
    const float4 k = V.kp[r];
    const int32_t id = A.map_id_of_row[r];
    if (finite3(k) && id >= 0 && (uint32_t)id < N) {
      proposed = true;
      uint32_t t;
      bool live = named_landmark(A.alias, N, (uint32_t)id, t);
      fx_map_landmark R;
      if (live) {
        R = reinterpret_cast<const fx_map_landmark *>(A.records)[t];
        live = record_eligible(R, 1u);
      }
      if (!live) {
        stale = true;
      } else {
        double wx, wy, wz;
        world_point(loc_of(A.loc, b)->pose, k, wx, wy, wz);
        const double dx = R.x - wx, dy = R.y - wy;
        const double dd = dx * dx + dy * dy;
        if (dd <= A.gd2) g = (int32_t)t, d2 = (unsigned long long)__double_as_longlong(dd);
        else gated = true;
      }
    }
  }
  if (r < A.K.q_max_rows) {
    A.tgt[r] = g;
    A.d2[r] = d2;
    if (A.observed) A.observed[r] = -1;
    if (g >= 0) atomicAdd(&A.cnt[g], 1u);
  }
  count_wave(proposed, &A.st[1]);
  count_wave(gated, &A.st[4]);
  count_wave(stale, &A.st[5]);
}

extern "C" __global__ __launch_bounds__(FXO_WG) void k_obs_count(FxMapObserveArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXO_NWAVE];
  const uint32_t i = blockIdx.x * FXO_WG + threadIdx.x;
  const uint32_t n = i < A.cap ? A.cnt[i] : 0u;
  uint32_t ea, eb, ta, tb;
  wg_scan2<FXO_NWAVE>(n, 0u, s_w, ea, eb, ta, tb);
  if (i < A.cap) {
    A.local[i] = ea;
    if (A.gained) A.gained[i] = 0u;
  }
  if (threadIdx.x == 0u) A.bsum[blockIdx.x] = ta, A.bsum[n_blocks + blockIdx.x] = 0u;
}

extern "C" __global__ __launch_bounds__(FXO_WG) void k_obs_top(FxMapObserveArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXO_NWAVE];
  uint32_t entries, unused;
  wg_scan2_blocks<FXO_NWAVE>(A.bsum, n_blocks, s_w, entries, unused);
  const uint32_t S = query_scans(A.K);
  uint32_t used = 0u;
  for (uint32_t b = threadIdx.x; b < S; b += FXO_WG) used += scan_used(A.loc, b, A.require_flags) ? 1u : 0u;
  uint32_t ea, eb, ta, tb;
  wg_scan2<FXO_NWAVE>(used, 0u, s_w, ea, eb, ta, tb);
  if (threadIdx.x == 0u) A.st[0] = ta, A.st[7] = entries;
}

extern "C" __global__ __launch_bounds__(FXO_WG) void k_obs_scatter(FxMapObserveArgs A) {
  const uint32_t r = blockIdx.x * FXO_WG + threadIdx.x;
  if (r >= A.K.q_max_rows) return;
  const int32_t g = A.tgt[r];
  if (g < 0) return;
  uint32_t b = 0u;
  (void)scan_of_row(kp_block_offsets(A.K.kp), query_scans(A.K), r, b);  // (a row with a target has a scan)
  const uint32_t slot = list_start(A, (uint32_t)g) + atomicAdd(&A.cur[g], 1u);
  if (slot >= A.K.q_max_rows) return;  // (never: the lists hold as many entries as rows have a target)
  const unsigned long long d2 = A.d2[r];
  A.ent[slot] = make_uint4(r, b, (uint32_t)d2, (uint32_t)(d2 >> 32));
}

extern "C" __global__ __launch_bounds__(FXO_WG) void k_obs_rank(FxMapObserveArgs A) {
  const uint32_t s = blockIdx.x * FXO_WG + threadIdx.x;
  if (s >= min(A.st[7], A.K.q_max_rows)) return;
  const uint32_t row = A.ent[s].x;
  const uint32_t g = (uint32_t)A.tgt[row];
  const uint32_t base = list_start(A, g), n = A.cnt[g];
  uint32_t rank = 0u;
  for (uint32_t j = 0u; j < n; ++j) rank += A.ent[base + j].x < row ? 1u : 0u;
  A.sorted[base + rank] = A.ent[s];  // (read again: an entry held across the loop is spilled to LDS)
}

extern "C" __global__ __launch_bounds__(FXO_WG) void k_obs_fold(FxMapObserveArgs A) {
  const uint32_t s = blockIdx.x * FXO_WG + threadIdx.x;
  if (s >= min(A.st[7], A.K.q_max_rows)) return;
  const uint32_t g = (uint32_t)A.tgt[A.sorted[s].x];
  if (list_start(A, g) != s) return;  // (the list's head works)
  const uint32_t n = A.cnt[g];
  const float4 *kp = kp_block_rows<float4>(A.K.kp, A.K.max_scans);
  fx_map_landmark *rec = reinterpret_cast<fx_map_landmark *>(A.records) + g;
  double *acc = A.acc + (size_t)g * FX_MAP_ACC;
  fx_map_landmark R;  // (only what changes: first_scan, last_scan and segment are neither read nor written)
  R.n_obs = rec->n_obs, R.flags = rec->flags;
  double sx = acc[0], sy = acc[1], sz = acc[2], dsx = acc[5], dsy = acc[6], q = acc[7];
  const double ax = acc[3], ay = acc[4];
  uint32_t k = 0u;
  for (uint32_t i = 0u; i < n;) {
    const uint4 first = A.sorted[s + i];
    const uint32_t scan = first.y;
    uint32_t best_row = first.x, j = i + 1u;
    unsigned long long best_d2 = entry_d2(first);
    for (; j < n; ++j) {  // the scan's other entries: rows ascend, so a tie in d2 keeps the lower row
      const uint4 f = A.sorted[s + j];
      if (f.y != scan) break;
      if (entry_d2(f) < best_d2) best_d2 = entry_d2(f), best_row = f.x;
    }
    double wx, wy, wz;
    world_point(loc_of(A.loc, scan)->pose, kp[best_row], wx, wy, wz);
    const double dx = wx - ax, dy = wy - ay;
    sx += wx, sy += wy, sz += wz;
    dsx += dx, dsy += dy;
    q += (dx * dx + dy * dy);
    if (A.observed) A.observed[best_row] = (int32_t)g;
    ++k;
    i = j;
  }
  if (A.mode == FX_OBS_APPLY) {
    R.n_obs += k;
    map_record_from_sums(R, sx, sy, sz, dsx, dsy, q);
    R.flags |= FX_MAP_LM_OBSERVED;
    acc[0] = sx, acc[1] = sy, acc[2] = sz, acc[5] = dsx, acc[6] = dsy, acc[7] = q;
    rec->x = R.x, rec->y = R.y, rec->z = R.z, rec->rms_xy = R.rms_xy, rec->n_obs = R.n_obs, rec->flags = R.flags;
  }
  if (A.gained) A.gained[g] = k;
  atomicAdd(&A.st[2], k);
  if (n > k) atomicAdd(&A.st[3], n - k);
  atomicAdd(&A.st[6], 1u);
}

extern "C" __global__ __launch_bounds__(64) void k_obs_finish(FxMapObserveArgs A) {
  if (threadIdx.x || blockIdx.x) return;
  if (A.result) {
    for (uint32_t i = 0; i < 7u; ++i) A.result[i] = A.st[i];
    A.result[7] = 0u;
  }
  if (A.mode == FX_OBS_APPLY) reinterpret_cast<fx_map_header *>(A.header)->n_obs += A.st[2];
}

extern "C" hipError_t fxk_map_observe(hipStream_t s, const FxMapObserveArgs &A) {
  const dim3 wg(FXO_WG);
  const uint32_t nl = (A.cap + FXO_WG - 1u) / FXO_WG, nr = (A.K.q_max_rows + FXO_WG - 1u) / FXO_WG;
  // the counts, the cursors and the state words behind them are one region of the scratch (fxk_map_observe_scratch)
  const hipError_t e = hipMemsetAsync(A.cnt, 0, (2u * (size_t)A.cap + FX_MAP_OBSERVE_ST_WORDS) * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  if (nr) hipLaunchKernelGGL(k_obs_classify, dim3(nr), wg, 0, s, A);
  hipLaunchKernelGGL(k_obs_count, dim3(nl), wg, 0, s, A, nl);
  hipLaunchKernelGGL(k_obs_top, dim3(1), wg, 0, s, A, nl);
  if (nr) {
    hipLaunchKernelGGL(k_obs_scatter, dim3(nr), wg, 0, s, A);
    hipLaunchKernelGGL(k_obs_rank, dim3(nr), wg, 0, s, A);
    hipLaunchKernelGGL(k_obs_fold, dim3(nr), wg, 0, s, A);
  }
  hipLaunchKernelGGL(k_obs_finish, dim3(1), dim3(64), 0, s, A);
  return hipGetLastError();
}

// bytes of the context's scratch for a map of `cap` landmarks and q_max_rows rows, and the pointers carved out of it
extern "C" size_t fxk_map_observe_scratch(FxMapObserveArgs *A, uint8_t *base) {
  const size_t cap = A->cap, nb = (cap + FXO_WG - 1u) / FXO_WG, rows = A->K.q_max_rows;
  FxCarve C{base, 0};
  A->cnt = C.take<uint32_t>(2u * cap + FX_MAP_OBSERVE_ST_WORDS);
  A->cur = base ? A->cnt + cap : (uint32_t *)nullptr;
  A->st = base ? A->cur + cap : (uint32_t *)nullptr;
  A->local = C.take<uint32_t>(cap);
  A->bsum = C.take<uint32_t>(2u * nb);
  A->d2 = C.take<unsigned long long>(rows);
  A->tgt = C.take<int32_t>(rows);
  A->ent = C.take<uint4>(rows);
  A->sorted = C.take<uint4>(rows);
  return C.o;
}
