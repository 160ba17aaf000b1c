// fx_map.hip — the persistent landmark map: one batch's tracks folded into the run's landmarks (include/fx.h fx_map_update).
//
// A track that begins at local row j of the batch's scan 0 continues the map landmark the carry table holds for row j of the
// scan the batch before ended with, when the caller says the two scans are one and their rows are the same bits.  Every decision
// is an integer (an atomicOr of "a row differs", an atomicAdd of observation counts: both order-free), every fp64 value is an
// ordered chain of correctly rounded operations on one lane (the build's -ffp-contract=off): the same bytes from run to run and
// with any number of contexts in flight.  Every count comes from the track's header on the device; the grids are sized by
// q_max_rows and max_landmarks and exit early.
//
// Launches, in stream order (FXMAP_WG = 256 rows or landmarks a workgroup):
//   k_map_compare     a thread a row of scan 0: its four words against the stored copy of the carry scan's row; any difference
//                     sets st[0] (only with FX_MAP_OVERLAP and equal row counts)
//   k_map_join        a thread a batch landmark: continues carry[first_row - kp_offset[0]], new, or not a landmark; the block's
//                     counts of new and continued ones
//   k_map_top         one workgroup: the exclusive prefix of the blocks' counts, and the update's numbering into st
//   k_map_accumulate  a thread a batch landmark: its id (n_needed + the new ones before it, or the landmark it continues), the
//                     sequential pass over its obs_row segment into the private sums, the public record
//   k_map_rows        a thread a row: map_id_of_row, and for the rows of scan S - 1 the carry table and the carry scan's copy
//   k_map_finish      one lane: the header
// The block's layout, the workgroup scan and the world-frame point of an observation are fx_device.h's (kp_block_*, wg_scan2,
// world_point): the ones fx_track.hip uses, which is what keeps the map equal to one long track.  The record from the sums
// (map_record_from_sums) is shared with fx_map_merge.hip.  The alias table is fx_map_merge's: a reset fills it with -1, the update
// never touches it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_device.h"
#include "fx_launch.h"
#include "../../include/fx.h"

#define FXMAP_WG 256
#define FXMAP_NWAVE (FXMAP_WG / 64)

static_assert(sizeof(fx_map_landmark) == 48 && sizeof(fx_map_header) == 88 && offsetof(fx_map_header, last_pose) == 40, "include/fx.h");

namespace {
// what the update reads of the batch: kp_offset, the rows as words, and the sizes of include/fx.h's "Sizes" clause
struct View {
  const uint32_t *off;
  const uint4 *kp;
  uint32_t S, rows, L;
};
__device__ __forceinline__ View view(const FxMapArgs &A) {
  const fx_track_header *h = reinterpret_cast<const fx_track_header *>(A.track_header);
  View v;
  v.off = kp_block_offsets(A.kp);
  v.kp = kp_block_rows<uint4>(A.kp, A.max_scans);
  v.S = min(h->scans, A.max_scans);
  v.rows = min(min(h->rows, A.max_total), A.q_max_rows);
  v.L = v.S ? min(h->n_landmarks, A.max_landmarks) : 0u;
  return v;
}
__device__ __forceinline__ uint32_t scan_lo(const View &v, uint32_t b) { return min(v.off[b], v.rows); }
__device__ __forceinline__ uint32_t scan_hi(const View &v, uint32_t b) { return max(min(v.off[b + 1u], v.rows), scan_lo(v, b)); }
// may the overlap be accepted, as far as the counts go (the rows are k_map_compare's)
__device__ __forceinline__ bool overlap_counts(const FxMapArgs &A, const View &v) {
  const fx_map_header *H = reinterpret_cast<const fx_map_header *>(A.header);
  return (A.flags & FX_MAP_OVERLAP) && v.S && H->scans && H->carry_rows == scan_hi(v, 0u) - scan_lo(v, 0u);
}
}  // namespace

extern "C" __global__ __launch_bounds__(64) void k_map_reset(FxMapArgs A) {
  if (threadIdx.x || blockIdx.x) return;
  fx_map_header h = {};
  h.last_pose.c = 1.0;
  *reinterpret_cast<fx_map_header *>(A.header) = h;
  for (uint32_t i = 0; i < FX_MAP_ST_WORDS; ++i) A.st[i] = 0u;
}

extern "C" __global__ __launch_bounds__(FXMAP_WG) void k_map_compare(FxMapArgs A) {
  const uint32_t j = blockIdx.x * FXMAP_WG + threadIdx.x;
  const View V = view(A);
  if (!overlap_counts(A, V)) return;
  const uint32_t lo = scan_lo(V, 0u), n0 = scan_hi(V, 0u) - lo;
  bool differs = false;
  if (j < n0 && j < A.max_carry) {  // (n0 == carry_rows <= max_carry)
    const uint4 a = V.kp[lo + j], b = A.carry_kp[j];
    differs = a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w;
  }
  if (__ballot(differs) && (threadIdx.x & 63u) == 0u) atomicOr(&A.st[0], 1u);
}

extern "C" __global__ __launch_bounds__(FXMAP_WG) void k_map_join(FxMapArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXMAP_NWAVE];
  const uint32_t i = blockIdx.x * FXMAP_WG + threadIdx.x;
  const View V = view(A);
  const fx_map_header *H = reinterpret_cast<const fx_map_header *>(A.header);
  uint32_t is_new = 0u, is_joined = 0u;
  if (i < V.L) {
    const fx_landmark lm = reinterpret_cast<const fx_landmark *>(A.landmarks)[i];
    // a record the track wrote passes; these bounds keep every later read inside the buffers whatever the record holds
    const bool ok = lm.n_obs >= 1u && lm.first_scan < V.S && lm.n_obs <= V.S - lm.first_scan && lm.obs0 <= A.q_max_rows &&
                    lm.n_obs <= A.q_max_rows - lm.obs0 && lm.first_row < V.rows;
    int32_t g = -1;
    if (ok && lm.first_scan == 0u && overlap_counts(A, V) && A.st[0] == 0u) {
      const uint32_t lo = scan_lo(V, 0u);
      if (lm.first_row >= lo && lm.first_row - lo < H->carry_rows) {
        g = A.carry[lm.first_row - lo];
        if (g < 0 || (uint32_t)g >= H->n_landmarks) g = -1;
      }
    }
    is_joined = ok && g >= 0, is_new = ok && g < 0;
    A.id_of_lm[i] = ok ? g : -2;
  }
  uint32_t ea, eb, ta, tb;
  wg_scan2<FXMAP_NWAVE>(is_new, is_joined, s_w, ea, eb, ta, tb);
  if (threadIdx.x == 0u) A.bsum[blockIdx.x] = ta, A.bsum[n_blocks + blockIdx.x] = tb;
}

extern "C" __global__ __launch_bounds__(FXMAP_WG) void k_map_top(FxMapArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXMAP_NWAVE];
  uint32_t base_a, base_b;
  wg_scan2_blocks<FXMAP_NWAVE>(A.bsum, n_blocks, s_w, base_a, base_b);
  if (threadIdx.x == 0u) {
    const View V = view(A);
    const fx_map_header *H = reinterpret_cast<const fx_map_header *>(A.header);
    const bool accepted = overlap_counts(A, V) && A.st[0] == 0u;
    A.st[1] = accepted ? 1u : 0u;
    A.st[2] = accepted ? H->scans - 1u : H->scans;
    A.st[3] = accepted ? H->segments - 1u : H->segments;
    A.st[4] = base_a, A.st[5] = base_b;
  }
}

extern "C" __global__ __launch_bounds__(FXMAP_WG) void k_map_accumulate(FxMapArgs A) {
  __shared__ uint32_t s_w[2 * FXMAP_NWAVE];
  const uint32_t i = blockIdx.x * FXMAP_WG + threadIdx.x;
  const View V = view(A);
  const fx_map_header *H = reinterpret_cast<const fx_map_header *>(A.header);
  const int32_t verdict = i < V.L ? A.id_of_lm[i] : -2;
  uint32_t ea, eb, ta, tb;
  wg_scan2<FXMAP_NWAVE>(verdict == -1 ? 1u : 0u, 0u, s_w, ea, eb, ta, tb);
  const bool joined = verdict >= 0;
  const uint32_t id = joined ? (uint32_t)verdict : H->n_needed + A.bsum[blockIdx.x] + ea;
  const bool stored = verdict >= -1 && id < A.cap;
  uint32_t added = 0u;
  if (stored) {
    const fx_landmark lm = reinterpret_cast<const fx_landmark *>(A.landmarks)[i];
    const fx_pose *poses = reinterpret_cast<const fx_pose *>(A.poses);
    const float4 *kp = reinterpret_cast<const float4 *>(V.kp);
    fx_map_landmark *rec = reinterpret_cast<fx_map_landmark *>(A.records) + id;
    double *acc = A.acc + (size_t)id * FX_MAP_ACC;
    const uint32_t scan_base = A.st[2], seg_base = A.st[3];
    double sx = 0.0, sy = 0.0, sz = 0.0, ax = 0.0, ay = 0.0, dsx = 0.0, dsy = 0.0, q = 0.0;
    fx_map_landmark R;
    if (joined) {
      sx = acc[0], sy = acc[1], sz = acc[2], ax = acc[3], ay = acc[4], dsx = acc[5], dsy = acc[6], q = acc[7];
      R = *rec;
      R.flags |= FX_MAP_LM_CONTINUED;
    } else {
      R.n_obs = 0u, R.first_scan = scan_base + lm.first_scan, R.segment = seg_base + poses[lm.first_scan].segment, R.flags = 0u;
    }
    for (uint32_t k = joined ? 1u : 0u; k < lm.n_obs; ++k) {
      double wx, wy, wz;  // (the track's rows are below `rows`)
      world_point(poses[lm.first_scan + k], kp[min(A.obs_row[lm.obs0 + k], V.rows - 1u)], wx, wy, wz);
      if (!joined && k == 0u) ax = wx, ay = wy;
      const double dx = wx - ax, dy = wy - ay;
      sx += wx, sy += wy, sz += wz;
      dsx += dx, dsy += dy;
      q += (dx * dx + dy * dy);
    }
    added = lm.n_obs - (joined ? 1u : 0u);
    R.n_obs += added;
    map_record_from_sums(R, sx, sy, sz, dsx, dsy, q);
    R.last_scan = scan_base + (lm.first_scan + lm.n_obs - 1u);
    acc[0] = sx, acc[1] = sy, acc[2] = sz, acc[3] = ax, acc[4] = ay, acc[5] = dsx, acc[6] = dsy, acc[7] = q;
    *rec = R;
  }
  if (i < V.L) A.id_of_lm[i] = stored ? (int32_t)id : -1;
  wg_scan2<FXMAP_NWAVE>(added, 0u, s_w, ea, eb, ta, tb);
  if (threadIdx.x == 0u && ta) atomicAdd(&A.st[7], ta);
}

extern "C" __global__ __launch_bounds__(FXMAP_WG) void k_map_rows(FxMapArgs A) {
  const uint32_t r = blockIdx.x * FXMAP_WG + threadIdx.x;
  if (r >= A.q_max_rows) return;
  const View V = view(A);
  int32_t id = -1;
  if (r < V.rows) {
    const int32_t l = A.landmark_of_row[r];
    if (l >= 0 && (uint32_t)l < V.L) id = A.id_of_lm[l];
  }
  if (A.map_id_of_row) A.map_id_of_row[r] = id;
  if (!V.S) return;
  const uint32_t lo = scan_lo(V, V.S - 1u), hi = scan_hi(V, V.S - 1u);
  if (hi - lo > A.max_carry || r < lo || r >= hi) return;
  const uint32_t j = r - lo;
  const bool keep = V.S == 1u && A.st[1] == 1u;  // (then the carry scan is this scan: row j is row j)
  A.carry[j] = id >= 0 ? id : keep ? A.carry[j] : -1;
  A.carry_kp[j] = V.kp[r];
}

extern "C" __global__ __launch_bounds__(64) void k_map_finish(FxMapArgs A) {
  if (threadIdx.x || blockIdx.x) return;
  const View V = view(A);
  const fx_track_header *t = reinterpret_cast<const fx_track_header *>(A.track_header);
  fx_map_header *H = reinterpret_cast<fx_map_header *>(A.header);
  fx_map_header h = *H;
  h.batches += 1u;
  h.last_joined = h.last_new = 0u;
  if (V.S) {
    const fx_pose last = reinterpret_cast<const fx_pose *>(A.poses)[V.S - 1u];
    const uint32_t n_last = scan_hi(V, V.S - 1u) - scan_lo(V, V.S - 1u);
    h.last_new = A.st[4], h.last_joined = A.st[5];
    h.n_needed += A.st[4];
    h.n_landmarks = min(h.n_needed, A.cap);
    h.n_obs += A.st[7];
    h.scans = A.st[2] + V.S;
    h.segments = A.st[3] + last.segment + 1u;
    h.carry_rows = n_last <= A.max_carry ? n_last : 0u;
    h.last_pose = last;
    if (h.n_needed > A.cap) h.flags |= FX_MAP_FULL;
    if ((A.flags & FX_MAP_OVERLAP) && A.st[1] == 0u) h.flags |= FX_MAP_OVERLAP_MISMATCH;
    if (t->n_landmarks > A.max_landmarks) h.flags |= FX_MAP_TRACK_TRUNCATED;
  }
  *H = h;
  A.st[0] = 0u, A.st[7] = 0u;
}

extern "C" hipError_t fxk_map_reset(hipStream_t s, const FxMapArgs &A) {
  const hipError_t e = hipMemsetAsync(A.alias, 0xff, (size_t)A.cap * sizeof(int32_t), s);  // every landmark live: -1
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_map_reset, dim3(1), dim3(64), 0, s, A);
  return hipGetLastError();
}

extern "C" hipError_t fxk_map_update(hipStream_t s, const FxMapArgs &A) {
  const dim3 wg(FXMAP_WG);
  const uint32_t nc = A.q_max_rows < A.max_carry ? A.q_max_rows : A.max_carry;
  const uint32_t nl = (A.max_landmarks + FXMAP_WG - 1u) / FXMAP_WG, nr = (A.q_max_rows + FXMAP_WG - 1u) / FXMAP_WG;
  if ((A.flags & FX_MAP_OVERLAP) && nc) hipLaunchKernelGGL(k_map_compare, dim3((nc + FXMAP_WG - 1u) / FXMAP_WG), wg, 0, s, A);
  if (nl) hipLaunchKernelGGL(k_map_join, dim3(nl), wg, 0, s, A, nl);
  hipLaunchKernelGGL(k_map_top, dim3(1), wg, 0, s, A, nl);
  if (nl) hipLaunchKernelGGL(k_map_accumulate, dim3(nl), wg, 0, s, A);
  if (nr) hipLaunchKernelGGL(k_map_rows, dim3(nr), wg, 0, s, A);
  hipLaunchKernelGGL(k_map_finish, dim3(1), dim3(64), 0, s, A);
  return hipGetLastError();
}

extern "C" uint32_t fxk_map_wg(void) { return FXMAP_WG; }
