// fx_map_localize.hip — scans localised against the persistent map under a prior pose (include/fx.h fx_map_localize): which
// landmark each keypoint row is, and each scan's pose in the map's frame.
//
// The association is defined over ALL (row, landmark) pairs; the grid (fx_map_grid.h: fx_map_merge's, with the search distance
// for its gate) only finds the landmarks that can be in reach.  Every choice is a minimum over a total order or an integer count,
// every fp64 sum an ordered chain on one lane (the build's -ffp-contract=off): the same bytes from run to run and with any number
// of contexts in flight.  The map is only read.
//
// Launches, in stream order, after fxk_map_grid_build's five (the merge's live set: alias -1, n_obs >= 1, finite x and y):
//   k_loc_search     a thread a row r < q_max_rows: the row's scan (fx_scan_query.h scan_of_row), the world
//                    point under the scan's prior (world_point), the walk over its 3 x 3 cells and the far bucket; the walk
//                    applies min_landmark_obs, the finite z and the segment to the candidates in reach and keeps the lowest
//                    (d2 bits, id).  Writes near[r] and d2[r] (scratch), nearest_of_row[r] when given, map_id_of_row[r] = -1
//   k_loc_consensus  one 256-thread workgroup a scan: fx_map_consensus.h's body (rank, hypotheses, refit: shared with
//                    fx_map_join_segments) over this gather:
//     gather      the scan's rows with a landmark into LDS in ascending row (wg_ordered_slot; at most FX_LOC_MAX_CORR)
// LDS of k_loc_consensus: fx_map_consensus.h's 57.9 KB.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_map_consensus.h"
#include "fx_map_grid.h"
#include "fx_scan_query.h"
#include "fx_launch.h"
#include "../../include/fx.h"

using namespace fxc;
using namespace fxg;

#define FXL_WG FXC_MAP_WG
#define FXL_NWAVE FXC_MAP_NWAVE

static_assert(sizeof(fx_localization) == 112 && sizeof(fx_localize_options) == 32 && sizeof(fx_pose) == 48, "include/fx.h");
static_assert(FX_LOC_MAX_CORR == FXC_MAP_MAX_CORR, "fx_map_consensus.h");


namespace {
__device__ __forceinline__ void write_no_fit(fx_localization *out, const fx_pose &prior, uint32_t n_corr, uint32_t flags) {
  fx_localization r;
  r.pose = prior;
  r.dc = 1.0, r.ds = 0.0, r.dtx = 0.0, r.dty = 0.0, r.dtz = 0.0;
  r.rms = INFINITY;
  r.n_corr = n_corr, r.n_inliers = 0u, r.flags = flags;
  r.hyp_a = r.hyp_b = 0xffffffffu;
  *out = r;
}
}  // namespace

extern "C" __global__ __launch_bounds__(FXL_WG) void k_loc_search(FxMapLocalizeArgs A) {
  const uint32_t r = blockIdx.x * FXL_WG + threadIdx.x;
  if (r >= A.K.q_max_rows) return;
  const KpView V = query_view(A.K);
  Near best;
  best.any = false, best.d2 = 0ull, best.id = 0u;
  uint32_t seg, scan;
  bool any_seg;
  if (r < V.rows && V.S && wanted_segment(A.G.header, A.segment, seg, any_seg) && scan_of_row(V.off, V.S, r, scan)) {
    const fx_pose P = reinterpret_cast<const fx_pose *>(A.priors)[scan];
    const float4 k = V.kp[r];
    if (finite_pose(P) && finite3(k)) {
      double wx, wy, wz;
      world_point(P, k, wx, wy, wz);
      const double tx = floor(wx * A.G.inv_edge), ty = floor(wy * A.G.inv_edge);
      const auto wanted = [&](const FxMapMergeCand &c) { return any_seg || c.segment == seg; };
      grid_neighbourhood(A.G, tx, ty, [&](uint32_t b) { walk_nearest(A.G, A.min_landmark_obs, b, wx, wy, wanted, best); });
    }
  }
  const int32_t g = best.any ? (int32_t)best.id : -1;
  A.near[r] = g;
  A.d2[r] = best.d2;
  A.map_id_of_row[r] = -1;
  if (A.nearest_of_row) A.nearest_of_row[r] = g;
}

extern "C" __global__ __launch_bounds__(FXL_WG) void k_loc_consensus(FxMapLocalizeArgs A) {
  __shared__ MapConsensusLds L;

  const uint32_t tid = threadIdx.x, b = blockIdx.x;
  const KpView V = query_view(A.K);
  const fx_pose prior = reinterpret_cast<const fx_pose *>(A.priors)[b];
  fx_localization *out = reinterpret_cast<fx_localization *>(A.out) + b;
  if (b >= V.S || !finite_pose(prior)) {  // (uniform)
    if (tid == 0u) write_no_fit(out, prior, 0u, b >= V.S ? FX_LOC_NO_SCAN : FX_LOC_BAD_PRIOR);
    return;
  }
  const fx_map_landmark *rec = records(A.G);
  uint32_t q_lo, q_hi;
  scan_rows(V, b, q_lo, q_hi);

  // ---- gather: the correspondences in ascending row, the first FX_LOC_MAX_CORR kept
  auto gather = [&](MapConsensusLds &L) {
    uint32_t found = 0u;  // (uniform)
    for (unsigned long long r0 = q_lo; r0 < q_hi && found <= FX_LOC_MAX_CORR; r0 += FXL_WG) {
      const uint32_t i = (uint32_t)min(r0 + tid, (unsigned long long)q_hi);
      int32_t g = -1;
      if (i < q_hi) g = A.near[i];
      const bool ok = g >= 0 && (uint32_t)g < A.G.cap;
      uint32_t slot, all;
      wg_ordered_slot<FXL_NWAVE>(ok, L.wave, found, slot, all);
      if (ok && slot < FX_LOC_MAX_CORR) {
        const fx_map_landmark R = rec[g];
        double wx, wy, wz;
        world_point(prior, V.kp[i], wx, wy, wz);
        L.xy[slot] = make_double4(wx, wy, R.x, R.y);
        L.dz[slot] = R.z - wz;
        L.d2[slot] = A.d2[i];
        L.row[slot] = i;
      }
      found += all;
      __syncthreads();  // (L.wave is written again next round)
    }
    return found;
  };
  MapConsensusOut O;
  const bool fitted = map_consensus(L, gather, A.inlier_dist, A.min_baseline, A.hyp_corr, O);
  const uint32_t flags = O.truncated ? FX_LOC_TRUNCATED : 0u;
  if (!fitted) {  // (uniform) fewer than 2 correspondences, or no sample passed the gates with 2 agreeing
    if (tid == 0u) write_no_fit(out, prior, O.n_corr, flags | FX_LOC_NO_HYPOTHESIS);
    return;
  }
  if (tid == 0u) {
    fx_localization r;
    r.pose = prior;
    r.dc = O.dc, r.ds = O.ds, r.dtx = O.dtx, r.dty = O.dty, r.dtz = O.dtz;
    r.rms = O.rms;
    r.n_corr = O.n_corr, r.n_inliers = O.n_inliers, r.flags = flags | (O.n_inliers >= A.min_inliers ? FX_LOC_VALID : 0u);
    r.hyp_a = O.hyp_a, r.hyp_b = O.hyp_b;
    if (r.flags & FX_LOC_VALID) {  // the track's good-link composition, p = D, r = the prior
      r.pose.c = r.dc * prior.c - r.ds * prior.s;
      r.pose.s = r.ds * prior.c + r.dc * prior.s;
      r.pose.tx = (r.dc * prior.tx - r.ds * prior.ty) + r.dtx;
      r.pose.ty = (r.ds * prior.tx + r.dc * prior.ty) + r.dty;
      r.pose.tz = prior.tz + r.dtz;
    }
    *out = r;
  }
  const uint32_t bit = L.final;
  for (uint32_t i = tid; i < O.n_corr; i += FXL_WG)
    if (L.flag[i] & bit) A.map_id_of_row[L.row[i]] = A.near[L.row[i]];
}

extern "C" hipError_t fxk_map_localize(hipStream_t s, const FxMapLocalizeArgs &A) {
  (void)fxk_map_grid_build(s, A.G);
  if (A.K.q_max_rows) hipLaunchKernelGGL(k_loc_search, dim3((A.K.q_max_rows + FXL_WG - 1u) / FXL_WG), dim3(FXL_WG), 0, s, A);
  hipLaunchKernelGGL(k_loc_consensus, dim3(A.K.n_scans), dim3(FXL_WG), 0, s, A);
  return hipGetLastError();
}

// bytes of the context's scratch for a map of A->G.cap landmarks and q_max_rows rows, and the pointers carved out of it: the grid's
// part of the merge's layout first (the two calls share the buffer: they are ordered on one stream), then the per-row arrays
extern "C" size_t fxk_map_localize_scratch(FxMapLocalizeArgs *A, uint8_t *base) {
  FxCarve C{base, fxk_map_merge_scratch(&A->G, base)};
  A->G.prop = A->G.pred = A->G.succ = nullptr, A->G.keep = nullptr;  // (the grid's mark leaves the merge's words alone)
  A->d2 = C.take<unsigned long long>(A->K.q_max_rows);
  A->near = C.take<int32_t>(A->K.q_max_rows);
  return C.o;
}
