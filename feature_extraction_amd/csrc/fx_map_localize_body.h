// fx_map_localize_body.h — the two bodies of fx_map_localize (include/fx.h) as device functions: what one row's search does and
// what one scan's consensus does under a prior.  csrc/fx_map_localize.hip runs them a thread a row and a workgroup a scan over the
// priors the caller gave; csrc/fx_map_follow.hip runs them scan after scan inside one workgroup, under priors it forms on the way.
// The clauses have this one statement on the device: the two files differ only in where a scan's prior comes from.
#ifndef FX_MAP_LOCALIZE_BODY_H_
#define FX_MAP_LOCALIZE_BODY_H_
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_map_consensus.h"
#include "fx_map_grid.h"
#include "fx_scan_query.h"
#include "../../include/fx.h"

#define FXL_WG FXC_MAP_WG
#define FXL_NWAVE FXC_MAP_NWAVE

static_assert(sizeof(fx_localization) == 112 && sizeof(fx_localize_options) == 32 && sizeof(fx_pose) == 48, "include/fx.h");
static_assert(FX_LOC_MAX_CORR == FXC_MAP_MAX_CORR, "fx_map_consensus.h");

namespace fxl {
using namespace fxc;
using namespace fxg;

__device__ __forceinline__ void write_no_fit(fx_localization *out, const fx_pose &prior, uint32_t n_corr, uint32_t flags) {
  fx_localization r;
  r.pose = prior;
  r.dc = 1.0, r.ds = 0.0, r.dtx = 0.0, r.dty = 0.0, r.dtz = 0.0;
  r.rms = INFINITY;
  r.n_corr = n_corr, r.n_inliers = 0u, r.flags = flags;
  r.hyp_a = r.hyp_b = 0xffffffffu;
  *out = r;
}

// the row body of k_loc_search: row r < q_max_rows of the view V under prior_of(the row's scan).  Writes near[r], d2[r],
// map_id_of_row[r] = -1 and nearest_of_row[r] when given
template <typename PriorOf>
__device__ __forceinline__ void search_row(const FxMapLocalizeArgs &A, const KpView &V, uint32_t r, PriorOf prior_of) {
  Near best;
  best.any = false, best.d2 = 0ull, best.id = 0u;
  uint32_t seg, scan;
  bool any_seg;
  if (r < V.rows && V.S && wanted_segment(A.G.header, A.segment, seg, any_seg) && scan_of_row(V.off, V.S, r, scan)) {
    const fx_pose P = prior_of(scan);
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

// the scan body of k_loc_consensus: every thread of one FXL_WG workgroup calls it for scan b under `prior` (uniform); near[] and
// d2[] of the scan's rows are visible to the workgroup.  Thread 0 writes *out; the inlier rows get their map_id_of_row.  Every
// branch around a barrier is uniform.  L is free for another scan once the workgroup has passed a barrier behind the call.
__device__ __forceinline__ void consensus_scan(const FxMapLocalizeArgs &A, MapConsensusLds &L, const KpView &V, uint32_t b, const fx_pose &prior,
                                               fx_localization *out) {
  const uint32_t tid = threadIdx.x;
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
}  // namespace fxl
#endif
