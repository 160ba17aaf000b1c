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
// The row body of k_loc_search and the scan body of k_loc_consensus are fx_map_localize_body.h's search_row and consensus_scan,
// which fx_map_follow.hip runs scan after scan inside one workgroup.
// LDS of k_loc_consensus: fx_map_consensus.h's 57.9 KB.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_map_localize_body.h"
#include "fx_launch.h"

using namespace fxl;

extern "C" __global__ __launch_bounds__(FXL_WG) void k_loc_search(FxMapLocalizeArgs A) {
  const uint32_t r = blockIdx.x * FXL_WG + threadIdx.x;
  if (r >= A.K.q_max_rows) return;
  const fx_pose *priors = reinterpret_cast<const fx_pose *>(A.priors);
  search_row(A, query_view(A.K), r, [&](uint32_t scan) { return priors[scan]; });
}

extern "C" __global__ __launch_bounds__(FXL_WG) void k_loc_consensus(FxMapLocalizeArgs A) {
  __shared__ MapConsensusLds L;

  const uint32_t b = blockIdx.x;
  const fx_pose prior = reinterpret_cast<const fx_pose *>(A.priors)[b];
  consensus_scan(A, L, query_view(A.K), b, prior, reinterpret_cast<fx_localization *>(A.out) + b);
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
