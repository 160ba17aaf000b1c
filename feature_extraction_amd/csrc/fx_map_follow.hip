// fx_map_follow.hip — chains of consecutive scans followed through the persistent map (include/fx.h fx_map_follow): the prior of a
// scan is the pose of the scan before it composed with the motion between them, and the scan is then localised as
// fx_map_localize localises it under that prior.  The search and the consensus are fx_map_localize_body.h's device functions, the
// ones k_loc_search and k_loc_consensus call: nothing of the localise is restated here.  The map is only read.
//
// Launches, in stream order:
//   fxk_map_grid_build's five, ONCE a call: the map does not change while the chains run
//   k_follow_fill   a thread a row r < q_max_rows: -1 into near (scratch), map_id_of_row and nearest_of_row (when given): what the
//                   localise leaves in non-rows and in the rows of scans without a finite prior
//   k_follow        one 256-thread workgroup a chain, a loop over the chain's scans; each turn:
//     prior      thread 0 forms the scan's prior from the pose of the scan before (LDS) and the chain's state (its registers: the
//                latest usable link, the streak, the start's segment) and puts it into LDS                          | barrier
//     search     the scan's rows dealt to the threads by stride: search_row writes near, d2 (scratch) and the two row words
//                                                                                                                     | barrier
//     consensus  consensus_scan: the gather over near and d2, fx_map_consensus.h's body, the record, the inlier rows' ids
//     state      thread 0 reads the record it wrote, writes follow[b] and poses[b] and the new pose into LDS        | barrier
// A workgroup never waits for another: no tickets, no spinning, no atomics between chains.  Every branch around a barrier is
// uniform: the loop's bounds come from the arguments and blockIdx, the scan's verdict (b >= S, a prior that is not finite) from
// the prior in LDS that every thread reads behind the first barrier, and consensus_scan's own branches are uniform.
//
// MapConsensusLds is reused from scan to scan.  What a short scan could read of a longer scan before it is never read:
//   xy, d2, dz, row  map_consensus and the tail of consensus_scan read the slots [0, n_corr) only, and this scan's gather wrote
//                    exactly those (wg_ordered_slot numbers the correspondences 0, 1, ... without a gap);
//   flag             read at i < n_corr only, behind the loop that writes every flag[i], i < n_corr, with = (not |=);
//   pool             read at ranks < H = min(n_corr, hyp_corr) only; the true ranks are a permutation of [0, n_corr), the capped
//                    count equals the true rank wherever that is below H, so each of pool[0 .. H) is written once this scan;
//   wave, fit, final written this scan in front of the barrier behind which they are read; where map_consensus returns false,
//                    flag, fit and final are not read at all.
// The barrier that ends a turn stands between the last reads of a scan (flag, row, final by all threads; wave on the path
// without a hypothesis) and the next scan's first writes.  near and d2 are per row, and the scans' rows are disjoint.
// Every fp64 value is an ordered chain on one lane (the build's -ffp-contract=off); a composed prior that is not finite is
// tested and dropped, never stored: the same bytes from run to run and with any number of contexts in flight.
// Every index is bounded by the arguments: b < n_scans bounds out, follow, poses and links[b - 1]; a row r < rows <=
// min(max_total, q_max_rows) bounds the block's rows, both row arrays, near and d2; blockIdx < n_chains bounds the start poses.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_map_localize_body.h"
#include "fx_launch.h"

using namespace fxl;

#define FXF_NONE 0xffffffffu

static_assert(sizeof(fx_follow_options) == 48 && sizeof(fx_follow_scan) == 64 && sizeof(fx_registration) == 64, "include/fx.h");
static_assert(offsetof(fx_follow_scan, flags) == 48 && FX_FOLLOW_NO_MOTION == FXF_NONE, "include/fx.h");

namespace {
// include/fx.h fx_map_follow, 2: a usable link
__device__ __forceinline__ bool usable(const fx_registration &R, uint32_t require_flags) {
  return (R.flags & require_flags) == require_flags && isfinite(R.c) && isfinite(R.s) && isfinite(R.tx) && isfinite(R.ty) && isfinite(R.tz);
}
}  // namespace

extern "C" __global__ __launch_bounds__(FXL_WG) void k_follow_fill(FxMapLocalizeArgs A) {
  const uint32_t r = blockIdx.x * FXL_WG + threadIdx.x;
  if (r >= A.K.q_max_rows) return;
  A.near[r] = -1;
  A.map_id_of_row[r] = -1;
  if (A.nearest_of_row) A.nearest_of_row[r] = -1;
}

extern "C" __global__ __launch_bounds__(FXL_WG) void k_follow(FxMapFollowArgs A) {
  __shared__ MapConsensusLds L;
  __shared__ fx_pose s_pose, s_prior;  // the pose of the scan before; this scan's prior

  const uint32_t tid = threadIdx.x, j = blockIdx.x;
  const KpView V = query_view(A.L.K);
  const uint32_t f = j * A.chain_scans, e = f + min(A.chain_scans, A.L.K.n_scans - f);  // (j < n_chains: f < n_scans)
  const fx_registration *links = reinterpret_cast<const fx_registration *>(A.links);
  fx_localization *out = reinterpret_cast<fx_localization *>(A.L.out);
  fx_follow_scan *follow = reinterpret_cast<fx_follow_scan *>(A.follow);
  fx_pose *poses = reinterpret_cast<fx_pose *>(A.poses);
  uint32_t last = FXF_NONE, streak = 0u, start_segment = 0u;  // (thread 0's: the chain's state)

  for (uint32_t b = f; b < e; ++b) {
    uint32_t fl = 0u, motion = FXF_NONE;
    // ---- prior
    if (tid == 0u) {
      fx_pose P;
      if (b == f) {
        P = reinterpret_cast<const fx_pose *>(A.starts)[j];
        start_segment = P.segment;
        fl = FX_FOLLOW_START;
      } else {
        P = s_pose;  // p*
        fl = FX_FOLLOW_HELD;
        const bool own = usable(links[b - 1u], A.require_flags);
        if (own) last = b - 1u;
        if (last != FXF_NONE && b < V.S && finite_pose(P)) {
          const fx_registration M = links[last];
          const double pc = P.c, ps = P.s;  // the track's good-link composition p* o m
          const double c = pc * M.c - ps * M.s, s = ps * M.c + pc * M.s;
          const double tx = (pc * M.tx - ps * M.ty) + P.tx, ty = (ps * M.tx + pc * M.ty) + P.ty, tz = P.tz + M.tz;
          if (isfinite(c) && isfinite(s) && isfinite(tx) && isfinite(ty) && isfinite(tz)) {
            P.c = c, P.s = s, P.tx = tx, P.ty = ty, P.tz = tz;
            P.segment = start_segment, P.flags = 0u;
            fl = own ? FX_FOLLOW_LINK : FX_FOLLOW_COASTED;
            motion = last;
          }
        }
      }
      s_prior = P;
    }
    __syncthreads();
    const fx_pose prior = s_prior;
    // ---- search
    if (b < V.S && finite_pose(prior)) {  // (uniform) otherwise the fill's -1 stands, as in the localise
      uint32_t q_lo, q_hi;
      scan_rows(V, b, q_lo, q_hi);
      for (unsigned long long r = (unsigned long long)q_lo + tid; r < q_hi; r += FXL_WG)
        search_row(A.L, V, (uint32_t)r, [&](uint32_t) { return prior; });
    }
    __syncthreads();
    // ---- consensus
    consensus_scan(A.L, L, V, b, prior, out + b);
    // ---- state
    if (tid == 0u) {
      const fx_pose pose = out[b].pose;  // (this thread wrote the record)
      streak = (out[b].flags & FX_LOC_VALID) ? 0u : streak + 1u;
      fx_follow_scan F;
      F.prior = prior;
      F.flags = fl | (streak >= A.max_lost ? FX_FOLLOW_LOST : 0u), F.motion = motion;
      F.streak = streak, F.reserved = 0u;
      follow[b] = F;
      if (poses) poses[b] = pose;
      s_pose = pose;
    }
    __syncthreads();
  }
}

extern "C" hipError_t fxk_map_follow(hipStream_t s, const FxMapFollowArgs &A) {
  (void)fxk_map_grid_build(s, A.L.G);
  const uint32_t q = A.L.K.q_max_rows;
  if (q) hipLaunchKernelGGL(k_follow_fill, dim3((q + FXL_WG - 1u) / FXL_WG), dim3(FXL_WG), 0, s, A.L);
  hipLaunchKernelGGL(k_follow, dim3(A.n_chains), dim3(FXL_WG), 0, s, A);
  return hipGetLastError();
}

// the localise's carve of the context's scratch: the grid's part of the merge's layout, then near and d2
extern "C" size_t fxk_map_follow_scratch(FxMapFollowArgs *A, uint8_t *base) { return fxk_map_localize_scratch(&A->L, base); }
