// fx_map_join.hip — two segments of the persistent map made one (include/fx.h fx_map_join_segments): the landmarks of segment src
// associated with those of segment dst under a prior transform, the correction fitted by fx_map_localize's consensus, src's sums,
// anchors and records moved into dst's frame and the segments renumbered.
//
// The association, its launches and their order are csrc/fx_map_assoc.h's (shared with fx_map_close_loop); N and the segment count
// come from the map's header on the device.  What is the join's own:
//   k_mj_search     the queries are the eligible landmarks of segment src, the targets those of segment dst
//   k_mj_consensus  one workgroup: fx_map_consensus.h's body over fx_map_assoc.h's gather; thread 0 composes T and decides whether
//                   the map changes; the record goes to the scratch (`fit`), the final inlier set to match_of_landmark
//   k_mj_apply      a thread a landmark i < N: when the fit says APPLIED, a landmark of segment src moves its sums, its anchor and
//                   its record; every landmark takes its new label.  Each reads and writes its own slot only: no in-place hazard
//   k_mj_finish     one lane: header.segments, last_pose, the result
// The header is read by every launch up to k_mj_apply and written by k_mj_finish alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_map_assoc.h"
#include "fx_launch.h"
#include "../../include/fx.h"

using namespace fxc;
using namespace fxg;
using namespace fxa;

static_assert(sizeof(fx_map_join_result) == 120 && sizeof(fx_map_join_options) == 32 && sizeof(fx_map_header) == 88, "include/fx.h");
static_assert(FX_JOIN_MAX_CORR == FXC_MAP_MAX_CORR, "fx_map_consensus.h");

namespace {
// what every launch needs of the state when the call runs: N, the segment count, the prior and the device refusals
struct Ctl {
  uint32_t N, SEG, refuse;
  Rigid p;
};
__device__ __forceinline__ Ctl control(const FxMapJoinArgs &A) {
  Ctl C;
  C.N = n_landmarks(A.S.G);
  C.SEG = reinterpret_cast<const fx_map_header *>(A.S.G.header)->segments;
  const bool finite = load_prior(A.S, C.p);
  C.refuse = (A.src >= C.SEG || A.dst >= C.SEG ? FX_JOIN_BAD_SEGMENT : 0u) | (finite ? 0u : FX_JOIN_BAD_PRIOR);
  return C;
}
__device__ __forceinline__ fx_map_join_result no_fit(const Rigid &prior, uint32_t flags) {
  fx_map_join_result r;
  store_rigid(r, prior);
  r.dc = 1.0, r.ds = 0.0, r.dtx = 0.0, r.dty = 0.0, r.dtz = 0.0;
  r.rms = INFINITY;
  r.n_src = r.n_corr = r.n_inliers = 0u, r.flags = flags, r.moved = 0u, r.label = FXA_NONE, r.segments = 0u;
  r.hyp_a = r.hyp_b = FXA_NONE;
  return r;
}
}  // namespace

extern "C" __global__ __launch_bounds__(FXA_WG) void k_mj_search(FxMapJoinArgs A, uint32_t n_blocks) {
  const Ctl C = control(A);
  search(
      A.S, C.N, C.refuse, C.p, n_blocks, [&](uint32_t i, const fx_map_landmark &R) { return eligible(A.S, i, R) && R.segment == A.src; },
      [&](const FxMapMergeCand &c) { return c.segment == A.dst; });
}

extern "C" __global__ __launch_bounds__(FXA_WG) void k_mj_consensus(FxMapJoinArgs A) {
  __shared__ MapConsensusLds L;
  const FxMapAssocArgs &S = A.S;
  const uint32_t tid = threadIdx.x;
  const Ctl C = control(A);
  fx_map_join_result *fit = reinterpret_cast<fx_map_join_result *>(S.fit);
  if (tid == 0u) S.st[2] = 0u;  // (k_mj_apply counts the moved landmarks into it)
  if (C.refuse || S.mode == FX_JOIN_GIVEN) {  // (uniform)
    if (tid == 0u) *fit = no_fit(C.p, C.refuse ? C.refuse : FX_JOIN_APPLIED);
    return;
  }
  MapConsensusOut O;
  const bool fitted = map_consensus(L, CorrGather{S, C.p}, S.inlier_dist, S.min_baseline, S.hyp_corr, O);
  const uint32_t flags = O.truncated ? FX_JOIN_TRUNCATED : 0u;
  if (!fitted) {  // (uniform)
    if (tid == 0u) {
      fx_map_join_result r = no_fit(C.p, flags | FX_JOIN_NO_HYPOTHESIS);
      r.n_src = S.st[0], r.n_corr = O.n_corr;
      *fit = r;
    }
    return;
  }
  if (tid == 0u) {
    fx_map_join_result r = no_fit(C.p, flags);
    r.dc = O.dc, r.ds = O.ds, r.dtx = O.dtx, r.dty = O.dty, r.dtz = O.dtz;
    r.rms = O.rms;
    r.n_src = S.st[0], r.n_corr = O.n_corr, r.n_inliers = O.n_inliers;
    r.hyp_a = O.hyp_a, r.hyp_b = O.hyp_b;
    if (O.n_inliers >= S.min_inliers) {
      Rigid D;
      D.c = O.dc, D.s = O.ds, D.tx = O.dtx, D.ty = O.dty, D.tz = O.dtz;
      store_rigid(r, compose(D, C.p));
      r.flags |= FX_JOIN_FITTED | (S.mode == FX_JOIN_FIT ? FX_JOIN_APPLIED : 0u);
    }
    *fit = r;
  }
  write_inliers(S, L, O.n_corr);
}

extern "C" __global__ __launch_bounds__(FXA_WG) void k_mj_apply(FxMapJoinArgs A) {
  const FxMapAssocArgs &S = A.S;
  const uint32_t i = blockIdx.x * FXA_WG + threadIdx.x;
  const fx_map_join_result *fit = reinterpret_cast<const fx_map_join_result *>(S.fit);
  bool moved = false;
  if ((fit->flags & FX_JOIN_APPLIED) && i < n_landmarks(S.G)) {
    fx_map_landmark *rec = reinterpret_cast<fx_map_landmark *>(S.G.records) + i;
    fx_map_landmark R = *rec;
    moved = R.segment == A.src;
    if (moved) move_landmark(S.G.acc + (size_t)i * FX_MAP_ACC, R, load_rigid(*fit));
    const uint32_t lo = min(A.src, A.dst), hi = max(A.src, A.dst);
    R.segment = R.segment == lo ? hi - 1u : (R.segment > lo ? R.segment - 1u : R.segment);
    *rec = R;
  }
  count_moved(S, moved);
}

extern "C" __global__ void k_mj_finish(FxMapJoinArgs A) {
  if (blockIdx.x || threadIdx.x) return;
  fx_map_header *H = reinterpret_cast<fx_map_header *>(const_cast<void *>(A.S.G.header));
  fx_map_join_result r = *reinterpret_cast<const fx_map_join_result *>(A.S.fit);
  const uint32_t SEG = H->segments;
  if (r.flags & FX_JOIN_APPLIED) {
    if (SEG - 1u == A.src) store_rigid(H->last_pose, compose(load_rigid(r), load_rigid(H->last_pose)));
    H->segments = SEG - 1u;
    r.moved = A.S.st[2];
    r.label = max(A.src, A.dst) - 1u;
  }
  r.segments = H->segments;
  if (A.result) *reinterpret_cast<fx_map_join_result *>(A.result) = r;
}

extern "C" hipError_t fxk_map_join(hipStream_t s, const FxMapJoinArgs &A) {
  return run(s, A, A.S.mode == FX_JOIN_GIVEN, A.S.mode == FX_JOIN_DRY_RUN, k_mj_search, k_mj_consensus, k_mj_apply, k_mj_finish);
}

extern "C" size_t fxk_map_join_scratch(FxMapJoinArgs *A, uint8_t *base) { return fxk_map_assoc_scratch(&A->S, base, sizeof(fx_map_join_result)); }
