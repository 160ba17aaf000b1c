// fx_map_loop.hip — a loop closed in the persistent map (include/fx.h fx_map_close_loop, fx_map_loop_correct_poses): the recent
// landmarks of one segment associated with its old ones under a prior transform, the closure T fitted by fx_map_localize's
// consensus, and every landmark of the segment moved by the part of T its mid-scan has between the loop's two ends.
//
// The association, its launches and their order are csrc/fx_map_assoc.h's (shared with fx_map_join_segments); N, the segment count
// and the last scan come from the map's header on the device.  Beside that file's chains every fp64 value here is an ordered chain
// of + - * / sqrt on one lane, every other choice an integer minimum or maximum.  What is the loop's own:
//   k_ml_search     the queries are the eligible landmarks of the segment begun within recent_scans of the last scan, the targets
//                   the segment's OLD ones: (uint64)last_scan + min_loop_scans <= the last scan
//   k_ml_consensus  one workgroup: fx_map_consensus.h's body over fx_map_assoc.h's gather; then the final inlier set's raw
//                   query x, y and the two scan numbers staged in the LDS the consensus no longer needs, and thread 0 reduces s0
//                   and s1, sums the pivot, composes T and decides whether the map changes; the record goes to the scratch
//                   (`fit`), the final inlier set to match_of_landmark
//   k_ml_apply      a thread a landmark i < N: when the fit says APPLIED, a landmark of the segment with alpha > 0 moves its sums,
//                   its anchor and its record under its T_alpha.  Each reads and writes its own slot only: no in-place hazard
//   k_ml_finish     one lane: last_pose, the result
// The header is read by every launch up to k_ml_apply and written by k_ml_finish alone.
//   k_ml_poses      fx_map_loop_correct_poses: a lane a pose, the same weight and the same T_alpha
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

static_assert(sizeof(fx_map_loop_result) == 144 && sizeof(fx_map_loop_options) == 72 && sizeof(fx_map_header) == 88 && sizeof(fx_pose) == 48,
              "include/fx.h");
static_assert(FX_LOOP_MAX_CORR == FXC_MAP_MAX_CORR, "fx_map_consensus.h");

namespace {
// what every launch needs of the state when the call runs: N, the segment count, the last scan, the resolved segment, the prior
// and the device refusals
struct Ctl {
  uint32_t N, SEG, seg, refuse;
  unsigned long long last;
  Rigid p;
};
__device__ __forceinline__ Ctl control(const FxMapLoopArgs &A) {
  Ctl C;
  const fx_map_header *H = reinterpret_cast<const fx_map_header *>(A.S.G.header);
  C.N = n_landmarks(A.S.G);
  C.SEG = H->segments;
  const uint32_t scans = H->scans;
  C.last = scans ? (unsigned long long)(scans - 1u) : 0ull;
  C.seg = A.segment == FX_LOC_LAST_SEGMENT ? (C.SEG ? C.SEG - 1u : FXA_NONE) : A.segment;
  const bool finite = load_prior(A.S, C.p);
  C.refuse = (C.seg >= C.SEG || !scans ? FX_LOOP_BAD_SEGMENT : 0u) | (finite ? 0u : FX_LOOP_BAD_PRIOR);
  return C;
}
// include/fx.h "Weight of a global scan interval": t2 = first_scan + last_scan, twice the mid-scan
__device__ __forceinline__ double loop_weight(unsigned long long t2, uint32_t s0, uint32_t s1) {
  const unsigned long long a = 2ull * s0, b = 2ull * s1;
  if (t2 <= a) return 0.0;
  if (t2 >= b) return 1.0;
  return (double)(t2 - a) / (double)(b - a);
}
// (include/fx.h "Interpolated transform" is csrc/fx_rigid.h's loop_transform, which fx_deskew_keypoint_block shares)
__device__ __forceinline__ fx_map_loop_result no_fit(const Ctl &C, uint32_t flags) {
  fx_map_loop_result r;
  store_rigid(r, C.p);
  r.dc = 1.0, r.ds = 0.0, r.dtx = 0.0, r.dty = 0.0, r.dtz = 0.0;
  r.px = 0.0, r.py = 0.0;
  r.rms = INFINITY;
  r.n_query = r.n_corr = r.n_inliers = 0u, r.flags = flags, r.moved = 0u;
  r.loop_first_scan = r.loop_last_scan = FXA_NONE, r.segment = C.seg;
  r.hyp_a = r.hyp_b = FXA_NONE, r.reserved = 0u;
  return r;
}
// "Too far" and "Apply" of a record whose T, bounds and pivot are set (mode GIVEN, or a fit with FX_LOOP_FITTED)
__device__ __forceinline__ uint32_t decide(uint32_t mode, double c) {
  if (!(c > 0.0)) return FX_LOOP_TOO_FAR;
  return mode != FX_LOOP_DRY_RUN ? FX_LOOP_APPLIED : 0u;
}
}  // namespace

extern "C" __global__ __launch_bounds__(FXA_WG) void k_ml_search(FxMapLoopArgs A, uint32_t n_blocks) {
  const Ctl C = control(A);
  const unsigned long long min_loop = A.min_loop_scans;
  search(
      A.S, C.N, C.refuse, C.p, n_blocks,
      [&](uint32_t i, const fx_map_landmark &R) {
        return eligible(A.S, i, R) && R.segment == C.seg && (unsigned long long)R.first_scan + A.recent_scans >= C.last;
      },
      [&](const FxMapMergeCand &c) { return c.segment == C.seg && (unsigned long long)c.last_scan + min_loop <= C.last; });
}

extern "C" __global__ __launch_bounds__(FXA_WG) void k_ml_consensus(FxMapLoopArgs A) {
  __shared__ MapConsensusLds L;
  const FxMapAssocArgs &S = A.S;
  const uint32_t tid = threadIdx.x;
  const Ctl C = control(A);
  fx_map_loop_result *fit = reinterpret_cast<fx_map_loop_result *>(S.fit);
  if (tid == 0u) S.st[2] = 0u;  // (k_ml_apply counts the moved landmarks into it)
  if (C.refuse || S.mode == FX_LOOP_GIVEN) {  // (uniform)
    if (tid == 0u) {
      fx_map_loop_result r = no_fit(C, C.refuse);
      if (!C.refuse) {
        r.loop_first_scan = A.given_s0, r.loop_last_scan = A.given_s1, r.px = A.given_px, r.py = A.given_py;
        r.flags = decide(S.mode, r.c);
      }
      *fit = r;
    }
    return;
  }
  MapConsensusOut O;
  const bool fitted = map_consensus(L, CorrGather{S, C.p}, S.inlier_dist, S.min_baseline, S.hyp_corr, O);
  const uint32_t flags = O.truncated ? FX_LOOP_TRUNCATED : 0u;
  if (!fitted) {  // (uniform)
    if (tid == 0u) {
      fx_map_loop_result r = no_fit(C, flags | FX_LOOP_NO_HYPOTHESIS);
      r.n_query = S.st[0], r.n_corr = O.n_corr;
      *fit = r;
    }
    return;
  }
  // ---- the final inlier set's query records and scan numbers into the slots' xy, which the consensus is done with (its last
  // barrier is behind every read of them): (raw x, raw y, the target's last_scan << 32 | the query's first_scan as bits)
  const fx_map_landmark *rec = records(S.G);
  const uint32_t bit = L.final;
  for (uint32_t k = tid; k < O.n_corr; k += FXA_WG)
    if (L.flag[k] & bit) {
      const uint32_t i = L.row[k];
      const uint32_t g = min((uint32_t)max(S.near[i], 0), S.G.cap - 1u);
      const fx_map_landmark Q = rec[i];
      const unsigned long long scans = ((unsigned long long)rec[g].last_scan << 32) | Q.first_scan;
      L.xy[k] = make_double4(Q.x, Q.y, __longlong_as_double((long long)scans), 0.0);
    }
  __syncthreads();
  if (tid == 0u) {
    fx_map_loop_result r = no_fit(C, flags);
    r.dc = O.dc, r.ds = O.ds, r.dtx = O.dtx, r.dty = O.dty, r.dtz = O.dtz;
    r.rms = O.rms;
    r.n_query = S.st[0], r.n_corr = O.n_corr, r.n_inliers = O.n_inliers;
    r.hyp_a = O.hyp_a, r.hyp_b = O.hyp_b;
    if (O.n_inliers >= S.min_inliers) {
      Rigid D;
      D.c = O.dc, D.s = O.ds, D.tx = O.dtx, D.ty = O.dty, D.tz = O.dtz;
      const Rigid T = compose(D, C.p);
      store_rigid(r, T);
      uint32_t s0 = 0u, s1 = FXA_NONE;
      double sx = 0.0, sy = 0.0;
      for (uint32_t k = 0; k < O.n_corr; ++k)
        if (L.flag[k] & bit) {
          const double4 v = L.xy[k];
          const unsigned long long scans = (unsigned long long)__double_as_longlong(v.z);
          s0 = max(s0, (uint32_t)(scans >> 32)), s1 = min(s1, (uint32_t)scans);
          sx += v.x, sy += v.y;
        }
      const double dn = (double)O.n_inliers;
      r.loop_first_scan = s0, r.loop_last_scan = s1, r.px = sx / dn, r.py = sy / dn;
      r.flags |= FX_LOOP_FITTED | decide(S.mode, T.c);
    }
    *fit = r;
  }
  write_inliers(S, L, O.n_corr);
}

extern "C" __global__ __launch_bounds__(FXA_WG) void k_ml_apply(FxMapLoopArgs A) {
  const FxMapAssocArgs &S = A.S;
  const uint32_t i = blockIdx.x * FXA_WG + threadIdx.x;
  const fx_map_loop_result *fit = reinterpret_cast<const fx_map_loop_result *>(S.fit);
  bool moved = false;
  if ((fit->flags & FX_LOOP_APPLIED) && i < n_landmarks(S.G)) {
    fx_map_landmark *rec = reinterpret_cast<fx_map_landmark *>(S.G.records) + i;
    fx_map_landmark R = *rec;
    const double alpha = R.segment == fit->segment
                             ? loop_weight((unsigned long long)R.first_scan + R.last_scan, fit->loop_first_scan, fit->loop_last_scan)
                             : 0.0;
    moved = alpha > 0.0;
    if (moved) {
      move_landmark(S.G.acc + (size_t)i * FX_MAP_ACC, R, loop_transform(load_rigid(*fit), fit->px, fit->py, alpha));
      if (R.n_obs) *rec = R;
    }
  }
  count_moved(S, moved);
}

extern "C" __global__ void k_ml_finish(FxMapLoopArgs A) {
  if (blockIdx.x || threadIdx.x) return;
  fx_map_header *H = reinterpret_cast<fx_map_header *>(const_cast<void *>(A.S.G.header));
  fx_map_loop_result r = *reinterpret_cast<const fx_map_loop_result *>(A.S.fit);
  if (r.flags & FX_LOOP_APPLIED) {
    const uint32_t SEG = H->segments, scans = H->scans;
    if (SEG && SEG - 1u == r.segment && scans) {
      const double alpha = loop_weight(2ull * (scans - 1u), r.loop_first_scan, r.loop_last_scan);
      if (alpha > 0.0) store_rigid(H->last_pose, compose(loop_transform(load_rigid(r), r.px, r.py, alpha), load_rigid(H->last_pose)));
    }
    r.moved = A.S.st[2];
  }
  if (A.result) *reinterpret_cast<fx_map_loop_result *>(A.result) = r;
}

extern "C" __global__ __launch_bounds__(FXA_WG) void k_ml_poses(const fx_map_loop_result *result, fx_pose *poses, uint32_t first, uint32_t n) {
  const uint32_t b = blockIdx.x * FXA_WG + threadIdx.x;
  if (b >= n || !(result->flags & FX_LOOP_APPLIED)) return;
  const double alpha = loop_weight(2ull * ((unsigned long long)first + b), result->loop_first_scan, result->loop_last_scan);
  if (!(alpha > 0.0)) return;
  fx_pose *p = poses + b;
  store_rigid(*p, compose(loop_transform(load_rigid(*result), result->px, result->py, alpha), load_rigid(*p)));
}

extern "C" hipError_t fxk_map_loop(hipStream_t s, const FxMapLoopArgs &A) {
  return run(s, A, A.S.mode == FX_LOOP_GIVEN, A.S.mode == FX_LOOP_DRY_RUN, k_ml_search, k_ml_consensus, k_ml_apply, k_ml_finish);
}

extern "C" hipError_t fxk_map_loop_poses(hipStream_t s, const void *result, void *poses, uint32_t first, uint32_t n) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_ml_poses, dim3((n + FXA_WG - 1u) / FXA_WG), dim3(FXA_WG), 0, s, reinterpret_cast<const fx_map_loop_result *>(result),
                     reinterpret_cast<fx_pose *>(poses), first, n);
  return hipGetLastError();
}

extern "C" size_t fxk_map_loop_scratch(FxMapLoopArgs *A, uint8_t *base) { return fxk_map_assoc_scratch(&A->S, base, sizeof(fx_map_loop_result)); }
