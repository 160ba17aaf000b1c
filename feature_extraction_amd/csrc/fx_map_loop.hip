// fx_map_loop.hip — a loop closed in the persistent map (include/fx.h fx_map_close_loop, fx_map_loop_correct_poses): the recent
// landmarks of one segment associated with its old ones under a prior transform, the closure T fitted by fx_map_localize's
// consensus, and every landmark of the segment moved by the part of T its mid-scan has between the loop's two ends.
//
// The association is defined over ALL (query, target) pairs; the grid (fx_map_grid.h, with the search distance for its gate) only
// finds the targets that can be in reach.  Every choice is a minimum over a total order, an integer prefix, an integer minimum or
// maximum or a 32-bit sum, every fp64 value an ordered chain of + - * / sqrt on one lane (the build's -ffp-contract=off): the same
// bytes from run to run and with any number of contexts in flight.  N, the segment count and the last scan come from the map's
// header on the device; the grids are sized by max_landmarks.
//
// Launches, in stream order (FXL_WG = 256 landmarks a workgroup), after fxk_map_grid_build's five:
//   k_ml_search     a thread a landmark i < max_landmarks: is it a query (eligible, of the segment, begun within recent_scans of the
//                   last scan), its point under the prior, the walk over its 3 x 3 cells and the far bucket for the nearest OLD
//                   target (walk_nearest_old); near[i], d2[i], match_of_landmark[i] = -1; the workgroup's exclusive prefix of
//                   (query, query with a target) and the block's totals (wg_scan2)
//   k_ml_top        one workgroup: the exclusive prefix of the blocks' totals (wg_scan2_blocks); st[0] = queries, st[1] = with a target
//   k_ml_gather     a thread a landmark: a query with a target and a prefix below FX_LOOP_MAX_CORR writes its id to corr[prefix]:
//                   the correspondences in ascending id
//   k_ml_consensus  one workgroup: fx_map_consensus.h's body over the gather that reads corr[]; then the final inlier set's raw
//                   query x, y and the two scan numbers staged in the LDS the consensus no longer needs, and thread 0 reduces s0
//                   and s1, sums the pivot, composes T and decides whether the map changes; the record goes to the scratch
//                   (`fit`), the final inlier set to match_of_landmark
//   k_ml_apply      a thread a landmark i < N: when the fit says APPLIED, a landmark of the segment with alpha > 0 moves its sums,
//                   its anchor and its record under its T_alpha.  Each reads and writes its own slot only: no in-place hazard
//   k_ml_finish     one lane: last_pose, the result
// mode FX_LOOP_GIVEN needs no search: a memset of match_of_landmark, then the last three launches.
// The header is read by every launch up to k_ml_apply and written by k_ml_finish alone.
//   k_ml_poses      fx_map_loop_correct_poses: a lane a pose, the same weight and the same T_alpha
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_map_consensus.h"
#include "fx_map_grid.h"
#include "../../include/fx.h"

using namespace fxc;
using namespace fxg;

#define FXL_WG FXC_MAP_WG
#define FXL_NWAVE FXC_MAP_NWAVE
#define FXL_NONE 0xffffffffu

static_assert(sizeof(fx_map_loop_result) == 144 && sizeof(fx_map_loop_options) == 72 && sizeof(fx_map_header) == 88 && sizeof(fx_pose) == 48,
              "include/fx.h");
static_assert(FX_LOOP_MAX_CORR == FXC_MAP_MAX_CORR, "fx_map_consensus.h");

extern "C" hipError_t fxk_map_grid_build(hipStream_t s, const FxMapMergeArgs &A);
extern "C" size_t fxk_map_merge_scratch(FxMapMergeArgs *A, uint8_t *base);

namespace {
struct Rigid {
  double c, s, tx, ty, tz;
};
// what every launch needs of the state when the call runs: N, the segment count, the last scan, the resolved segment, the prior
// and the device refusals
struct Ctl {
  uint32_t N, SEG, seg, refuse;
  unsigned long long last;
  Rigid p;
};
__device__ __forceinline__ Ctl control(const FxMapLoopArgs &A) {
  Ctl C;
  const fx_map_header *H = reinterpret_cast<const fx_map_header *>(A.G.header);
  C.N = n_landmarks(A.G);
  C.SEG = H->segments;
  const uint32_t scans = H->scans;
  C.last = scans ? (unsigned long long)(scans - 1u) : 0ull;
  C.seg = A.segment == FX_LOC_LAST_SEGMENT ? (C.SEG ? C.SEG - 1u : FXL_NONE) : A.segment;
  const double *p = A.prior_device ? A.prior_device : A.prior;
  C.p.c = p[0], C.p.s = p[1], C.p.tx = p[2], C.p.ty = p[3], C.p.tz = p[4];
  const bool finite = isfinite(C.p.c) && isfinite(C.p.s) && isfinite(C.p.tx) && isfinite(C.p.ty) && isfinite(C.p.tz);
  C.refuse = (C.seg >= C.SEG || !scans ? FX_LOOP_BAD_SEGMENT : 0u) | (finite ? 0u : FX_LOOP_BAD_PRIOR);
  return C;
}
// the good-link composition of fx_map_localize's Pose clause: p o r
__device__ __forceinline__ Rigid compose(const Rigid &p, const Rigid &r) {
  Rigid o;
  o.c = p.c * r.c - p.s * r.s;
  o.s = p.s * r.c + p.c * r.s;
  o.tx = (p.c * r.tx - p.s * r.ty) + p.tx;
  o.ty = (p.s * r.tx + p.c * r.ty) + p.ty;
  o.tz = r.tz + p.tz;
  return o;
}
// a record's point under the prior
__device__ __forceinline__ void prior_point(const Rigid &P, const fx_map_landmark &R, double &wx, double &wy, double &wz) {
  wx = (P.c * R.x - P.s * R.y) + P.tx;
  wy = (P.s * R.x + P.c * R.y) + P.ty;
  wz = R.z + P.tz;
}
__device__ __forceinline__ bool is_query(const FxMapLoopArgs &A, const Ctl &C, uint32_t i, const fx_map_landmark &R) {
  return A.G.alias[i] == -1 && R.n_obs >= A.min_landmark_obs && isfinite(R.x) && isfinite(R.y) && isfinite(R.z) && R.segment == C.seg &&
         (unsigned long long)R.first_scan + A.recent_scans >= C.last;
}
// include/fx.h "Weight of a global scan interval": t2 = first_scan + last_scan, twice the mid-scan
__device__ __forceinline__ double loop_weight(unsigned long long t2, uint32_t s0, uint32_t s1) {
  const unsigned long long a = 2ull * s0, b = 2ull * s1;
  if (t2 <= a) return 0.0;
  if (t2 >= b) return 1.0;
  return (double)(t2 - a) / (double)(b - a);
}
// include/fx.h "Interpolated transform": the one statement on the device, for the landmarks, last_pose and the poses.  alpha in (0, 1]
__device__ __forceinline__ Rigid loop_transform(const Rigid &T, double px, double py, double alpha) {
  if (alpha == 1.0) return T;
  const double cu = (1.0 - alpha) + alpha * T.c, su = alpha * T.s;
  const double nrm = sqrt(cu * cu + su * su);
  Rigid o;
  o.c = cu / nrm, o.s = su / nrm;
  const double gx = (T.c * px - T.s * py) + T.tx, gy = (T.s * px + T.c * py) + T.ty;
  const double hx = px + alpha * (gx - px), hy = py + alpha * (gy - py);
  o.tx = hx - (o.c * px - o.s * py);
  o.ty = hy - (o.s * px + o.c * py);
  o.tz = alpha * T.tz;
  return o;
}
__device__ __forceinline__ Rigid transform_of(const fx_map_loop_result &r) {
  Rigid T;
  T.c = r.c, T.s = r.s, T.tx = r.tx, T.ty = r.ty, T.tz = r.tz;
  return T;
}
__device__ __forceinline__ fx_map_loop_result no_fit(const Ctl &C, uint32_t flags) {
  fx_map_loop_result r;
  r.c = C.p.c, r.s = C.p.s, r.tx = C.p.tx, r.ty = C.p.ty, r.tz = C.p.tz;
  r.dc = 1.0, r.ds = 0.0, r.dtx = 0.0, r.dty = 0.0, r.dtz = 0.0;
  r.px = 0.0, r.py = 0.0;
  r.rms = INFINITY;
  r.n_query = r.n_corr = r.n_inliers = 0u, r.flags = flags, r.moved = 0u;
  r.loop_first_scan = r.loop_last_scan = FXL_NONE, r.segment = C.seg;
  r.hyp_a = r.hyp_b = FXL_NONE, r.reserved = 0u;
  return r;
}
// "Too far" and "Apply" of a record whose T, bounds and pivot are set (mode GIVEN, or a fit with FX_LOOP_FITTED)
__device__ __forceinline__ uint32_t decide(uint32_t mode, double c) {
  if (!(c > 0.0)) return FX_LOOP_TOO_FAR;
  return mode != FX_LOOP_DRY_RUN ? FX_LOOP_APPLIED : 0u;
}
}  // namespace

extern "C" __global__ __launch_bounds__(FXL_WG) void k_ml_search(FxMapLoopArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXL_NWAVE];
  const uint32_t i = blockIdx.x * FXL_WG + threadIdx.x;
  const Ctl C = control(A);
  bool query = false;
  Near best;
  best.any = false, best.d2 = 0ull, best.id = 0u;
  if (i < C.N && !C.refuse) {
    const fx_map_landmark R = records(A.G)[i];
    if (is_query(A, C, i, R)) {
      query = true;
      double wx, wy, wz;
      prior_point(C.p, R, wx, wy, wz);
      const double tx = floor(wx * A.G.inv_edge), ty = floor(wy * A.G.inv_edge);
      grid_neighbourhood(A.G, tx, ty, [&](uint32_t b) {
        walk_nearest_old(A.G, A.min_landmark_obs, b, wx, wy, C.seg, (unsigned long long)A.min_loop_scans, C.last, best);
      });
    }
  }
  uint32_t ea, eb, ta, tb;
  wg_scan2<FXL_NWAVE>(query ? 1u : 0u, best.any ? 1u : 0u, s_w, ea, eb, ta, tb);
  if (i < A.G.cap) {
    A.near[i] = best.any ? (int32_t)best.id : -1;
    A.d2[i] = best.d2;
    A.local[i] = eb;
    if (A.match) A.match[i] = -1;
  }
  if (threadIdx.x == 0u) A.bsum[blockIdx.x] = ta, A.bsum[n_blocks + blockIdx.x] = tb;
}

extern "C" __global__ __launch_bounds__(FXL_WG) void k_ml_top(FxMapLoopArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXL_NWAVE];
  uint32_t tot_a, tot_b;
  wg_scan2_blocks<FXL_NWAVE>(A.bsum, n_blocks, s_w, tot_a, tot_b);
  if (threadIdx.x == 0u) A.st[0] = tot_a, A.st[1] = tot_b;
}

extern "C" __global__ __launch_bounds__(FXL_WG) void k_ml_gather(FxMapLoopArgs A, uint32_t n_blocks) {
  const uint32_t i = blockIdx.x * FXL_WG + threadIdx.x;
  if (i >= A.G.cap || A.near[i] < 0) return;
  const uint32_t slot = A.bsum[n_blocks + blockIdx.x] + A.local[i];
  if (slot < FX_LOOP_MAX_CORR) A.corr[slot] = i;
}

extern "C" __global__ __launch_bounds__(FXL_WG) void k_ml_consensus(FxMapLoopArgs A) {
  __shared__ MapConsensusLds L;
  const uint32_t tid = threadIdx.x;
  const Ctl C = control(A);
  fx_map_loop_result *fit = reinterpret_cast<fx_map_loop_result *>(A.fit);
  if (tid == 0u) A.st[2] = 0u;  // (k_ml_apply counts the moved landmarks into it)
  if (C.refuse || A.mode == FX_LOOP_GIVEN) {  // (uniform)
    if (tid == 0u) {
      fx_map_loop_result r = no_fit(C, C.refuse);
      if (!C.refuse) {
        r.loop_first_scan = A.given_s0, r.loop_last_scan = A.given_s1, r.px = A.given_px, r.py = A.given_py;
        r.flags = decide(A.mode, r.c);
      }
      *fit = r;
    }
    return;
  }
  const fx_map_landmark *rec = records(A.G);
  // ---- gather: the correspondences k_ml_gather listed in ascending id
  auto gather = [&](MapConsensusLds &L) {
    const uint32_t found = A.st[1];
    const uint32_t n = min(found, FX_LOOP_MAX_CORR);
    for (uint32_t k = tid; k < n; k += FXL_WG) {
      const uint32_t i = min(A.corr[k], A.G.cap - 1u);
      const uint32_t g = min((uint32_t)max(A.near[i], 0), A.G.cap - 1u);  // (a listed query has a target: the clamps never act)
      const fx_map_landmark Q = rec[i], R = rec[g];
      double wx, wy, wz;
      prior_point(C.p, Q, wx, wy, wz);
      L.xy[k] = make_double4(wx, wy, R.x, R.y);
      L.dz[k] = R.z - wz;
      L.d2[k] = A.d2[i];
      L.row[k] = i;
    }
    __syncthreads();
    return found;
  };
  MapConsensusOut O;
  const bool fitted = map_consensus(L, gather, A.inlier_dist, A.min_baseline, A.hyp_corr, O);
  const uint32_t flags = O.truncated ? FX_LOOP_TRUNCATED : 0u;
  if (!fitted) {  // (uniform)
    if (tid == 0u) {
      fx_map_loop_result r = no_fit(C, flags | FX_LOOP_NO_HYPOTHESIS);
      r.n_query = A.st[0], r.n_corr = O.n_corr;
      *fit = r;
    }
    return;
  }
  // ---- the final inlier set's query records and scan numbers into the slots' xy, which the consensus is done with (its last
  // barrier is behind every read of them): (raw x, raw y, the target's last_scan << 32 | the query's first_scan as bits)
  const uint32_t bit = L.final;
  for (uint32_t k = tid; k < O.n_corr; k += FXL_WG)
    if (L.flag[k] & bit) {
      const uint32_t i = L.row[k];
      const uint32_t g = min((uint32_t)max(A.near[i], 0), A.G.cap - 1u);
      const fx_map_landmark Q = rec[i];
      const unsigned long long scans = ((unsigned long long)rec[g].last_scan << 32) | Q.first_scan;
      L.xy[k] = make_double4(Q.x, Q.y, __longlong_as_double((long long)scans), 0.0);
    }
  __syncthreads();
  if (tid == 0u) {
    fx_map_loop_result r = no_fit(C, flags);
    r.dc = O.dc, r.ds = O.ds, r.dtx = O.dtx, r.dty = O.dty, r.dtz = O.dtz;
    r.rms = O.rms;
    r.n_query = A.st[0], r.n_corr = O.n_corr, r.n_inliers = O.n_inliers;
    r.hyp_a = O.hyp_a, r.hyp_b = O.hyp_b;
    if (O.n_inliers >= A.min_inliers) {
      Rigid D;
      D.c = O.dc, D.s = O.ds, D.tx = O.dtx, D.ty = O.dty, D.tz = O.dtz;
      const Rigid T = compose(D, C.p);
      r.c = T.c, r.s = T.s, r.tx = T.tx, r.ty = T.ty, r.tz = T.tz;
      uint32_t s0 = 0u, s1 = FXL_NONE;
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
      r.flags |= FX_LOOP_FITTED | decide(A.mode, T.c);
    }
    *fit = r;
  }
  if (A.match) {
    for (uint32_t k = tid; k < O.n_corr; k += FXL_WG)
      if (L.flag[k] & bit) A.match[L.row[k]] = A.near[L.row[k]];
  }
}

extern "C" __global__ __launch_bounds__(FXL_WG) void k_ml_apply(FxMapLoopArgs A) {
  const uint32_t i = blockIdx.x * FXL_WG + threadIdx.x;
  const fx_map_loop_result *fit = reinterpret_cast<const fx_map_loop_result *>(A.fit);
  bool moved = false;
  if ((fit->flags & FX_LOOP_APPLIED) && i < n_landmarks(A.G)) {
    fx_map_landmark *rec = reinterpret_cast<fx_map_landmark *>(A.G.records) + i;
    fx_map_landmark R = *rec;
    const double alpha = R.segment == fit->segment
                             ? loop_weight((unsigned long long)R.first_scan + R.last_scan, fit->loop_first_scan, fit->loop_last_scan)
                             : 0.0;
    moved = alpha > 0.0;
    if (moved) {
      const Rigid T = loop_transform(transform_of(*fit), fit->px, fit->py, alpha);
      const double c = T.c, s = T.s, tx = T.tx, ty = T.ty, tz = T.tz;
      double *a = A.G.acc + (size_t)i * FX_MAP_ACC;  // Sx, Sy, Sz, ax, ay, Dx, Dy, Q
      const double n = (double)R.n_obs;
      const double sx = (c * a[0] - s * a[1]) + n * tx, sy = (s * a[0] + c * a[1]) + n * ty, sz = a[2] + n * tz;
      const double ax = (c * a[3] - s * a[4]) + tx, ay = (s * a[3] + c * a[4]) + ty;
      const double dx = c * a[5] - s * a[6], dy = s * a[5] + c * a[6];
      a[0] = sx, a[1] = sy, a[2] = sz, a[3] = ax, a[4] = ay, a[5] = dx, a[6] = dy;
      if (R.n_obs) {
        map_record_from_sums(R, sx, sy, sz, dx, dy, a[7]);
        *rec = R;
      }
    }
  }
  const unsigned long long vote = __ballot(moved);
  if ((threadIdx.x & 63u) == 0u && vote) atomicAdd(&A.st[2], (uint32_t)__popcll(vote));
}

extern "C" __global__ void k_ml_finish(FxMapLoopArgs A) {
  if (blockIdx.x || threadIdx.x) return;
  fx_map_header *H = reinterpret_cast<fx_map_header *>(const_cast<void *>(A.G.header));
  fx_map_loop_result r = *reinterpret_cast<const fx_map_loop_result *>(A.fit);
  if (r.flags & FX_LOOP_APPLIED) {
    const uint32_t SEG = H->segments, scans = H->scans;
    if (SEG && SEG - 1u == r.segment && scans) {
      const double alpha = loop_weight(2ull * (scans - 1u), r.loop_first_scan, r.loop_last_scan);
      if (alpha > 0.0) {
        Rigid P;
        P.c = H->last_pose.c, P.s = H->last_pose.s, P.tx = H->last_pose.tx, P.ty = H->last_pose.ty, P.tz = H->last_pose.tz;
        const Rigid O = compose(loop_transform(transform_of(r), r.px, r.py, alpha), P);
        H->last_pose.c = O.c, H->last_pose.s = O.s, H->last_pose.tx = O.tx, H->last_pose.ty = O.ty, H->last_pose.tz = O.tz;
      }
    }
    r.moved = A.st[2];
  }
  if (A.result) *reinterpret_cast<fx_map_loop_result *>(A.result) = r;
}

extern "C" __global__ __launch_bounds__(FXL_WG) void k_ml_poses(const fx_map_loop_result *result, fx_pose *poses, uint32_t first, uint32_t n) {
  const uint32_t b = blockIdx.x * FXL_WG + threadIdx.x;
  if (b >= n || !(result->flags & FX_LOOP_APPLIED)) return;
  const double alpha = loop_weight(2ull * ((unsigned long long)first + b), result->loop_first_scan, result->loop_last_scan);
  if (!(alpha > 0.0)) return;
  fx_pose *p = poses + b;
  Rigid P;
  P.c = p->c, P.s = p->s, P.tx = p->tx, P.ty = p->ty, P.tz = p->tz;
  const Rigid O = compose(loop_transform(transform_of(*result), result->px, result->py, alpha), P);
  p->c = O.c, p->s = O.s, p->tx = O.tx, p->ty = O.ty, p->tz = O.tz;
}

extern "C" hipError_t fxk_map_loop(hipStream_t s, const FxMapLoopArgs &A) {
  const dim3 wg(FXL_WG);
  const uint32_t nl = (A.G.cap + FXL_WG - 1u) / FXL_WG;
  if (A.mode == FX_LOOP_GIVEN) {
    if (A.match) {
      const hipError_t e = hipMemsetAsync(A.match, 0xff, (size_t)A.G.cap * sizeof(int32_t), s);
      if (e != hipSuccess) return e;
    }
  } else {
    (void)fxk_map_grid_build(s, A.G);
    hipLaunchKernelGGL(k_ml_search, dim3(nl), wg, 0, s, A, nl);
    hipLaunchKernelGGL(k_ml_top, dim3(1), wg, 0, s, A, nl);
    hipLaunchKernelGGL(k_ml_gather, dim3(nl), wg, 0, s, A, nl);
  }
  hipLaunchKernelGGL(k_ml_consensus, dim3(1), wg, 0, s, A);
  if (A.mode != FX_LOOP_DRY_RUN) hipLaunchKernelGGL(k_ml_apply, dim3(nl), wg, 0, s, A);
  hipLaunchKernelGGL(k_ml_finish, dim3(1), dim3(64), 0, s, A);
  return hipGetLastError();
}

extern "C" hipError_t fxk_map_loop_poses(hipStream_t s, const void *result, void *poses, uint32_t first, uint32_t n) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_ml_poses, dim3((n + FXL_WG - 1u) / FXL_WG), dim3(FXL_WG), 0, s, reinterpret_cast<const fx_map_loop_result *>(result),
                     reinterpret_cast<fx_pose *>(poses), first, n);
  return hipGetLastError();
}

// bytes of the context's scratch for a map of A->G.cap landmarks, and the pointers carved out of it: the grid's part of the merge's
// layout first (the map calls share the buffer: they are ordered on one stream), then the loop's arrays
extern "C" size_t fxk_map_loop_scratch(FxMapLoopArgs *A, uint8_t *base) {
  size_t o = fxk_map_merge_scratch(&A->G, base);
  A->G.prop = A->G.pred = A->G.succ = nullptr, A->G.keep = nullptr;  // (the grid's mark leaves the merge's words alone)
  const size_t cap = A->G.cap, nb = (cap + FXL_WG - 1u) / FXL_WG;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += (bytes + 15u) & ~(size_t)15;
    return base ? base + at : (uint8_t *)nullptr;
  };
  A->fit = take(sizeof(fx_map_loop_result));
  A->st = (uint32_t *)take(FX_MAP_LOOP_ST_WORDS * 4u);
  A->d2 = (unsigned long long *)take(cap * 8u);
  A->near = (int32_t *)take(cap * 4u);
  A->local = (uint32_t *)take(cap * 4u);
  A->bsum = (uint32_t *)take(2u * nb * 4u);
  A->corr = (uint32_t *)take(FX_LOOP_MAX_CORR * 4u);
  return o;
}
