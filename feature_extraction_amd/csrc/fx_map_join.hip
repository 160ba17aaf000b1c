// fx_map_join.hip — two segments of the persistent map made one (include/fx.h fx_map_join_segments): the landmarks of segment src
// associated with those of segment dst under a prior transform, the correction fitted by fx_map_localize's consensus, src's sums,
// anchors and records moved into dst's frame and the segments renumbered.
//
// The association is defined over ALL (query, target) pairs; the grid (fx_map_grid.h, with the search distance for its gate) only
// finds the targets that can be in reach.  Every choice is a minimum over a total order, an integer prefix or a 32-bit sum, every
// fp64 value an ordered chain on one lane (the build's -ffp-contract=off): the same bytes from run to run and with any number of
// contexts in flight.  N and the segment count come from the map's header on the device; the grids are sized by max_landmarks.
//
// Launches, in stream order (FXJ_WG = 256 landmarks a workgroup), after fxk_map_grid_build's five:
//   k_mj_search     a thread a landmark i < max_landmarks: is it a query (alias -1, n_obs >= min_landmark_obs, finite x y z, segment
//                   src), its point under the prior, the walk over its 3 x 3 cells and the far bucket for the nearest target (the
//                   walk is fx_map_localize's, with segment dst); near[i], d2[i], match_of_landmark[i] = -1; the workgroup's
//                   exclusive prefix of (query, query with a target) and the block's totals (wg_scan2)
//   k_mj_top        one workgroup: the exclusive prefix of the blocks' totals (wg_scan2_blocks); st[0] = queries, st[1] = with a target
//   k_mj_gather     a thread a landmark: a query with a target and a prefix below FX_JOIN_MAX_CORR writes its id to corr[prefix]:
//                   the correspondences in ascending id
//   k_mj_consensus  one workgroup: fx_map_consensus.h's body over the gather that reads corr[]; thread 0 composes T and decides
//                   whether the map changes; the record goes to the scratch (`fit`), the final inlier set to match_of_landmark
//   k_mj_apply      a thread a landmark i < N: when the fit says APPLIED, a landmark of segment src moves its sums, its anchor and
//                   its record; every landmark takes its new label.  Each reads and writes its own slot only: no in-place hazard
//   k_mj_finish     one lane: header.segments, last_pose, the result
// mode FX_JOIN_GIVEN needs no search: a memset of match_of_landmark, then the last three launches.
// The header is read by every launch up to k_mj_apply and written by k_mj_finish alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_map_consensus.h"
#include "fx_map_grid.h"
#include "../../include/fx.h"

using namespace fxc;
using namespace fxg;

#define FXJ_WG FXC_MAP_WG
#define FXJ_NWAVE FXC_MAP_NWAVE
#define FXJ_NONE 0xffffffffu

static_assert(sizeof(fx_map_join_result) == 120 && sizeof(fx_map_join_options) == 32 && sizeof(fx_map_header) == 88, "include/fx.h");
static_assert(FX_JOIN_MAX_CORR == FXC_MAP_MAX_CORR, "fx_map_consensus.h");

extern "C" hipError_t fxk_map_grid_build(hipStream_t s, const FxMapMergeArgs &A);
extern "C" size_t fxk_map_merge_scratch(FxMapMergeArgs *A, uint8_t *base);

namespace {
struct Rigid {
  double c, s, tx, ty, tz;
};
// what every launch needs of the state when the call runs: N, the segment count, the prior and the device refusals
struct Ctl {
  uint32_t N, SEG, refuse;
  Rigid p;
};
__device__ __forceinline__ Ctl control(const FxMapJoinArgs &A) {
  Ctl C;
  C.N = n_landmarks(A.G);
  C.SEG = reinterpret_cast<const fx_map_header *>(A.G.header)->segments;
  const double *p = A.prior_device ? A.prior_device : A.prior;
  C.p.c = p[0], C.p.s = p[1], C.p.tx = p[2], C.p.ty = p[3], C.p.tz = p[4];
  const bool finite = isfinite(C.p.c) && isfinite(C.p.s) && isfinite(C.p.tx) && isfinite(C.p.ty) && isfinite(C.p.tz);
  C.refuse = (A.src >= C.SEG || A.dst >= C.SEG ? FX_JOIN_BAD_SEGMENT : 0u) | (finite ? 0u : FX_JOIN_BAD_PRIOR);
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
__device__ __forceinline__ bool is_query(const FxMapJoinArgs &A, uint32_t i, const fx_map_landmark &R) {
  return A.G.alias[i] == -1 && R.n_obs >= A.min_landmark_obs && isfinite(R.x) && isfinite(R.y) && isfinite(R.z) && R.segment == A.src;
}
__device__ __forceinline__ fx_map_join_result no_fit(const Rigid &prior, uint32_t flags) {
  fx_map_join_result r;
  r.c = prior.c, r.s = prior.s, r.tx = prior.tx, r.ty = prior.ty, r.tz = prior.tz;
  r.dc = 1.0, r.ds = 0.0, r.dtx = 0.0, r.dty = 0.0, r.dtz = 0.0;
  r.rms = INFINITY;
  r.n_src = r.n_corr = r.n_inliers = 0u, r.flags = flags, r.moved = 0u, r.label = FXJ_NONE, r.segments = 0u;
  r.hyp_a = r.hyp_b = FXJ_NONE;
  return r;
}
}  // namespace

extern "C" __global__ __launch_bounds__(FXJ_WG) void k_mj_search(FxMapJoinArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXJ_NWAVE];
  const uint32_t i = blockIdx.x * FXJ_WG + threadIdx.x;
  const Ctl C = control(A);
  bool query = false;
  Near best;
  best.any = false, best.d2 = 0ull, best.id = 0u;
  if (i < C.N && !C.refuse) {
    const fx_map_landmark R = records(A.G)[i];
    if (is_query(A, i, R)) {
      query = true;
      double wx, wy, wz;
      prior_point(C.p, R, wx, wy, wz);
      const double tx = floor(wx * A.G.inv_edge), ty = floor(wy * A.G.inv_edge);
      grid_neighbourhood(A.G, tx, ty, [&](uint32_t b) { walk_nearest(A.G, A.min_landmark_obs, b, wx, wy, A.dst, false, best); });
    }
  }
  uint32_t ea, eb, ta, tb;
  wg_scan2<FXJ_NWAVE>(query ? 1u : 0u, best.any ? 1u : 0u, s_w, ea, eb, ta, tb);
  if (i < A.G.cap) {
    A.near[i] = best.any ? (int32_t)best.id : -1;
    A.d2[i] = best.d2;
    A.local[i] = eb;
    if (A.match) A.match[i] = -1;
  }
  if (threadIdx.x == 0u) A.bsum[blockIdx.x] = ta, A.bsum[n_blocks + blockIdx.x] = tb;
}

extern "C" __global__ __launch_bounds__(FXJ_WG) void k_mj_top(FxMapJoinArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXJ_NWAVE];
  uint32_t tot_a, tot_b;
  wg_scan2_blocks<FXJ_NWAVE>(A.bsum, n_blocks, s_w, tot_a, tot_b);
  if (threadIdx.x == 0u) A.st[0] = tot_a, A.st[1] = tot_b;
}

extern "C" __global__ __launch_bounds__(FXJ_WG) void k_mj_gather(FxMapJoinArgs A, uint32_t n_blocks) {
  const uint32_t i = blockIdx.x * FXJ_WG + threadIdx.x;
  if (i >= A.G.cap || A.near[i] < 0) return;
  const uint32_t slot = A.bsum[n_blocks + blockIdx.x] + A.local[i];
  if (slot < FX_JOIN_MAX_CORR) A.corr[slot] = i;
}

extern "C" __global__ __launch_bounds__(FXJ_WG) void k_mj_consensus(FxMapJoinArgs A) {
  __shared__ MapConsensusLds L;
  const uint32_t tid = threadIdx.x;
  const Ctl C = control(A);
  fx_map_join_result *fit = reinterpret_cast<fx_map_join_result *>(A.fit);
  if (tid == 0u) A.st[2] = 0u;  // (k_mj_apply counts the moved landmarks into it)
  if (C.refuse || A.mode == FX_JOIN_GIVEN) {  // (uniform)
    if (tid == 0u) *fit = no_fit(C.p, C.refuse ? C.refuse : FX_JOIN_APPLIED);
    return;
  }
  const fx_map_landmark *rec = records(A.G);
  // ---- gather: the correspondences k_mj_gather listed in ascending id
  auto gather = [&](MapConsensusLds &L) {
    const uint32_t found = A.st[1];
    const uint32_t n = min(found, FX_JOIN_MAX_CORR);
    for (uint32_t k = tid; k < n; k += FXJ_WG) {
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
  const uint32_t flags = O.truncated ? FX_JOIN_TRUNCATED : 0u;
  if (!fitted) {  // (uniform)
    if (tid == 0u) {
      fx_map_join_result r = no_fit(C.p, flags | FX_JOIN_NO_HYPOTHESIS);
      r.n_src = A.st[0], r.n_corr = O.n_corr;
      *fit = r;
    }
    return;
  }
  if (tid == 0u) {
    fx_map_join_result r = no_fit(C.p, flags);
    r.dc = O.dc, r.ds = O.ds, r.dtx = O.dtx, r.dty = O.dty, r.dtz = O.dtz;
    r.rms = O.rms;
    r.n_src = A.st[0], r.n_corr = O.n_corr, r.n_inliers = O.n_inliers;
    r.hyp_a = O.hyp_a, r.hyp_b = O.hyp_b;
    if (O.n_inliers >= A.min_inliers) {
      Rigid D;
      D.c = O.dc, D.s = O.ds, D.tx = O.dtx, D.ty = O.dty, D.tz = O.dtz;
      const Rigid T = compose(D, C.p);
      r.c = T.c, r.s = T.s, r.tx = T.tx, r.ty = T.ty, r.tz = T.tz;
      r.flags |= FX_JOIN_FITTED | (A.mode == FX_JOIN_FIT ? FX_JOIN_APPLIED : 0u);
    }
    *fit = r;
  }
  if (A.match) {
    const uint32_t bit = L.final;
    for (uint32_t k = tid; k < O.n_corr; k += FXJ_WG)
      if (L.flag[k] & bit) A.match[L.row[k]] = A.near[L.row[k]];
  }
}

extern "C" __global__ __launch_bounds__(FXJ_WG) void k_mj_apply(FxMapJoinArgs A) {
  const uint32_t i = blockIdx.x * FXJ_WG + threadIdx.x;
  const fx_map_join_result *fit = reinterpret_cast<const fx_map_join_result *>(A.fit);
  bool moved = false;
  if ((fit->flags & FX_JOIN_APPLIED) && i < n_landmarks(A.G)) {
    fx_map_landmark *rec = reinterpret_cast<fx_map_landmark *>(A.G.records) + i;
    fx_map_landmark R = *rec;
    moved = R.segment == A.src;
    if (moved) {
      const double c = fit->c, s = fit->s, tx = fit->tx, ty = fit->ty, tz = fit->tz;
      double *a = A.G.acc + (size_t)i * FX_MAP_ACC;  // Sx, Sy, Sz, ax, ay, Dx, Dy, Q
      const double n = (double)R.n_obs;
      const double sx = (c * a[0] - s * a[1]) + n * tx, sy = (s * a[0] + c * a[1]) + n * ty, sz = a[2] + n * tz;
      const double ax = (c * a[3] - s * a[4]) + tx, ay = (s * a[3] + c * a[4]) + ty;
      const double dx = c * a[5] - s * a[6], dy = s * a[5] + c * a[6];
      a[0] = sx, a[1] = sy, a[2] = sz, a[3] = ax, a[4] = ay, a[5] = dx, a[6] = dy;
      if (R.n_obs) map_record_from_sums(R, sx, sy, sz, dx, dy, a[7]);
    }
    const uint32_t lo = min(A.src, A.dst), hi = max(A.src, A.dst);
    R.segment = R.segment == lo ? hi - 1u : (R.segment > lo ? R.segment - 1u : R.segment);
    *rec = R;
  }
  const unsigned long long vote = __ballot(moved);
  if ((threadIdx.x & 63u) == 0u && vote) atomicAdd(&A.st[2], (uint32_t)__popcll(vote));
}

extern "C" __global__ void k_mj_finish(FxMapJoinArgs A) {
  if (blockIdx.x || threadIdx.x) return;
  fx_map_header *H = reinterpret_cast<fx_map_header *>(const_cast<void *>(A.G.header));
  fx_map_join_result r = *reinterpret_cast<const fx_map_join_result *>(A.fit);
  const uint32_t SEG = H->segments;
  if (r.flags & FX_JOIN_APPLIED) {
    if (SEG - 1u == A.src) {
      Rigid T, P;
      T.c = r.c, T.s = r.s, T.tx = r.tx, T.ty = r.ty, T.tz = r.tz;
      P.c = H->last_pose.c, P.s = H->last_pose.s, P.tx = H->last_pose.tx, P.ty = H->last_pose.ty, P.tz = H->last_pose.tz;
      const Rigid O = compose(T, P);
      H->last_pose.c = O.c, H->last_pose.s = O.s, H->last_pose.tx = O.tx, H->last_pose.ty = O.ty, H->last_pose.tz = O.tz;
    }
    H->segments = SEG - 1u;
    r.moved = A.st[2];
    r.label = max(A.src, A.dst) - 1u;
  }
  r.segments = H->segments;
  if (A.result) *reinterpret_cast<fx_map_join_result *>(A.result) = r;
}

extern "C" hipError_t fxk_map_join(hipStream_t s, const FxMapJoinArgs &A) {
  const dim3 wg(FXJ_WG);
  const uint32_t nl = (A.G.cap + FXJ_WG - 1u) / FXJ_WG;
  if (A.mode == FX_JOIN_GIVEN) {
    if (A.match) {
      const hipError_t e = hipMemsetAsync(A.match, 0xff, (size_t)A.G.cap * sizeof(int32_t), s);
      if (e != hipSuccess) return e;
    }
  } else {
    (void)fxk_map_grid_build(s, A.G);
    hipLaunchKernelGGL(k_mj_search, dim3(nl), wg, 0, s, A, nl);
    hipLaunchKernelGGL(k_mj_top, dim3(1), wg, 0, s, A, nl);
    hipLaunchKernelGGL(k_mj_gather, dim3(nl), wg, 0, s, A, nl);
  }
  hipLaunchKernelGGL(k_mj_consensus, dim3(1), wg, 0, s, A);
  if (A.mode != FX_JOIN_DRY_RUN) hipLaunchKernelGGL(k_mj_apply, dim3(nl), wg, 0, s, A);
  hipLaunchKernelGGL(k_mj_finish, dim3(1), dim3(64), 0, s, A);
  return hipGetLastError();
}

// bytes of the context's scratch for a map of A->G.cap landmarks, and the pointers carved out of it: the grid's part of the merge's
// layout first (the map calls share the buffer: they are ordered on one stream), then the join's arrays
extern "C" size_t fxk_map_join_scratch(FxMapJoinArgs *A, uint8_t *base) {
  size_t o = fxk_map_merge_scratch(&A->G, base);
  A->G.prop = A->G.pred = A->G.succ = nullptr, A->G.keep = nullptr;  // (the grid's mark leaves the merge's words alone)
  const size_t cap = A->G.cap, nb = (cap + FXJ_WG - 1u) / FXJ_WG;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += (bytes + 15u) & ~(size_t)15;
    return base ? base + at : (uint8_t *)nullptr;
  };
  A->fit = take(sizeof(fx_map_join_result));
  A->st = (uint32_t *)take(FX_MAP_JOIN_ST_WORDS * 4u);
  A->d2 = (unsigned long long *)take(cap * 8u);
  A->near = (int32_t *)take(cap * 4u);
  A->local = (uint32_t *)take(cap * 4u);
  A->bsum = (uint32_t *)take(2u * nb * 4u);
  A->corr = (uint32_t *)take(FX_JOIN_MAX_CORR * 4u);
  return o;
}
