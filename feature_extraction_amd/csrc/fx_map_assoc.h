// fx_map_assoc.h — what fx_map_join_segments (csrc/fx_map_join.hip) and fx_map_close_loop (csrc/fx_map_loop.hip) share: one set of
// the map's landmarks (the queries) associated with another (the targets) under a prior rigid transform, the correction fitted by
// fx_map_localize's consensus (csrc/fx_map_consensus.h), and landmarks moved under the transform that comes of it.  What differs
// between the calls arrives as a value or a predicate; nothing here asks which call it serves.
//
// Every fp64 expression is an ordered chain on one lane (the build's -ffp-contract=off): compose, prior_point and move_landmark
// are the one statement of their chains, so the calls cannot drift apart.
//
// The launches of a call, in stream order (FXA_WG = 256 landmarks a workgroup), after fxk_map_grid_build's five:
//   search      the call's kernel around search(): a thread a landmark i < max_landmarks: is it a query, its point under the prior,
//               the walk over its 3 x 3 cells and the far bucket for the nearest target the call accepts; near[i], d2[i],
//               match_of_landmark[i] = -1; the workgroup's exclusive prefix of (query, query with a target) and the block's totals
//   k_ma_top    one workgroup: the exclusive prefix of the blocks' totals (wg_scan2_blocks); st[0] = queries, st[1] = with a target
//   k_ma_gather a thread a landmark: a query with a target and a prefix below FXC_MAP_MAX_CORR writes its id to corr[prefix]:
//               the correspondences in ascending id
//   consensus, apply, finish   the call's own kernels, built from CorrGather, write_inliers, move_landmark and count_moved
// mode GIVEN needs no search: a memset of match_of_landmark, then the last three launches.  DRY_RUN skips apply.
#ifndef FX_MAP_ASSOC_H_
#define FX_MAP_ASSOC_H_
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fx_map_consensus.h"
#include "fx_map_grid.h"
#include "fx_launch.h"
#include "fx_rigid.h"
#include "fx_scan_query.h"

#define FXA_WG FXC_MAP_WG
#define FXA_NWAVE FXC_MAP_NWAVE
#define FXA_NONE 0xffffffffu


namespace fxa {
// (Rigid: csrc/fx_rigid.h)
// a Rigid from / into anything with the members c, s, tx, ty, tz: an fx_pose, the head of a result record
template <typename P>
__device__ __forceinline__ Rigid load_rigid(const P &p) {
  Rigid r;
  r.c = p.c, r.s = p.s, r.tx = p.tx, r.ty = p.ty, r.tz = p.tz;
  return r;
}
template <typename P>
__device__ __forceinline__ void store_rigid(P &p, const Rigid &r) {
  p.c = r.c, p.s = r.s, p.tx = r.tx, p.ty = r.ty, p.tz = r.tz;
}
// the call's prior, from the device when the caller gave it there; false: a component is not finite (the device refusal)
__device__ __forceinline__ bool load_prior(const FxMapAssocArgs &S, Rigid &P) {
  const double *p = S.prior_device ? S.prior_device : S.prior;
  P.c = p[0], P.s = p[1], P.tx = p[2], P.ty = p[3], P.tz = p[4];
  return isfinite(P.c) && isfinite(P.s) && isfinite(P.tx) && isfinite(P.ty) && isfinite(P.tz);
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
// the part of a query's eligibility every call asks for
__device__ __forceinline__ bool eligible(const FxMapAssocArgs &S, uint32_t i, const fx_map_landmark &R) {
  return S.G.alias[i] == -1 && record_eligible(R, S.min_landmark_obs);
}

// The body of a call's search kernel.  N, refuse, prior: the call's control; is_query(i, record): is landmark i a query;
// accept(candidate): may this FxMapMergeCand be a target (walk_nearest applies the gate, the order and the rest of the eligibility).
template <typename IsQuery, typename Accept>
__device__ __forceinline__ void search(const FxMapAssocArgs &S, uint32_t N, uint32_t refuse, const Rigid &prior, uint32_t n_blocks, IsQuery is_query,
                                       Accept accept) {
  __shared__ uint32_t s_w[2 * FXA_NWAVE];
  const uint32_t i = blockIdx.x * FXA_WG + threadIdx.x;
  bool query = false;
  fxg::Near best;
  best.any = false, best.d2 = 0ull, best.id = 0u;
  if (i < N && !refuse) {
    const fx_map_landmark R = fxg::records(S.G)[i];
    if (is_query(i, R)) {
      query = true;
      double wx, wy, wz;
      prior_point(prior, R, wx, wy, wz);
      const double tx = floor(wx * S.G.inv_edge), ty = floor(wy * S.G.inv_edge);
      fxg::grid_neighbourhood(S.G, tx, ty, [&](uint32_t b) { fxg::walk_nearest(S.G, S.min_landmark_obs, b, wx, wy, accept, best); });
    }
  }
  uint32_t ea, eb, ta, tb;
  wg_scan2<FXA_NWAVE>(query ? 1u : 0u, best.any ? 1u : 0u, s_w, ea, eb, ta, tb);
  if (i < S.G.cap) {
    S.near[i] = best.any ? (int32_t)best.id : -1;
    S.d2[i] = best.d2;
    S.local[i] = eb;
    if (S.match) S.match[i] = -1;
  }
  if (threadIdx.x == 0u) S.bsum[blockIdx.x] = ta, S.bsum[n_blocks + blockIdx.x] = tb;
}

// fx_map_consensus.h's gather over the correspondences k_ma_gather listed in ascending id
struct CorrGather {
  const FxMapAssocArgs &S;
  const Rigid &prior;
  __device__ __forceinline__ uint32_t operator()(fxc::MapConsensusLds &L) const {
    const fx_map_landmark *rec = fxg::records(S.G);
    const uint32_t found = S.st[1];
    const uint32_t n = min(found, FXC_MAP_MAX_CORR);
    for (uint32_t k = threadIdx.x; k < n; k += FXA_WG) {
      const uint32_t i = min(S.corr[k], S.G.cap - 1u);
      const uint32_t g = min((uint32_t)max(S.near[i], 0), S.G.cap - 1u);  // (a listed query has a target: the clamps never act)
      const fx_map_landmark Q = rec[i], R = rec[g];
      double wx, wy, wz;
      prior_point(prior, Q, wx, wy, wz);
      L.xy[k] = make_double4(wx, wy, R.x, R.y);
      L.dz[k] = R.z - wz;
      L.d2[k] = S.d2[i];
      L.row[k] = i;
    }
    __syncthreads();
    return found;
  }
};
// the final inlier set to match_of_landmark
__device__ __forceinline__ void write_inliers(const FxMapAssocArgs &S, const fxc::MapConsensusLds &L, uint32_t n_corr) {
  if (!S.match) return;
  const uint32_t bit = L.final;
  for (uint32_t k = threadIdx.x; k < n_corr; k += FXA_WG)
    if (L.flag[k] & bit) S.match[L.row[k]] = S.near[L.row[k]];
}
// a landmark's sums a = (Sx, Sy, Sz, ax, ay, Dx, Dy, Q), its anchor and (when it has observations) its record under T
__device__ __forceinline__ void move_landmark(double *a, fx_map_landmark &R, const Rigid &T) {
  const double c = T.c, s = T.s, tx = T.tx, ty = T.ty, tz = T.tz;
  const double n = (double)R.n_obs;
  const double sx = (c * a[0] - s * a[1]) + n * tx, sy = (s * a[0] + c * a[1]) + n * ty, sz = a[2] + n * tz;
  const double ax = (c * a[3] - s * a[4]) + tx, ay = (s * a[3] + c * a[4]) + ty;
  const double dx = c * a[5] - s * a[6], dy = s * a[5] + c * a[6];
  a[0] = sx, a[1] = sy, a[2] = sz, a[3] = ax, a[4] = ay, a[5] = dx, a[6] = dy;
  if (R.n_obs) map_record_from_sums(R, sx, sy, sz, dx, dy, a[7]);
}
// the moved landmarks counted into st[2], a wavefront's at once (every lane of the workgroup calls it)
__device__ __forceinline__ void count_moved(const FxMapAssocArgs &S, bool moved) { count_wave(moved, &S.st[2]); }

// A call's launches (the list above).  Args: the call's arguments, whose member S is the shared part; the kernels are the call's.
template <typename Args>
hipError_t run(hipStream_t s, const Args &A, bool given, bool dry_run, void (*k_search)(Args, uint32_t), void (*k_consensus)(Args),
               void (*k_apply)(Args), void (*k_finish)(Args)) {
  const FxMapAssocArgs &S = A.S;
  const dim3 wg(FXA_WG);
  const uint32_t nl = (S.G.cap + FXA_WG - 1u) / FXA_WG;
  if (given) {
    if (S.match) {
      const hipError_t e = hipMemsetAsync(S.match, 0xff, (size_t)S.G.cap * sizeof(int32_t), s);
      if (e != hipSuccess) return e;
    }
  } else {
    (void)fxk_map_grid_build(s, S.G);
    hipLaunchKernelGGL(k_search, dim3(nl), wg, 0, s, A, nl);
    fxk_map_assoc_rank(s, S, nl);
  }
  hipLaunchKernelGGL(k_consensus, dim3(1), wg, 0, s, A);
  if (!dry_run) hipLaunchKernelGGL(k_apply, dim3(nl), wg, 0, s, A);
  hipLaunchKernelGGL(k_finish, dim3(1), dim3(64), 0, s, A);
  return hipGetLastError();
}
}  // namespace fxa
#endif
