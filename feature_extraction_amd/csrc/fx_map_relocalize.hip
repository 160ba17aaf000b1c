// fx_map_relocalize.hip — a scan's pose in the persistent map without a prior (include/fx.h fx_map_relocalize): pairs of keypoints
// (seeds) are laid on pairs of landmarks of the same length, and each rigid transform that results is scored by the keypoints it
// lands on a landmark.
//
// The seed, hypothesis, score, winner and rival clauses are fx_map_constellation.h's (fx_map_find_loop shares them), with the two
// grids they walk (P, the pair grid, and Q, the score grid: built by fx_map_grid.hip, alive together in the context's scratch);
// the walks filter by the eligibility bytes k_rl_elig writes.  Every decision is an integer or a minimum / maximum over a total
// order, every fp64 value an ordered chain on one lane (the build's -ffp-contract=off): the same bytes from run to run and with
// any number of contexts in flight.  The map is only read.
//
// Launches, in stream order, after fxk_map_grid_build's five for P and five for Q:
//   k_rl_elig     a thread a landmark: eligible or not (alias -1 and fx_scan_query.h's wanted_segment and record_eligible)
//   k_rl_prep     a workgroup a scan: map_id_of_row = -1 (all workgroups share the rows), the first FX_RELOC_MAX_KP finite rows in
//                 ascending row (wg_ordered_slot), the candidate pairs' d2 in LDS, their ranks by counting, the first max_seeds
//   k_rl_hyp<0>   a workgroup a (scan, seed, FXR_CHUNK slots of P): a lane a landmark g; it walks the h about g, forms the
//                 hypothesis a -> g, b -> h and scores it: the scan's keypoints come from LDS, each image walks Q's 3 x 3 cells.
//                 The lane keeps its best (score, lowest h); the workgroup's best (score, lowest g, lowest h) goes to `partial`,
//                 the hypotheses counted go to n_hyp (64-bit integer atomic add)
//   k_rl_reduce   a workgroup a scan: the partials' best by (score, lowest seed, lowest g, lowest h); the winner's transform
//   k_rl_hyp<1>   the same enumeration; a hypothesis is scored only when it is a rival of the winner; the best score among them
//                 by a 32-bit integer atomic max
//   k_rl_finish   a wavefront a scan: the landmark of every keypoint under the winner (lowest (d2 bits, id) in reach), t_z, the
//                 flags, the record, map_id_of_row of a VALID scan
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_map_constellation.h"
#include "fx_scan_query.h"
#include "fx_launch.h"
#include "../../include/fx.h"

using namespace fxs;

static_assert(sizeof(fx_relocalization) == 96 && sizeof(fx_relocalize_options) == 40 && sizeof(fx_pose) == 48, "include/fx.h");
static_assert(FX_RELOC_MAX_KP == FXR_MAX_PT, "fx_map_constellation.h");


namespace {
// the search of scan b
__device__ __forceinline__ Search search_of(const FxMapRelocalizeArgs &A, uint32_t b) {
  Search S;
  S.P = &A.P, S.Q = &A.Q, S.elig = A.elig;
  S.pt = A.kq + (size_t)b * FX_RELOC_MAX_KP * 3u;
  S.n_pt = A.meta[4u * b], S.n_seeds = A.meta[4u * b + 1u];
  S.seeds = A.seeds + (size_t)b * FX_RELOC_MAX_KP;
  S.inlier_dist = A.inlier_dist, S.pair_tol = A.pair_tol, S.min_baseline = A.min_baseline;
  S.max_seeds = A.max_seeds, S.chunks = A.chunks;
  S.partial = A.partial + (size_t)b * A.max_seeds * A.chunks;
  S.win = A.win + b, S.n_hyp = A.n_hyp + b, S.runner = A.runner + b;
  return S;
}
}  // namespace

extern "C" __global__ __launch_bounds__(FXR_WG) void k_rl_elig(FxMapRelocalizeArgs A) {
  const uint32_t i = blockIdx.x * FXR_WG + threadIdx.x;
  if (i >= A.P.cap) return;
  uint32_t seg;
  bool any_seg;
  const bool ok = i < n_landmarks(A.P) && wanted_segment(A.P.header, A.segment, seg, any_seg) && A.P.alias[i] == -1 &&
                  record_eligible(records(A.P)[i], A.min_landmark_obs, any_seg, seg);
  A.elig[i] = ok ? 1 : 0;
}

extern "C" __global__ __launch_bounds__(FXR_WG) void k_rl_prep(FxMapRelocalizeArgs A) {
  __shared__ double s_x[FX_RELOC_MAX_KP], s_y[FX_RELOC_MAX_KP];
  __shared__ unsigned long long s_key[FXR_MAX_PAIRS];  // d2 bits of a candidate pair, 0: no candidate (mb mb is never 0)
  __shared__ uint32_t s_wave[FXR_NWAVE];
  __shared__ uint32_t s_count;

  const uint32_t tid = threadIdx.x, b = blockIdx.x;
  for (unsigned long long r = (unsigned long long)b * FXR_WG + tid; r < A.K.q_max_rows; r += (unsigned long long)A.K.n_scans * FXR_WG)
    A.map_id_of_row[r] = -1;
  if (tid == 0u) A.n_hyp[b] = 0ull, A.runner[b] = 0u, s_count = 0u;
  const KpView V = query_view(A.K);
  uint32_t *meta = A.meta + 4u * b;
  if (b >= V.S) {  // (uniform)
    if (tid < 4u) meta[tid] = 0u;
    return;
  }
  uint32_t q_lo, q_hi;
  scan_rows(V, b, q_lo, q_hi);

  // ---- the used keypoints: the finite rows in ascending row, the first FX_RELOC_MAX_KP kept
  uint32_t found = 0u;  // (uniform)
  for (unsigned long long r0 = q_lo; r0 < q_hi && found <= FX_RELOC_MAX_KP; r0 += FXR_WG) {
    const uint32_t i = (uint32_t)min(r0 + tid, (unsigned long long)q_hi);
    float4 k = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < q_hi) k = V.kp[i];
    const bool ok = i < q_hi && finite3(k);
    uint32_t slot, all;
    wg_ordered_slot<FXR_NWAVE>(ok, s_wave, found, slot, all);
    if (ok && slot < FX_RELOC_MAX_KP) {
      double *q = A.kq + ((size_t)b * FX_RELOC_MAX_KP + slot) * 3u;
      q[0] = (double)k.x, q[1] = (double)k.y, q[2] = (double)k.z;
      A.krow[(size_t)b * FX_RELOC_MAX_KP + slot] = i;
      s_x[slot] = (double)k.x, s_y[slot] = (double)k.y;
    }
    found += all;
    __syncthreads();  // (s_wave is written again next round)
  }
  const uint32_t n_kp = min(found, FX_RELOC_MAX_KP);
  __syncthreads();

  // ---- the seeds: the candidate pairs ranked by descending d2 bits, then ascending (a, c)
  rank_seeds(s_x, s_y, n_kp, A.min_baseline, A.max_baseline, A.max_seeds, A.seeds + (size_t)b * FX_RELOC_MAX_KP, s_key, &s_count);
  if (tid == 0u) {
    meta[0] = n_kp, meta[1] = min(s_count, A.max_seeds), meta[2] = found > FX_RELOC_MAX_KP ? FX_RELOC_TRUNCATED : 0u, meta[3] = 0u;
  }
}

template <int PASS>
__global__ __launch_bounds__(FXR_WG) void k_rl_hyp(FxMapRelocalizeArgs A) {
  hyp_block<PASS>(search_of(A, A.scan0 + blockIdx.z), blockIdx.y, blockIdx.x);
}

extern "C" __global__ __launch_bounds__(FXR_WG) void k_rl_reduce(FxMapRelocalizeArgs A) { reduce_block(search_of(A, blockIdx.x)); }

extern "C" __global__ __launch_bounds__(64) void k_rl_finish(FxMapRelocalizeArgs A) {
  __shared__ int32_t s_lm[FX_RELOC_MAX_KP];
  __shared__ uint32_t s_valid;
  const uint32_t tid = threadIdx.x, b = blockIdx.x;
  const uint32_t S = query_scans(A.K);
  const uint32_t n_kp = min(A.meta[4u * b], FX_RELOC_MAX_KP), n_seeds = A.meta[4u * b + 1u], trunc = A.meta[4u * b + 2u];
  const FxRelocWinner W = A.win[b];
  const double idd = (double)A.inlier_dist;
  const double *kq = A.kq + (size_t)b * FX_RELOC_MAX_KP * 3u;
  int32_t lm = -1;
  if (W.score && tid < n_kp) {
    Hyp<double> T;
    T.c = W.c, T.s = W.s, T.tx = W.tx, T.ty = W.ty;
    double wx, wy;
    image(T, kq[3u * tid], kq[3u * tid + 1u], wx, wy);
    lm = nearest(A.Q, A.elig, wx, wy, idd * idd);
  }
  s_lm[tid] = lm;
  __syncthreads();
  if (tid == 0u) {
    fx_relocalization r;
    r.pose.c = 1.0, r.pose.s = 0.0, r.pose.tx = 0.0, r.pose.ty = 0.0, r.pose.tz = 0.0, r.pose.segment = 0u, r.pose.flags = 0u;
    r.n_hyp = A.n_hyp[b];
    r.n_kp = n_kp, r.n_seeds = n_seeds, r.score = 0u, r.runner_up = 0u;
    r.seed_a = r.seed_b = r.lm_a = r.lm_b = 0xffffffffu;
    r.reserved = 0u;
    if (b >= S) {
      r.flags = FX_RELOC_NO_SCAN;
    } else if (!W.score) {
      r.flags = trunc | FX_RELOC_NO_HYPOTHESIS;
    } else {
      double sz = 0.0;
      uint32_t n = 0u;
      for (uint32_t k = 0; k < n_kp; ++k)
        if (s_lm[k] >= 0) {
          sz += records(A.P)[s_lm[k]].z - kq[3u * k + 2u];
          ++n;
        }
      const uint32_t seed = A.seeds[(size_t)b * FX_RELOC_MAX_KP + W.seed];
      r.pose.c = W.c, r.pose.s = W.s, r.pose.tx = W.tx, r.pose.ty = W.ty, r.pose.tz = sz / (double)n;
      r.pose.segment = records(A.P)[W.g].segment;
      r.score = n, r.runner_up = A.runner[b];
      r.seed_a = A.krow[(size_t)b * FX_RELOC_MAX_KP + (seed & 255u)], r.seed_b = A.krow[(size_t)b * FX_RELOC_MAX_KP + ((seed >> 8) & 255u)];
      r.lm_a = W.g, r.lm_b = W.h;
      const bool enough = r.score >= A.min_inliers, clear = r.score - r.runner_up >= A.min_margin && r.score >= r.runner_up;
      r.flags = trunc | (enough ? (clear ? FX_RELOC_VALID : FX_RELOC_AMBIGUOUS) : 0u);
    }
    reinterpret_cast<fx_relocalization *>(A.out)[b] = r;
    s_valid = r.flags & FX_RELOC_VALID;
  }
  __syncthreads();
  if (s_valid && lm >= 0) {
    const uint32_t row = A.krow[(size_t)b * FX_RELOC_MAX_KP + tid];
    if (row < A.K.q_max_rows) A.map_id_of_row[row] = lm;
  }
}

extern "C" hipError_t fxk_map_relocalize(hipStream_t s, const FxMapRelocalizeArgs &A) {
  (void)fxk_map_grid_build(s, A.P);
  (void)fxk_map_grid_build(s, A.Q);
  hipLaunchKernelGGL(k_rl_elig, dim3((A.P.cap + FXR_WG - 1u) / FXR_WG), dim3(FXR_WG), 0, s, A);
  hipLaunchKernelGGL(k_rl_prep, dim3(A.K.n_scans), dim3(FXR_WG), 0, s, A);
  auto hyp = [&](int pass) {  // (a grid's z holds 65535 scans)
    FxMapRelocalizeArgs B = A;
    for (B.scan0 = 0u; B.scan0 < A.K.n_scans; B.scan0 += 65535u) {
      const uint32_t n = A.K.n_scans - B.scan0 < 65535u ? A.K.n_scans - B.scan0 : 65535u;
      const dim3 grid(A.chunks, A.max_seeds, n);
      if (pass == 0) hipLaunchKernelGGL(k_rl_hyp<0>, grid, dim3(FXR_WG), 0, s, B);
      else hipLaunchKernelGGL(k_rl_hyp<1>, grid, dim3(FXR_WG), 0, s, B);
    }
  };
  hyp(0);
  hipLaunchKernelGGL(k_rl_reduce, dim3(A.K.n_scans), dim3(FXR_WG), 0, s, A);
  hyp(1);
  hipLaunchKernelGGL(k_rl_finish, dim3(A.K.n_scans), dim3(64), 0, s, A);
  return hipGetLastError();
}

// bytes of the context's scratch for a map of A->P.cap landmarks and n_scans scans, and the pointers carved out of it: the pair
// grid in the merge's layout first, the score grid in the same layout behind it, then the call's own arrays
extern "C" size_t fxk_map_relocalize_scratch(FxMapRelocalizeArgs *A, uint8_t *base) {
  FxCarve C{base, fxk_map_merge_scratch(&A->P, base)};
  C.o += fxk_map_merge_scratch(&A->Q, base ? base + C.o : nullptr);
  A->P.prop = A->P.pred = A->P.succ = nullptr, A->P.keep = nullptr;  // (the grid's mark leaves the merge's words alone)
  A->Q.prop = A->Q.pred = A->Q.succ = nullptr, A->Q.keep = nullptr;
  const size_t n = A->K.n_scans, K = FX_RELOC_MAX_KP;
  A->kq = C.take<double>(n * K * 3u);
  A->n_hyp = C.take<unsigned long long>(n);
  A->win = C.take<FxRelocWinner>(n);
  A->partial = C.take<FxRelocPartial>(n * A->max_seeds * A->chunks);
  A->krow = C.take<uint32_t>(n * K);
  A->seeds = C.take<uint32_t>(n * K);
  A->meta = C.take<uint32_t>(n * 4u);
  A->runner = C.take<uint32_t>(n);
  A->elig = C.take<uint8_t>(A->P.cap);
  return C.o;
}
