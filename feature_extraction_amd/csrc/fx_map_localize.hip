// fx_map_localize.hip — scans localised against the persistent map under a prior pose (include/fx.h fx_map_localize): which
// landmark each keypoint row is, and each scan's pose in the map's frame.
//
// The association is defined over ALL (row, landmark) pairs; the grid (fx_map_grid.h: fx_map_merge's, with the search distance
// for its gate) only finds the landmarks that can be in reach.  Every choice is a minimum over a total order or an integer count,
// every fp64 sum an ordered chain on one lane (the build's -ffp-contract=off): the same bytes from run to run and with any number
// of contexts in flight.  The map is only read.
//
// Launches, in stream order, after fxk_map_grid_build's five (the merge's live set: alias -1, n_obs >= 1, finite x and y):
//   k_loc_search     a thread a row r < q_max_rows: the row's scan by binary search in kp_offset (as k_track_init), the world
//                    point under the scan's prior (world_point), the walk over its 3 x 3 cells and the far bucket; the walk
//                    applies min_landmark_obs, the finite z and the segment to the candidates in reach and keeps the lowest
//                    (d2 bits, id).  Writes near[r] and d2[r] (scratch), nearest_of_row[r] when given, map_id_of_row[r] = -1
//   k_loc_consensus  one 256-thread workgroup a scan, shaped like k_register:
//     gather      the scan's rows with a landmark into LDS in ascending row by ballot + prefix (at most FX_LOC_MAX_CORR)
//     rank        the pool: the H correspondences of lowest (d2 bits, row), by counting in LDS
//     hypotheses  the samples dealt to the threads by stride, fp64; a thread walks the correspondences once (all lanes read the
//                 same LDS address, a broadcast); (count, lowest sample) reduced by shuffles, then over the wavefronts in LDS
//     refit       thread 0 runs the sequential fp64 sums; the membership tests between them are dealt to all threads
//   The hypothesis, the agreement test and the refit are fx_consensus.h's, which fx_register.hip instantiates in fp32.
// LDS of k_loc_consensus: 1024 x (32 B of xy + 8 B of d2 bits + 8 B of t_z - q_z + 4 B row + 4 B flags) + the pool = 57.9 KB.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_consensus.h"
#include "fx_map_grid.h"
#include "../../include/fx.h"

using namespace fxc;
using namespace fxg;

#define FXL_WG 256
#define FXL_NWAVE (FXL_WG / 64)
#define FXL_MAX_HYP 128u
#define FXL_IDX_BITS 13  // samples of a pool of 128: 8128 < 2^13

static_assert(sizeof(fx_localization) == 112 && sizeof(fx_localize_options) == 32 && sizeof(fx_pose) == 48, "include/fx.h");
static_assert(FXL_MAX_HYP * (FXL_MAX_HYP - 1u) / 2u < (1u << FXL_IDX_BITS), "sample index bits");
static_assert(FX_LOC_MAX_CORR < (1u << (32 - FXL_IDX_BITS)), "count bits");

extern "C" hipError_t fxk_map_grid_build(hipStream_t s, const FxMapMergeArgs &A);
extern "C" size_t fxk_map_merge_scratch(FxMapMergeArgs *A, uint8_t *base);

namespace {
// scans and rows that take part (include/fx.h: as in fx_track_landmarks)
__device__ __forceinline__ uint32_t loc_scans(const FxMapLocalizeArgs &A) { return min(min(A.n_scans, A.kp[0]), A.max_scans); }
__device__ __forceinline__ uint32_t loc_rows(const FxMapLocalizeArgs &A) { return min(min(A.kp[1], A.max_total), A.q_max_rows); }
__device__ __forceinline__ bool finite_pose(const fx_pose &P) {
  return isfinite(P.c) && isfinite(P.s) && isfinite(P.tx) && isfinite(P.ty) && isfinite(P.tz);
}
// the segment a landmark must have: false, nothing is eligible; any: every segment passes
__device__ __forceinline__ bool wanted_segment(const FxMapLocalizeArgs &A, uint32_t &seg, bool &any) {
  any = A.segment == FX_LOC_ANY_SEGMENT;
  seg = A.segment;
  if (A.segment == FX_LOC_LAST_SEGMENT) {
    const uint32_t n = reinterpret_cast<const fx_map_header *>(A.G.header)->segments;
    if (!n) return false;
    seg = n - 1u;
  }
  return true;
}
// the nearest eligible landmark so far of one row: smallest d2 (bits), then lowest id
struct Near {
  unsigned long long d2;
  uint32_t id;
  bool any;
};
__device__ __forceinline__ void walk(const FxMapLocalizeArgs &A, uint32_t b, double wx, double wy, uint32_t seg, bool any_seg, Near &best) {
  const FxMapMergeArgs &G = A.G;
  const uint32_t end = min(bucket_end(G, b), G.cap);
  for (uint32_t p = bucket_begin(G, b); p < end; ++p) {
    const FxMapMergeCand c = G.cand[p];
    const double dx = c.x - wx, dy = c.y - wy;
    const double d2 = dx * dx + dy * dy;
    if (!(d2 <= G.md2) || !(any_seg || c.segment == seg) || c.id >= G.cap) continue;
    const unsigned long long k = (unsigned long long)__double_as_longlong(d2);
    if (best.any && !(k < best.d2 || (k == best.d2 && c.id < best.id))) continue;
    const fx_map_landmark R = records(G)[c.id];  // (the grid holds the merge's live set: the rest of the eligibility is here)
    if (R.n_obs < A.min_landmark_obs || !isfinite(R.z)) continue;
    best.any = true, best.d2 = k, best.id = c.id;
  }
}
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
  if (r >= A.q_max_rows) return;
  const uint32_t S = loc_scans(A), rows = loc_rows(A);
  const uint32_t *off = kp_block_offsets(A.kp);
  Near best;
  best.any = false, best.d2 = 0ull, best.id = 0u;
  uint32_t seg;
  bool any_seg;
  if (r < rows && S && wanted_segment(A, seg, any_seg)) {
    uint32_t lo = 0u, hi = S;  // the largest b in [0, S] with kp_offset[b] <= r (kp_offset[0] = 0)
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1u) >> 1;
      if (off[mid] <= r) lo = mid;
      else hi = mid - 1u;
    }
    if (lo < S && off[lo] <= r && r < off[lo + 1u]) {
      const fx_pose P = reinterpret_cast<const fx_pose *>(A.priors)[lo];
      const float4 k = kp_block_rows<float4>(A.kp, A.max_scans)[r];
      if (finite_pose(P) && finite3(k)) {
        double wx, wy, wz;
        world_point(P, k, wx, wy, wz);
        const double tx = floor(wx * A.G.inv_edge), ty = floor(wy * A.G.inv_edge);
        grid_neighbourhood(A.G, tx, ty, [&](uint32_t b) { walk(A, b, wx, wy, seg, any_seg, best); });
      }
    }
  }
  const int32_t g = best.any ? (int32_t)best.id : -1;
  A.near[r] = g;
  A.d2[r] = best.d2;
  A.map_id_of_row[r] = -1;
  if (A.nearest_of_row) A.nearest_of_row[r] = g;
}

extern "C" __global__ __launch_bounds__(FXL_WG) void k_loc_consensus(FxMapLocalizeArgs A) {
  __shared__ double4 s_xy[FX_LOC_MAX_CORR];             // (qx, qy, tx, ty): the world point under the prior, the landmark
  __shared__ unsigned long long s_d2[FX_LOC_MAX_CORR];  // d2 bits of the association
  __shared__ double s_dz[FX_LOC_MAX_CORR];              // t_z - q_z
  __shared__ uint32_t s_row[FX_LOC_MAX_CORR];
  __shared__ uint32_t s_flag[FX_LOC_MAX_CORR];  // bit 0 / 1 = member of the first / second inlier set
  __shared__ uint32_t s_pool[FXL_MAX_HYP];      // pool rank -> correspondence
  __shared__ uint32_t s_wave[FXL_NWAVE];
  __shared__ Fit s_fit;
  __shared__ uint32_t s_final;  // the flag bit of the final inlier set

  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, b = blockIdx.x;
  const uint32_t S = loc_scans(A), rows = loc_rows(A);
  const fx_pose prior = reinterpret_cast<const fx_pose *>(A.priors)[b];
  fx_localization *out = reinterpret_cast<fx_localization *>(A.out) + b;
  if (b >= S || !finite_pose(prior)) {  // (uniform)
    if (tid == 0u) write_no_fit(out, prior, 0u, b >= S ? FX_LOC_NO_SCAN : FX_LOC_BAD_PRIOR);
    return;
  }
  const uint32_t *off = kp_block_offsets(A.kp);
  const float4 *kp = kp_block_rows<float4>(A.kp, A.max_scans);
  const fx_map_landmark *rec = records(A.G);
  const uint32_t q_lo = min(off[b], rows), q_hi = max(min(off[b + 1u], rows), q_lo);

  // ---- gather: the correspondences in ascending row, the first FX_LOC_MAX_CORR kept
  uint32_t found = 0u;  // (uniform)
  for (unsigned long long r0 = q_lo; r0 < q_hi && found <= FX_LOC_MAX_CORR; r0 += FXL_WG) {
    const uint32_t i = (uint32_t)min(r0 + tid, (unsigned long long)q_hi);
    int32_t g = -1;
    if (i < q_hi) g = A.near[i];
    const bool ok = g >= 0 && (uint32_t)g < A.G.cap;
    const unsigned long long bal = __ballot(ok);
    if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = 0u, all = 0u;
#pragma unroll
    for (uint32_t w = 0; w < FXL_NWAVE; ++w) {
      const uint32_t n = s_wave[w];
      before += w < wave ? n : 0u;
      all += n;
    }
    const uint32_t slot = found + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    if (ok && slot < FX_LOC_MAX_CORR) {
      const fx_map_landmark R = rec[g];
      double wx, wy, wz;
      world_point(prior, kp[i], wx, wy, wz);
      s_xy[slot] = make_double4(wx, wy, R.x, R.y);
      s_dz[slot] = R.z - wz;
      s_d2[slot] = A.d2[i];
      s_row[slot] = i;
    }
    found += all;
    __syncthreads();  // (s_wave is written again next round)
  }
  const uint32_t n_corr = min(found, FX_LOC_MAX_CORR);
  uint32_t flags = found > FX_LOC_MAX_CORR ? FX_LOC_TRUNCATED : 0u;
  const uint32_t H = min(n_corr, A.hyp_corr);

  // ---- rank the pool: correspondence i has rank #{j : (d2_j, j) < (d2_i, i)} (rows ascend with i); ranks below H are the pool
  for (uint32_t i = tid; i < n_corr; i += FXL_WG) {
    const unsigned long long di = s_d2[i];
    uint32_t rank = 0u;
    for (uint32_t j = 0; j < n_corr && rank < H; ++j) {
      const unsigned long long dj = s_d2[j];
      rank += (dj < di || (dj == di && j < i)) ? 1u : 0u;
    }
    if (rank < H) s_pool[rank] = i;
  }
  __syncthreads();

  // ---- hypotheses: key = count << 13 | (8191 - sample), the maximum wins: most agreeing, then the lowest sample
  const double idd = (double)A.inlier_dist, mbd = (double)A.min_baseline;
  const double mb2 = mbd * mbd, gate = 2.0 * idd, id2 = idd * idd;
  const uint32_t n_samples = H * (H - (H ? 1u : 0u)) / 2u;
  uint32_t best = 0u;
  for (uint32_t idx = tid; idx < n_samples; idx += FXL_WG) {
    uint32_t a, c;
    sample_ranks(idx, H, a, c);
    Hyp<double> h;
    if (!hypothesis(s_xy[s_pool[a]], s_xy[s_pool[c]], mb2, gate, h)) continue;
    uint32_t count = 0u;
    for (uint32_t i = 0; i < n_corr; ++i) count += agrees(h, s_xy[i], id2) ? 1u : 0u;
    if (count >= 2u) best = max(best, (count << FXL_IDX_BITS) | (((1u << FXL_IDX_BITS) - 1u) - idx));
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o, 64));
  if (lane == 0u) s_wave[wave] = best;
  __syncthreads();
  best = max(max(s_wave[0], s_wave[1]), max(s_wave[2], s_wave[3]));

  if (!best) {  // (uniform) fewer than 2 correspondences, or no sample passed the gates with 2 agreeing
    if (tid == 0u) write_no_fit(out, prior, n_corr, flags | FX_LOC_NO_HYPOTHESIS);
    return;
  }

  // ---- the winner's agreeing set (bit 0): the same operations give the same bits
  uint32_t wa, wb;
  sample_ranks(((1u << FXL_IDX_BITS) - 1u) - (best & ((1u << FXL_IDX_BITS) - 1u)), H, wa, wb);
  const uint32_t n0 = best >> FXL_IDX_BITS;
  Hyp<double> h0;
  (void)hypothesis(s_xy[s_pool[wa]], s_xy[s_pool[wb]], mb2, gate, h0);
  for (uint32_t i = tid; i < n_corr; i += FXL_WG) s_flag[i] = agrees(h0, s_xy[i], id2) ? 1u : 0u;
  __syncthreads();
  if (tid == 0u) {
    Fit f;
    f.c = h0.c, f.s = h0.s;
    fit_set(s_xy, s_flag, n_corr, 1u, n0, f);
    s_fit = f;
  }
  __syncthreads();
  // ---- the set the first fit agrees with (bit 1)
  {
    const Fit f = s_fit;
    for (uint32_t i = tid; i < n_corr; i += FXL_WG) s_flag[i] |= residual2(f, s_xy[i]) <= id2 ? 2u : 0u;
  }
  __syncthreads();
  if (tid == 0u) {
    Fit f = s_fit;
    uint32_t n1 = 0u;
    for (uint32_t i = 0; i < n_corr; ++i) n1 += (s_flag[i] >> 1) & 1u;
    uint32_t bit = 1u, n = n0;
    if (n1 >= 2u) {
      bit = 2u, n = n1;
      fit_set(s_xy, s_flag, n_corr, bit, n, f);
    }
    double sz = 0.0, sr = 0.0;
    for (uint32_t i = 0; i < n_corr; ++i)
      if (s_flag[i] & bit) {
        sz += s_dz[i];
        sr += residual2(f, s_xy[i]);
      }
    fx_localization r;
    r.pose = prior;
    r.dc = f.c, r.ds = f.s, r.dtx = f.tx, r.dty = f.ty, r.dtz = sz / (double)n;
    r.rms = (float)sqrt(sr / (double)n);
    r.n_corr = n_corr, r.n_inliers = n, r.flags = flags | (n >= A.min_inliers ? FX_LOC_VALID : 0u);
    r.hyp_a = s_row[s_pool[wa]], r.hyp_b = s_row[s_pool[wb]];
    if (r.flags & FX_LOC_VALID) {  // the track's good-link composition, p = D, r = the prior
      r.pose.c = r.dc * prior.c - r.ds * prior.s;
      r.pose.s = r.ds * prior.c + r.dc * prior.s;
      r.pose.tx = (r.dc * prior.tx - r.ds * prior.ty) + r.dtx;
      r.pose.ty = (r.ds * prior.tx + r.dc * prior.ty) + r.dty;
      r.pose.tz = prior.tz + r.dtz;
    }
    *out = r;
    s_final = bit;
  }
  __syncthreads();
  const uint32_t bit = s_final;
  for (uint32_t i = tid; i < n_corr; i += FXL_WG)
    if (s_flag[i] & bit) A.map_id_of_row[s_row[i]] = A.near[s_row[i]];
}

extern "C" hipError_t fxk_map_localize(hipStream_t s, const FxMapLocalizeArgs &A) {
  (void)fxk_map_grid_build(s, A.G);
  if (A.q_max_rows) hipLaunchKernelGGL(k_loc_search, dim3((A.q_max_rows + FXL_WG - 1u) / FXL_WG), dim3(FXL_WG), 0, s, A);
  hipLaunchKernelGGL(k_loc_consensus, dim3(A.n_scans), dim3(FXL_WG), 0, s, A);
  return hipGetLastError();
}

// bytes of the context's scratch for a map of A->G.cap landmarks and q_max_rows rows, and the pointers carved out of it: the grid's
// part of the merge's layout first (the two calls share the buffer: they are ordered on one stream), then the per-row arrays
extern "C" size_t fxk_map_localize_scratch(FxMapLocalizeArgs *A, uint8_t *base) {
  size_t o = fxk_map_merge_scratch(&A->G, base);
  A->G.prop = A->G.pred = A->G.succ = nullptr, A->G.keep = nullptr;  // (the grid's mark leaves the merge's words alone)
  const size_t n = A->q_max_rows;
  A->d2 = (unsigned long long *)(base ? base + o : nullptr);
  o += (n * 8u + 15u) & ~(size_t)15;
  A->near = (int32_t *)(base ? base + o : nullptr);
  o += (n * 4u + 15u) & ~(size_t)15;
  return o;
}
