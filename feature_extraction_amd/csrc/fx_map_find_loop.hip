// fx_map_find_loop.hip — a loop's closure in the persistent map without a prior (include/fx.h fx_map_find_loop): the recent
// landmarks of a segment (the queries) are laid on its old ones, or on another segment's (the targets), as fx_map_relocalize lays
// a scan's keypoints on the map's landmarks.
//
// The search is fx_map_constellation.h's, with fx_map_relocalize's two grids (P, the pair grid, and Q, the score grid: built by
// fx_map_grid.hip over the merge's live set, alive together in the context's scratch).  One eligibility byte a landmark tells
// the walks what it is: 0 neither, 1 a target (the only value the search lays a point on), 2 a candidate query.  Every decision
// is an integer or a minimum / maximum over a total order, every fp64 value an ordered chain on one lane (the build's
// -ffp-contract=off): the same bytes from run to run and with any number of contexts in flight.  The map is only read.
//
// Launches, in stream order, after a memset of n_hyp and the state words and fxk_map_grid_build's five for P and five for Q:
//   k_fl_elig     a thread a landmark: its byte (alias -1, fx_scan_query.h's record_eligible, the segment, the window),
//                 match_of_landmark = -1, n_targets by ballot and a 32-bit integer atomic add; the resolved segments and the
//                 refusal go to the state words
//   k_fl_select   one workgroup: the candidate queries in descending id, found by walking the eligibility BYTES downwards from N
//                 (16 bytes a thread at a glance, then a workgroup's 256 at a time with wg_ordered_slot where a query lies)
//                 until a 65th or id 0; the 48-byte records are read for the used queries alone; then the seeds (rank_seeds)
//   k_fl_hyp<0>   a workgroup a (seed, FXR_CHUNK slots of P): hyp_block<0>
//   k_fl_reduce   one workgroup: reduce_block
//   k_fl_hyp<1>   the same enumeration over the winner's rivals: hyp_block<1>
//   k_fl_finish   a wavefront: the target of every query under the winner (lowest (d2 bits, id) in reach), wtz, the flags, the
//                 record, match_of_landmark of a VALID result
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_map_constellation.h"
#include "fx_scan_query.h"
#include "fx_launch.h"
#include "../../include/fx.h"

using namespace fxs;

static_assert(sizeof(fx_map_loop_candidate) == 136 && sizeof(fx_map_find_loop_options) == 52, "include/fx.h");
static_assert(FX_FIND_MAX_QUERY == FXR_MAX_PT, "fx_map_constellation.h");
static_assert(FX_FIND_ST_WORDS == 8, "fx_device.h");


namespace {
#define FXF_NONE 0xffffffffu
#define FXF_SPAN (FXR_WG * 16u)  // landmarks a round of the query selection looks at

// does a word of four eligibility bytes hold a 2
__device__ __forceinline__ bool has_two(uint32_t w) {
  const uint32_t y = w ^ 0x02020202u;
  return ((y - 0x01010101u) & ~y & 0x80808080u) != 0u;
}

// what every launch needs of the header: the segments resolved and the refusal
struct Ctl {
  uint32_t N, qseg, tseg, refuse;
  bool same;                 // the targets are qseg's own old landmarks
  unsigned long long last;
};
__device__ __forceinline__ Ctl control(const FxMapFindLoopArgs &A) {
  const fx_map_header *H = reinterpret_cast<const fx_map_header *>(A.P.header);
  Ctl C;
  C.N = n_landmarks(A.P);
  const uint32_t SEG = H->segments, scans = H->scans;
  C.last = scans ? (unsigned long long)(scans - 1u) : 0ull;
  const uint32_t last_seg = SEG ? SEG - 1u : FXF_NONE;
  C.qseg = A.segment == FX_LOC_LAST_SEGMENT ? last_seg : A.segment;
  C.same = A.target_segment == FX_FIND_SAME_SEGMENT;
  C.tseg = C.same ? C.qseg : (A.target_segment == FX_LOC_LAST_SEGMENT ? last_seg : A.target_segment);
  C.refuse = (C.qseg >= SEG || C.tseg >= SEG || !scans || (!C.same && C.tseg == C.qseg)) ? FX_FIND_BAD_SEGMENT : 0u;
  return C;
}
__device__ __forceinline__ Search search_of(const FxMapFindLoopArgs &A) {
  Search S;
  S.P = &A.P, S.Q = &A.Q, S.elig = A.elig;
  S.pt = A.kq;
  S.n_pt = A.st[2], S.n_seeds = A.st[3];
  S.seeds = A.seeds;
  S.inlier_dist = A.inlier_dist, S.pair_tol = A.pair_tol, S.min_baseline = A.min_baseline;
  S.max_seeds = A.max_seeds, S.chunks = A.chunks;
  S.partial = A.partial;
  S.win = A.win, S.n_hyp = A.n_hyp, S.runner = A.st + 1;
  return S;
}
}  // namespace

extern "C" __global__ __launch_bounds__(FXR_WG) void k_fl_elig(FxMapFindLoopArgs A) {
  const uint32_t i = blockIdx.x * FXR_WG + threadIdx.x;
  const Ctl C = control(A);
  if (i == 0u) A.st[5] = C.qseg, A.st[6] = C.tseg, A.st[7] = C.refuse;
  uint8_t kind = 0;
  if (i < C.N && !C.refuse) {
    const fx_map_landmark R = records(A.P)[i];
    if (A.P.alias[i] == -1 && record_eligible(R, A.min_landmark_obs)) {
      const bool old = !C.same || (unsigned long long)R.last_scan + A.min_loop_scans <= C.last;
      if (R.segment == C.tseg && old) kind = 1;
      else if (R.segment == C.qseg && (unsigned long long)R.first_scan + A.recent_scans >= C.last) kind = 2;
    }
  }
  if (i < A.P.cap) {
    A.elig[i] = kind;
    if (A.match) A.match[i] = -1;
  }
  count_wave(kind == 1, &A.st[0]);
}

extern "C" __global__ __launch_bounds__(FXR_WG) void k_fl_select(FxMapFindLoopArgs A) {
  __shared__ double s_x[FXR_MAX_PT], s_y[FXR_MAX_PT];
  __shared__ unsigned long long s_key[FXR_MAX_PAIRS];
  __shared__ uint32_t s_wave[FXR_NWAVE];
  __shared__ uint32_t s_count;

  const uint32_t tid = threadIdx.x;
  if (tid == 0u) s_count = 0u;
  const uint32_t N = n_landmarks(A.P);
  // ---- the used queries: the bytes of value 2 in descending id, the first FX_FIND_MAX_QUERY kept (a refused call has none).  The
  // map is walked in spans of 16 bytes a thread from aligned borders; a span without a 2 costs one load and one barrier
  uint32_t found = 0u;  // (uniform)
  for (uint32_t top = N; top > 0u && found <= FX_FIND_MAX_QUERY;) {
    const uint32_t lo = (top - 1u) / FXF_SPAN * FXF_SPAN, at = lo + tid * 16u;
    bool any = false;
    if (at + 16u <= top) {
      const uint4 v = *reinterpret_cast<const uint4 *>(A.elig + at);  // (the bytes begin on a 16-byte border of the scratch)
      any = has_two(v.x) || has_two(v.y) || has_two(v.z) || has_two(v.w);
    } else {
      for (uint32_t i = at; i < top; ++i) any |= A.elig[i] == 2;
    }
    if (__syncthreads_or(any ? 1 : 0)) {
      for (uint32_t hi = top; hi > lo && found <= FX_FIND_MAX_QUERY; hi -= min(hi - lo, (uint32_t)FXR_WG)) {
        const bool in = tid < hi - lo;
        const uint32_t i = in ? hi - 1u - tid : 0u;  // (thread order is descending id)
        const bool ok = in && A.elig[i] == 2;
        uint32_t slot, all;
        wg_ordered_slot<FXR_NWAVE>(ok, s_wave, found, slot, all);
        if (ok && slot < FX_FIND_MAX_QUERY) {
          const fx_map_landmark R = records(A.P)[i];
          double *q = A.kq + (size_t)slot * 3u;
          q[0] = R.x, q[1] = R.y, q[2] = R.z;
          A.kid[slot] = i;
          s_x[slot] = R.x, s_y[slot] = R.y;
        }
        found += all;
        __syncthreads();  // (s_wave is written again next round)
      }
    }
    top = lo;
  }
  const uint32_t n_query = min(found, FX_FIND_MAX_QUERY);
  __syncthreads();
  rank_seeds(s_x, s_y, n_query, A.min_baseline, A.max_baseline, A.max_seeds, A.seeds, s_key, &s_count);
  if (tid == 0u) A.st[2] = n_query, A.st[3] = min(s_count, A.max_seeds), A.st[4] = found > FX_FIND_MAX_QUERY ? FX_FIND_TRUNCATED : 0u;
}

template <int PASS>
__global__ __launch_bounds__(FXR_WG) void k_fl_hyp(FxMapFindLoopArgs A) {
  hyp_block<PASS>(search_of(A), blockIdx.y, blockIdx.x);
}

extern "C" __global__ __launch_bounds__(FXR_WG) void k_fl_reduce(FxMapFindLoopArgs A) { reduce_block(search_of(A)); }

extern "C" __global__ __launch_bounds__(64) void k_fl_finish(FxMapFindLoopArgs A) {
  __shared__ int32_t s_lm[FXR_MAX_PT];
  __shared__ uint32_t s_valid;
  const uint32_t tid = threadIdx.x;
  const uint32_t n_query = min(A.st[2], FX_FIND_MAX_QUERY), n_seeds = A.st[3], trunc = A.st[4], refuse = A.st[7];
  const FxRelocWinner W = *A.win;
  const double idd = (double)A.inlier_dist;
  int32_t lm = -1;
  if (W.score && tid < n_query) {
    Hyp<double> T;
    T.c = W.c, T.s = W.s, T.tx = W.tx, T.ty = W.ty;
    double wx, wy;
    image(T, A.kq[3u * tid], A.kq[3u * tid + 1u], wx, wy);
    lm = nearest(A.Q, A.elig, wx, wy, idd * idd);
  }
  s_lm[tid] = lm;
  __syncthreads();
  if (tid == 0u) {
    fx_map_loop_candidate r;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    r.c = r.s = r.tx = r.ty = r.tz = nan;
    r.wc = 1.0, r.ws = 0.0, r.wtx = 0.0, r.wty = 0.0, r.wtz = 0.0;
    r.n_hyp = *A.n_hyp;
    r.n_query = n_query, r.n_targets = A.st[0], r.n_seeds = n_seeds, r.score = 0u, r.runner_up = 0u;
    r.seed_a = r.seed_b = r.lm_a = r.lm_b = FXF_NONE;
    r.segment = A.st[5], r.target_segment = A.st[6];
    if (refuse) {
      r.flags = refuse;
    } else if (!W.score) {
      r.flags = trunc | FX_FIND_NO_HYPOTHESIS;
    } else {
      double sz = 0.0;
      uint32_t n = 0u;
      for (uint32_t k = 0; k < n_query; ++k)
        if (s_lm[k] >= 0) {
          sz += records(A.P)[s_lm[k]].z - A.kq[3u * k + 2u];
          ++n;
        }
      const uint32_t seed = A.seeds[W.seed];
      r.wc = W.c, r.ws = W.s, r.wtx = W.tx, r.wty = W.ty, r.wtz = sz / (double)n;
      r.score = n, r.runner_up = A.st[1];
      r.seed_a = A.kid[seed & 255u], r.seed_b = A.kid[(seed >> 8) & 255u];
      r.lm_a = W.g, r.lm_b = W.h;
      const bool enough = r.score >= A.min_inliers, clear = r.score - r.runner_up >= A.min_margin && r.score >= r.runner_up;
      r.flags = trunc | (enough ? (clear ? FX_FIND_VALID : FX_FIND_AMBIGUOUS) : 0u);
      if (r.flags & FX_FIND_VALID) r.c = r.wc, r.s = r.ws, r.tx = r.wtx, r.ty = r.wty, r.tz = r.wtz;
    }
    *reinterpret_cast<fx_map_loop_candidate *>(A.result) = r;
    s_valid = r.flags & FX_FIND_VALID;
  }
  __syncthreads();
  if (s_valid && lm >= 0 && A.match) {  // (lm >= 0 only for tid < n_query: kid's slots beyond n_query are never written)
    const uint32_t i = A.kid[tid];
    if (i < A.P.cap) A.match[i] = lm;
  }
}

extern "C" hipError_t fxk_map_find_loop(hipStream_t s, const FxMapFindLoopArgs &A) {
  (void)hipMemsetAsync(A.n_hyp, 0, 8u + FX_FIND_ST_WORDS * 4u, s);
  (void)fxk_map_grid_build(s, A.P);
  (void)fxk_map_grid_build(s, A.Q);
  hipLaunchKernelGGL(k_fl_elig, dim3((A.P.cap + FXR_WG - 1u) / FXR_WG), dim3(FXR_WG), 0, s, A);
  hipLaunchKernelGGL(k_fl_select, dim3(1), dim3(FXR_WG), 0, s, A);
  const dim3 grid(A.chunks, A.max_seeds);
  hipLaunchKernelGGL(k_fl_hyp<0>, grid, dim3(FXR_WG), 0, s, A);
  hipLaunchKernelGGL(k_fl_reduce, dim3(1), dim3(FXR_WG), 0, s, A);
  hipLaunchKernelGGL(k_fl_hyp<1>, grid, dim3(FXR_WG), 0, s, A);
  hipLaunchKernelGGL(k_fl_finish, dim3(1), dim3(64), 0, s, A);
  return hipGetLastError();
}

// bytes of the context's scratch for a map of A->P.cap landmarks, and the pointers carved out of it: the pair grid in the merge's
// layout first, the score grid in the same layout behind it, then the call's own arrays
extern "C" size_t fxk_map_find_loop_scratch(FxMapFindLoopArgs *A, uint8_t *base) {
  FxCarve C{base, fxk_map_merge_scratch(&A->P, base)};
  C.o += fxk_map_merge_scratch(&A->Q, base ? base + C.o : nullptr);
  A->P.prop = A->P.pred = A->P.succ = nullptr, A->P.keep = nullptr;  // (the grid's mark leaves the merge's words alone)
  A->Q.prop = A->Q.pred = A->Q.succ = nullptr, A->Q.keep = nullptr;
  const size_t K = FX_FIND_MAX_QUERY;
  uint8_t *ctl = C.take<uint8_t>(8u + FX_FIND_ST_WORDS * 4u);
  A->n_hyp = (unsigned long long *)ctl;
  A->st = (uint32_t *)(ctl ? ctl + 8 : nullptr);
  A->kq = C.take<double>(K * 3u);
  A->win = C.take<FxRelocWinner>(1u);
  A->partial = C.take<FxRelocPartial>((size_t)A->max_seeds * A->chunks);
  A->kid = C.take<uint32_t>(K);
  A->seeds = C.take<uint32_t>(K);
  A->elig = C.take<uint8_t>(A->P.cap);
  return C.o;
}
