// fx_scan_query.h — what the calls that read a keypoint block as a query share (fx_track_landmarks, fx_map_localize,
// fx_map_follow, fx_map_relocalize, fx_map_observe, fx_map_expect, fx_map_discover), and the eligibility clauses and workgroup idioms of the
// map's calls.  Every decision here is part of the bit-for-bit contract of include/fx.h: each has this one definition, and the
// kernels cite it.
#ifndef FX_SCAN_QUERY_H_
#define FX_SCAN_QUERY_H_
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fx_device.h"

// ---- the query: a keypoint block as a call reads it (fx_device.h FxKpQuery)
// the block's kp_offset[max_scans + 1] and (x, y, z, elevation) rows, and the scans and rows that take part
struct KpView {
  const uint32_t *off;
  const float4 *kp;
  uint32_t S, rows;
};
__device__ __forceinline__ uint32_t query_scans(const FxKpQuery &K) { return min(min(K.n_scans, K.kp[0]), K.max_scans); }
__device__ __forceinline__ uint32_t query_rows(const FxKpQuery &K) { return min(min(K.kp[1], K.max_total), K.q_max_rows); }
__device__ __forceinline__ KpView query_view(const FxKpQuery &K) {
  KpView v;
  v.off = kp_block_offsets(K.kp);
  v.kp = kp_block_rows<float4>(K.kp, K.max_scans);
  v.S = query_scans(K), v.rows = query_rows(K);
  return v;
}
// the scan of row r < rows among S >= 1 scans; false: a non-row (no scan owns it)
__device__ __forceinline__ bool scan_of_row(const uint32_t *off, uint32_t S, uint32_t r, uint32_t &b) {
  uint32_t lo = 0u, hi = S;  // the largest b in [0, S] with kp_offset[b] <= r (kp_offset[0] = 0)
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (off[mid] <= r) lo = mid;
    else hi = mid - 1u;
  }
  b = lo;
  return lo < S && off[lo] <= r && r < off[lo + 1u];
}
// the rows [q_lo, q_hi) of scan b < S that take part
__device__ __forceinline__ void scan_rows(const KpView &V, uint32_t b, uint32_t &q_lo, uint32_t &q_hi) {
  q_lo = min(V.off[b], V.rows);
  q_hi = max(min(V.off[b + 1u], V.rows), q_lo);
}

// ---- which scans count
__host__ __device__ inline bool finite_pose(const fx_pose &P) {
  return isfinite(P.c) && isfinite(P.s) && isfinite(P.tx) && isfinite(P.ty) && isfinite(P.tz);
}
__device__ __forceinline__ const fx_localization *loc_of(const void *loc, uint32_t b) { return reinterpret_cast<const fx_localization *>(loc) + b; }
// a used scan: its localisation has every required flag and a finite pose
__device__ __forceinline__ bool scan_used(const void *loc, uint32_t b, uint32_t require_flags) {
  const fx_localization *L = loc_of(loc, b);
  return (L->flags & require_flags) == require_flags && finite_pose(L->pose);
}

// ---- which landmarks count
// the landmark t that id < N names: a merge since the localise is followed through the alias table; false: t is not a live landmark
// below N.  What the call asks of t's record stays with the call
__device__ __forceinline__ bool named_landmark(const int32_t *alias, uint32_t N, uint32_t id, uint32_t &t) {
  const int32_t a = alias[id];
  t = a >= 0 ? (uint32_t)a : id;
  return t < N && alias[t] == -1;
}
// the segment a landmark must have (FX_LOC_ANY_SEGMENT, FX_LOC_LAST_SEGMENT or a number): false, nothing is eligible (the last
// segment of a map of none); any: every segment passes
__device__ __forceinline__ bool wanted_segment(const void *header, uint32_t segment, uint32_t &seg, bool &any) {
  any = segment == FX_LOC_ANY_SEGMENT;
  seg = segment;
  if (segment == FX_LOC_LAST_SEGMENT) {
    const uint32_t n = reinterpret_cast<const fx_map_header *>(header)->segments;
    if (!n) return false;
    seg = n - 1u;
  }
  return true;
}
// what eligibility asks of the record of a live landmark (alias -1 is the caller's test), without and with the segment
__device__ __forceinline__ bool record_eligible(const fx_map_landmark &R, uint32_t min_obs) {
  return R.n_obs >= min_obs && isfinite(R.x) && isfinite(R.y) && isfinite(R.z);
}
__device__ __forceinline__ bool record_eligible(const fx_map_landmark &R, uint32_t min_obs, bool any_seg, uint32_t seg) {
  return record_eligible(R, min_obs) && (any_seg || R.segment == seg);
}

// ---- two workgroup idioms
// The slot of a true lane when the true lanes of a workgroup of NWAVE wavefronts are numbered in ascending thread order from
// `found`, and how many there are: ballot, a popcount a wavefront in s_wave[NWAVE] (LDS), a prefix over the wavefronts.  Every
// thread calls it; the caller keeps its loop and its cap, adds `all` to `found` and puts a barrier before the next call.
template <uint32_t NWAVE>
__device__ __forceinline__ void wg_ordered_slot(bool ok, uint32_t *s_wave, uint32_t found, uint32_t &slot, uint32_t &all) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(ok);
  if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t before = 0u;
  all = 0u;
#pragma unroll
  for (uint32_t w = 0; w < NWAVE; ++w) {
    const uint32_t n = s_wave[w];
    before += w < wave ? n : 0u;
    all += n;
  }
  slot = found + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
}
// a wavefront's count of a verdict added to a state word (every lane of the wavefront calls it)
__device__ __forceinline__ void count_wave(bool v, uint32_t *word) {
  const unsigned long long vote = __ballot(v);
  if ((threadIdx.x & 63u) == 0u && vote) atomicAdd(word, (uint32_t)__popcll(vote));
}
#endif
