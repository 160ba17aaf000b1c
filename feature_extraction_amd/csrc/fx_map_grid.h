// fx_map_grid.h — the hashed grid over the map's live landmarks, which fx_map_merge (csrc/fx_map_merge.hip: a landmark looks for
// its predecessor), fx_map_localize (csrc/fx_map_localize.hip: a keypoint looks for its landmark), fx_map_join_segments
// (csrc/fx_map_join.hip: a landmark of one segment looks for its twin in another) and fx_map_close_loop (csrc/fx_map_loop.hip: a
// recent landmark looks for its old twin in the same segment) search; fx_map_relocalize and fx_map_find_loop walk two of them
// (csrc/fx_map_constellation.h).  The kernels that build it are csrc/fx_map_grid.hip's; what a search needs on the device is here.
//
// A grid is described by an FxMapMergeArgs (fx_device.h): the gate md2 = d d with d the call's distance widened to double, inv_edge
// = 1 / the cell edge, the table of `table` buckets (a power of two; bucket `table` is the far list) and the scratch arrays
// count / start / bsum / bucket / cand / st.  The grid holds the landmarks that take part in a merge (takes_part below): a search
// that wants fewer filters in its walk.  Neither the order inside a bucket nor a hash collision nor the table's size may change
// a byte of what a search returns: every search takes a minimum over a total order.
//
// The grid.  Cell edge E = md (1 + 2^-8), md = the call's distance widened to double (fx_map_merge: merge_dist, fx_map_localize:
// search_dist; E is exact: 24 + 9 bits); a coordinate's cell is floor(t),
// t = fl(x * fl(1 / E)).  Claim: two landmarks that pass the gate lie at most one cell apart in x and in y, as long as one of them
// has |floor(t)| < 2^39 ("near").  Proof, for x, u = 2^-53: the gate holds for computed values, fl(fl(dx dx) + fl(dy dy)) <=
// fl(md md) with dx = fl(px - qx); rounding is monotone and the second term is not negative, so fl(dx dx) <= fl(md md), so
// dx^2 (1 - u) <= md^2 (1 + u) (a dx^2 that underflows is far below any md^2, md >= 2^-149), and with |px - qx| <= |dx| / (1 - u):
// |px - qx| <= md (1 + 2^-50).  t carries two roundings: t = (x / E)(1 + d), |d| < 2^-51.  One of the two is near, so both have
// |x / E| < 2^39 + 3 < 2^40, and |tp - tq| <= |px - qx| / E + 2^-51 (|px| + |qx|) / E < (1 + 2^-50) / (1 + 2^-8) + 2^-10
// < 1 - 2^-8 + 2^-15 + 2^-10 < 1.  Two numbers less than 1 apart have floors at most 1 apart.  Landmarks that are not near
// (|floor(t)| >= 2^39 in x or y: beyond 10^11 m at the default gate) are kept out of the table in one list, the far bucket, which
// every search walks as well (it is empty in any real map); a far landmark below 2^41 also searches its 3 x 3 cells, which by the
// claim hold every near landmark within its gate, and beyond 2^41 no near landmark can be within it.
//
// The proof asks nothing of p and q but that they are doubles that pass the gate, so it covers a query point that is no landmark
// (fx_map_localize's world point of a keypoint row) as it covers a landmark: a query below 2^41 searches its 3 x 3 cells and the
// far bucket, one beyond searches the far bucket alone.  A query coordinate that is not finite passes no gate and finds nothing.
// For the same reason the items of a grid need not be landmarks: fx_map_discover (csrc/fx_map_discover.hip) builds a second grid
// over the world points of its free rows (FxMapMergeArgs::points, the same build launches) and walks it with grid_neighbourhood.
#ifndef FX_MAP_GRID_H_
#define FX_MAP_GRID_H_
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fx_device.h"

#define FXMM_WG 256
#define FXMM_NWAVE (FXMM_WG / 64)
#define FXMM_NONE 0xffffffffu

namespace fxg {
constexpr double kFar = 549755813888.0;    // 2^39: cells from here on go to the far bucket
constexpr double kReach = 2199023255552.0;  // 2^41: a far landmark below this still searches its 3 x 3 cells

__device__ __forceinline__ uint32_t n_landmarks(const FxMapMergeArgs &A) {
  return min(reinterpret_cast<const fx_map_header *>(A.header)->n_landmarks, A.cap);
}
__device__ __forceinline__ const fx_map_landmark *records(const FxMapMergeArgs &A) { return reinterpret_cast<const fx_map_landmark *>(A.records); }
__device__ __forceinline__ bool takes_part(const FxMapMergeArgs &A, uint32_t i, const fx_map_landmark &R) {
  return A.alias[i] == -1 && R.n_obs >= 1u && isfinite(R.x) && isfinite(R.y);
}
__device__ __forceinline__ uint32_t bucket_of_cell(long long cx, long long cy, uint32_t table) {
  unsigned long long h = (unsigned long long)cx * 0x9E3779B97F4A7C15ull + (unsigned long long)cy * 0xC2B2AE3D27D4EB4Full;
  h ^= h >> 32;
  h *= 0xD6E8FEB86659FD93ull;
  h ^= h >> 32;
  return (uint32_t)h & (table - 1u);
}
// first slot of bucket b (b <= table) in the sorted order; the slot behind the last bucket is the number of landmarks in the grid
__device__ __forceinline__ uint32_t bucket_begin(const FxMapMergeArgs &A, uint32_t b) { return A.bsum[b / FXMM_WG] + A.start[b]; }
__device__ __forceinline__ uint32_t bucket_end(const FxMapMergeArgs &A, uint32_t b) { return b == A.table ? A.st[3] : bucket_begin(A, b + 1u); }
// the 3 x 3 cells about the cell (tx, ty) = floor(coordinate * inv_edge) of a point, then the far bucket: visit(bucket) for each
// (a bucket met twice changes nothing: every search is a minimum)
template <typename Visit>
__device__ __forceinline__ void grid_neighbourhood(const FxMapMergeArgs &A, double tx, double ty, Visit visit) {
  if (fabs(tx) < kReach && fabs(ty) < kReach) {
    const long long cx = (long long)tx, cy = (long long)ty;
    for (int oy = -1; oy <= 1; ++oy)
      for (int ox = -1; ox <= 1; ++ox) visit(bucket_of_cell(cx + ox, cy + oy, A.table));
  }
  visit(A.table);
}
// the nearest eligible landmark so far of one query point: smallest d2 (bits), then lowest id
struct Near {
  unsigned long long d2;
  uint32_t id;
  bool any;
};
// One bucket of the nearest search of fx_map_localize's association clause (include/fx.h), which fx_map_join_segments and
// fx_map_close_loop share: the candidates of bucket b within the gate of (wx, wy) that the call accepts (accept(candidate):
// fx_map_localize "of the segment, or of any", the join "of segment dst", the loop "of the segment and OLD"), with at least min_obs
// observations and a finite z (the grid holds the merge's live set: the rest of the eligibility is here), by the lowest
// (d2 bits, id).  The record is read only for a candidate that would win.
template <typename Accept>
__device__ __forceinline__ void walk_nearest(const FxMapMergeArgs &G, uint32_t min_obs, uint32_t b, double wx, double wy, Accept accept,
                                             Near &best) {
  const uint32_t end = min(bucket_end(G, b), G.cap);
  for (uint32_t p = bucket_begin(G, b); p < end; ++p) {
    const FxMapMergeCand c = G.cand[p];
    const double dx = c.x - wx, dy = c.y - wy;
    const double d2 = dx * dx + dy * dy;
    const bool accepted = accept(c);  // (a plain value before the test: the candidate is read whole, not field by field down a branch)
    if (!(d2 <= G.md2) || !accepted || c.id >= G.cap) continue;
    const unsigned long long k = (unsigned long long)__double_as_longlong(d2);
    if (best.any && !(k < best.d2 || (k == best.d2 && c.id < best.id))) continue;
    const fx_map_landmark R = records(G)[c.id];
    if (R.n_obs < min_obs || !isfinite(R.z)) continue;
    best.any = true, best.d2 = k, best.id = c.id;
  }
}
}  // namespace fxg
#endif
