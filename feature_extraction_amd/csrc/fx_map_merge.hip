// fx_map_merge.hip — spatial re-association in the persistent map: the fragments of one pole, which broken tracks left as several
// landmarks, folded into one (include/fx.h fx_map_merge).
//
// The result is defined over ALL pairs of landmarks; the grid below only finds the pairs that can pass the distance gate.  Every
// choice is a minimum over a total order (the proposal key, the 64-bit atomic minimum of the acceptance) or an integer count, so
// neither the order inside a bucket nor a hash collision nor the table's size can change a byte; every fp64 value is an ordered
// chain on one lane (the build's -ffp-contract=off).  Counts come from the map's header on the device; the grids are sized by the
// map's max_landmarks and exit early.
//
// The grid.  Cell edge E = md (1 + 2^-8), md = (double)merge_dist (exact: 24 + 9 bits); a coordinate's cell is floor(t),
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
// Launches, in stream order (FXMM_WG = 256 landmarks or buckets a workgroup; N = the header's n_landmarks):
//   k_mm_clear    the buckets' counts and the state words to 0
//   k_mm_mark     a thread a landmark: does it take part (alias -1, n_obs >= 1, x and y finite), its bucket, the bucket's count
//                 (32-bit atomic add); resets its proposal, its acceptance word and its links
//   k_mm_scan     a workgroup a block of buckets: the exclusive prefix of the counts inside the block (wg_scan2)
//   k_mm_top      one workgroup: the blocks' exclusive prefix (wg_scan2_blocks) and the number of landmarks in the grid
//   k_mm_scatter  a thread a landmark: its (x, y, last_scan, segment, id) into its bucket's range, the slot by an atomic on the count
//   k_mm_search   a thread a landmark h: the 3 x 3 cells' buckets and the far bucket; the best g by (greatest last_scan, smallest
//                 d2 as bits, lowest id); prop[h] = g and keep[g] = min(keep[g], first_scan[h] << 32 | h)
//   k_mm_link     a thread a landmark h: its proposal was kept iff the low word of keep[prop[h]] is h: pred[h], succ[g]
//   k_mm_fold     a thread a landmark: a root (a kept link out, none in) folds its chain, member by member, in chain order
//   k_mm_repoint  a thread an alias entry / carry entry: entries that point at a landmark absorbed by this call to its root; the
//                 landmarks that take part now are counted
//   k_mm_finish   one lane: the result
// A root writes its own record and sums, and the flags and alias of its members; it reads its members' sums, which nobody writes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_device.h"
#include "../../include/fx.h"

#define FXMM_WG 256
#define FXMM_NWAVE (FXMM_WG / 64)
#define FXMM_NONE 0xffffffffu

static_assert(sizeof(fx_map_landmark) == 48 && sizeof(FxMapMergeCand) == 32 && sizeof(fx_map_merge_result) == 16, "include/fx.h");

namespace {
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

// the best predecessor so far of one h: greatest last_scan, then smallest d2 (bits), then lowest id
struct Best {
  uint32_t last, id;
  unsigned long long d2;
  bool any;
};
__device__ __forceinline__ void walk(const FxMapMergeArgs &A, uint32_t b, uint32_t h, const fx_map_landmark &R, Best &best) {
  const uint32_t end = min(bucket_end(A, b), A.cap);
  for (uint32_t p = bucket_begin(A, b); p < end; ++p) {
    const FxMapMergeCand c = A.cand[p];
    if (c.id == h || c.segment != R.segment || c.last_scan >= R.first_scan || R.first_scan - c.last_scan > A.max_gap) continue;
    const double dx = c.x - R.x, dy = c.y - R.y;
    const double d2 = dx * dx + dy * dy;
    if (!(d2 <= A.md2)) continue;
    const unsigned long long k = (unsigned long long)__double_as_longlong(d2);
    const bool better = !best.any || c.last_scan > best.last || (c.last_scan == best.last && (k < best.d2 || (k == best.d2 && c.id < best.id)));
    if (better) best.any = true, best.last = c.last_scan, best.d2 = k, best.id = c.id;
  }
}
}  // namespace

extern "C" __global__ __launch_bounds__(FXMM_WG) void k_mm_clear(FxMapMergeArgs A) {
  const uint32_t b = blockIdx.x * FXMM_WG + threadIdx.x;
  if (b <= A.table) A.count[b] = 0u;
  if (b < FX_MAP_MERGE_ST_WORDS) A.st[b] = 0u;
}

extern "C" __global__ __launch_bounds__(FXMM_WG) void k_mm_mark(FxMapMergeArgs A) {
  const uint32_t i = blockIdx.x * FXMM_WG + threadIdx.x;
  if (i >= n_landmarks(A)) return;
  const fx_map_landmark R = records(A)[i];
  uint32_t b = FXMM_NONE;
  if (takes_part(A, i, R)) {
    const double tx = floor(R.x * A.inv_edge), ty = floor(R.y * A.inv_edge);
    const bool far = !(fabs(tx) < kFar && fabs(ty) < kFar);
    b = far ? A.table : bucket_of_cell((long long)tx, (long long)ty, A.table);
    atomicAdd(&A.count[b], 1u);
  }
  A.bucket[i] = b;
  A.prop[i] = -1, A.pred[i] = -1, A.succ[i] = -1;
  A.keep[i] = ~0ull;
}

extern "C" __global__ __launch_bounds__(FXMM_WG) void k_mm_scan(FxMapMergeArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXMM_NWAVE];
  const uint32_t b = blockIdx.x * FXMM_WG + threadIdx.x;
  uint32_t ea, eb, ta, tb;
  wg_scan2<FXMM_NWAVE>(b <= A.table ? A.count[b] : 0u, 0u, s_w, ea, eb, ta, tb);
  if (b <= A.table) A.start[b] = ea;
  if (threadIdx.x == 0u) A.bsum[blockIdx.x] = ta, A.bsum[n_blocks + blockIdx.x] = 0u;
}

extern "C" __global__ __launch_bounds__(FXMM_WG) void k_mm_top(FxMapMergeArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXMM_NWAVE];
  uint32_t total, unused;
  wg_scan2_blocks<FXMM_NWAVE>(A.bsum, n_blocks, s_w, total, unused);
  if (threadIdx.x == 0u) A.st[3] = total;
}

extern "C" __global__ __launch_bounds__(FXMM_WG) void k_mm_scatter(FxMapMergeArgs A) {
  const uint32_t i = blockIdx.x * FXMM_WG + threadIdx.x;
  if (i >= n_landmarks(A)) return;
  const uint32_t b = A.bucket[i];
  if (b == FXMM_NONE) return;
  const uint32_t slot = bucket_begin(A, b) + (atomicSub(&A.count[b], 1u) - 1u);  // any order inside the bucket
  if (slot >= A.cap) return;  // (cannot happen: the counts are of landmarks below cap)
  const fx_map_landmark R = records(A)[i];
  FxMapMergeCand c;
  c.x = R.x, c.y = R.y, c.last_scan = R.last_scan, c.segment = R.segment, c.id = i, c.pad_ = 0u;
  A.cand[slot] = c;
}

extern "C" __global__ __launch_bounds__(FXMM_WG) void k_mm_search(FxMapMergeArgs A) {
  const uint32_t h = blockIdx.x * FXMM_WG + threadIdx.x;
  bool proposes = false;
  if (h < n_landmarks(A) && A.bucket[h] != FXMM_NONE) {
    const fx_map_landmark R = records(A)[h];
    const double tx = floor(R.x * A.inv_edge), ty = floor(R.y * A.inv_edge);
    Best best;
    best.any = false, best.last = 0u, best.id = 0u, best.d2 = 0ull;
    if (fabs(tx) < kReach && fabs(ty) < kReach) {
      const long long cx = (long long)tx, cy = (long long)ty;
      for (int oy = -1; oy <= 1; ++oy)
        for (int ox = -1; ox <= 1; ++ox) walk(A, bucket_of_cell(cx + ox, cy + oy, A.table), h, R, best);  // (a bucket met twice changes nothing)
    }
    walk(A, A.table, h, R, best);
    if (best.any) {
      proposes = true;
      A.prop[h] = (int32_t)best.id;
      atomicMin(&A.keep[best.id], ((unsigned long long)R.first_scan << 32) | h);
    }
  }
  const unsigned long long vote = __ballot(proposes);
  if ((threadIdx.x & 63u) == 0u && vote) atomicAdd(&A.st[0], (uint32_t)__popcll(vote));
}

extern "C" __global__ __launch_bounds__(FXMM_WG) void k_mm_link(FxMapMergeArgs A) {
  const uint32_t h = blockIdx.x * FXMM_WG + threadIdx.x;
  bool kept = false;
  if (h < n_landmarks(A)) {
    const int32_t g = A.prop[h];
    if (g >= 0 && (uint32_t)(A.keep[g] & 0xffffffffull) == h) kept = true, A.pred[h] = g, A.succ[g] = (int32_t)h;
  }
  const unsigned long long vote = __ballot(kept);
  if ((threadIdx.x & 63u) == 0u && vote) atomicAdd(&A.st[1], (uint32_t)__popcll(vote));
}

extern "C" __global__ __launch_bounds__(FXMM_WG) void k_mm_fold(FxMapMergeArgs A) {
  const uint32_t r = blockIdx.x * FXMM_WG + threadIdx.x;
  const uint32_t N = n_landmarks(A);
  if (r >= N || A.succ[r] < 0 || A.pred[r] >= 0) return;
  fx_map_landmark *rec = reinterpret_cast<fx_map_landmark *>(A.records);
  fx_map_landmark R = rec[r];
  double *acc = A.acc + (size_t)r * FX_MAP_ACC;
  double sx = acc[0], sy = acc[1], sz = acc[2], dsx = acc[5], dsy = acc[6], q = acc[7];
  const double ax = acc[3], ay = acc[4];
  int32_t m = A.succ[r];
  for (uint32_t steps = 0u; m >= 0 && (uint32_t)m < N && steps < N; ++steps) {  // (a chain is simple: the bounds only keep the walk in memory)
    const fx_map_landmark M = rec[m];
    const double *b = A.acc + (size_t)m * FX_MAP_ACC;
    const double nm = (double)M.n_obs;
    const double ex = b[3] - ax, ey = b[4] - ay;
    sx += b[0], sy += b[1], sz += b[2];
    q += ((b[7] + 2.0 * (ex * b[5] + ey * b[6])) + nm * (ex * ex + ey * ey));
    dsx += (b[5] + nm * ex), dsy += (b[6] + nm * ey);
    R.n_obs += M.n_obs;
    R.last_scan = M.last_scan;
    R.flags |= FX_MAP_LM_MERGED | (M.flags & FX_MAP_LM_CONTINUED);
    rec[m].flags = M.flags | FX_MAP_LM_ABSORBED;
    A.alias[m] = (int32_t)r;
    m = A.succ[m];
  }
  map_record_from_sums(R, sx, sy, sz, dsx, dsy, q);
  acc[0] = sx, acc[1] = sy, acc[2] = sz, acc[5] = dsx, acc[6] = dsy, acc[7] = q;
  rec[r] = R;
}

extern "C" __global__ __launch_bounds__(FXMM_WG) void k_mm_repoint(FxMapMergeArgs A) {
  const uint32_t i = blockIdx.x * FXMM_WG + threadIdx.x;
  const uint32_t N = n_landmarks(A);
  const uint32_t n_carry = min(reinterpret_cast<const fx_map_header *>(A.header)->carry_rows, A.max_carry);
  // an entry points at a landmark that was live when the call began: now that one is live still, or its alias is its root.  Reading
  // through two levels gives the root whether or not the entry in between was rewritten already.
  bool live = false;
  if (i < N) {
    const int32_t a = A.alias[i];
    if (a >= 0 && (uint32_t)a < N) {
      const int32_t root = A.alias[a];
      if (root >= 0) A.alias[i] = root;
    }
    live = takes_part(A, i, records(A)[i]);  // (alias[i] == -1 is never rewritten)
  }
  if (i < n_carry) {
    const int32_t c = A.carry[i];
    if (c >= 0 && (uint32_t)c < N) {
      const int32_t a = A.alias[c];
      if (a >= 0 && (uint32_t)a < N) {
        const int32_t root = A.alias[a];
        A.carry[i] = root >= 0 ? root : a;
      }
    }
  }
  const unsigned long long vote = __ballot(live);
  if ((threadIdx.x & 63u) == 0u && vote) atomicAdd(&A.st[2], (uint32_t)__popcll(vote));
}

extern "C" __global__ __launch_bounds__(64) void k_mm_finish(FxMapMergeArgs A) {
  if (threadIdx.x || blockIdx.x || !A.result) return;
  A.result[0] = A.st[0], A.result[1] = A.st[1], A.result[2] = A.st[2], A.result[3] = 0u;
}

extern "C" hipError_t fxk_map_merge(hipStream_t s, const FxMapMergeArgs &A) {
  const dim3 wg(FXMM_WG);
  const uint32_t nb = (A.table + 1u + FXMM_WG - 1u) / FXMM_WG, nl = (A.cap + FXMM_WG - 1u) / FXMM_WG;
  const uint32_t nr = ((A.cap > A.max_carry ? A.cap : A.max_carry) + FXMM_WG - 1u) / FXMM_WG;
  hipLaunchKernelGGL(k_mm_clear, dim3(nb), wg, 0, s, A);
  hipLaunchKernelGGL(k_mm_mark, dim3(nl), wg, 0, s, A);
  hipLaunchKernelGGL(k_mm_scan, dim3(nb), wg, 0, s, A, nb);
  hipLaunchKernelGGL(k_mm_top, dim3(1), wg, 0, s, A, nb);
  hipLaunchKernelGGL(k_mm_scatter, dim3(nl), wg, 0, s, A);
  hipLaunchKernelGGL(k_mm_search, dim3(nl), wg, 0, s, A);
  hipLaunchKernelGGL(k_mm_link, dim3(nl), wg, 0, s, A);
  hipLaunchKernelGGL(k_mm_fold, dim3(nl), wg, 0, s, A);
  hipLaunchKernelGGL(k_mm_repoint, dim3(nr), wg, 0, s, A);
  hipLaunchKernelGGL(k_mm_finish, dim3(1), dim3(64), 0, s, A);
  return hipGetLastError();
}

// buckets of the table for a map of `cap` landmarks: the power of two at or above it (load at most 1)
extern "C" uint32_t fxk_map_merge_table(uint32_t cap) {
  uint32_t t = 1u;
  while (t < cap && t < 0x80000000u) t <<= 1;
  return t;
}

// bytes of the context's scratch for a map of `cap` landmarks, and the pointers carved out of it
extern "C" size_t fxk_map_merge_scratch(FxMapMergeArgs *A, uint8_t *base) {
  const size_t cap = A->cap, nbuckets = (size_t)A->table + 1u, nb = (nbuckets + FXMM_WG - 1u) / FXMM_WG;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += (bytes + 15u) & ~(size_t)15;
    return base ? base + at : (uint8_t *)nullptr;
  };
  A->cand = (FxMapMergeCand *)take(cap * sizeof(FxMapMergeCand));
  A->keep = (unsigned long long *)take(cap * 8u);
  A->st = (uint32_t *)take(FX_MAP_MERGE_ST_WORDS * 4u);
  A->count = (uint32_t *)take(nbuckets * 4u);
  A->start = (uint32_t *)take(nbuckets * 4u);
  A->bsum = (uint32_t *)take(2u * nb * 4u);
  A->bucket = (uint32_t *)take(cap * 4u);
  A->prop = (int32_t *)take(cap * 4u);
  A->pred = (int32_t *)take(cap * 4u);
  A->succ = (int32_t *)take(cap * 4u);
  return o;
}

extern "C" uint32_t fxk_map_merge_wg(void) { return FXMM_WG; }
