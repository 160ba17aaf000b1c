// fx_map_grid.hip — building the hashed grid over the map's live landmarks (fx_map_grid.h) for fx_map_merge and fx_map_localize.
// The same launches build a grid over points that are no landmarks (A.points given: fx_map_discover's free rows): grid_item is the
// one place that knows which of the two an item is.
//
// Launches, in stream order (FXMM_WG = 256 landmarks or buckets a workgroup; N = the header's n_landmarks, or *A.n_points):
//   k_mm_clear    the buckets' counts and the state words to 0
//   k_mm_mark     a thread a landmark: does it take part (alias -1, n_obs >= 1, x and y finite), its bucket, the bucket's count
//                 (32-bit atomic add); when the caller is the merge (A.prop given) it resets the landmark's proposal, its
//                 acceptance word and its links
//   k_mm_scan     a workgroup a block of buckets: the exclusive prefix of the counts inside the block (wg_scan2)
//   k_mm_top      one workgroup: the blocks' exclusive prefix (wg_scan2_blocks) and the number of landmarks in the grid
//   k_mm_scatter  a thread a landmark: its (x, y, last_scan, segment, id) into its bucket's range, the slot by an atomic on the count
// The slots inside a bucket are in completion order: no search may depend on it (fx_map_grid.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_launch.h"
#include "fx_map_grid.h"

using namespace fxg;

static_assert(sizeof(fx_map_landmark) == 48 && sizeof(FxMapMergeCand) == 32, "include/fx.h");

namespace {
// the items the grid is built over: the map's landmarks, or the points of A.points
__device__ __forceinline__ uint32_t grid_items(const FxMapMergeArgs &A) { return A.points ? min(*A.n_points, A.cap) : n_landmarks(A); }
// item i < grid_items as the search reads it; false: it takes no part.  A point takes part always and carries no scan and no segment
__device__ __forceinline__ bool grid_item(const FxMapMergeArgs &A, uint32_t i, FxMapMergeCand &c) {
  c.id = i, c.pad_ = 0u;
  if (A.points) {
    const double2 p = A.points[i];
    c.x = p.x, c.y = p.y, c.last_scan = 0u, c.segment = 0u;
    return true;
  }
  const fx_map_landmark R = records(A)[i];
  c.x = R.x, c.y = R.y, c.last_scan = R.last_scan, c.segment = R.segment;
  return takes_part(A, i, R);
}
}  // namespace

extern "C" __global__ __launch_bounds__(FXMM_WG) void k_mm_clear(FxMapMergeArgs A) {
  const uint32_t b = blockIdx.x * FXMM_WG + threadIdx.x;
  if (b <= A.table) A.count[b] = 0u;
  if (b < FX_MAP_MERGE_ST_WORDS) A.st[b] = 0u;
}

extern "C" __global__ __launch_bounds__(FXMM_WG) void k_mm_mark(FxMapMergeArgs A) {
  const uint32_t i = blockIdx.x * FXMM_WG + threadIdx.x;
  if (i >= grid_items(A)) return;
  FxMapMergeCand c;
  uint32_t b = FXMM_NONE;
  if (grid_item(A, i, c)) {
    const double tx = floor(c.x * A.inv_edge), ty = floor(c.y * A.inv_edge);
    const bool far = !(fabs(tx) < kFar && fabs(ty) < kFar);
    b = far ? A.table : bucket_of_cell((long long)tx, (long long)ty, A.table);
    atomicAdd(&A.count[b], 1u);
  }
  A.bucket[i] = b;
  if (A.prop) {
    A.prop[i] = -1, A.pred[i] = -1, A.succ[i] = -1;
    A.keep[i] = ~0ull;
  }
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
  if (i >= grid_items(A)) return;
  const uint32_t b = A.bucket[i];
  if (b == FXMM_NONE) return;
  const uint32_t slot = bucket_begin(A, b) + (atomicSub(&A.count[b], 1u) - 1u);  // any order inside the bucket
  if (slot >= A.cap) return;  // (cannot happen: the counts are of landmarks below cap)
  FxMapMergeCand c;
  (void)grid_item(A, i, c);
  A.cand[slot] = c;
}

extern "C" hipError_t fxk_map_grid_build(hipStream_t s, const FxMapMergeArgs &A) {
  const dim3 wg(FXMM_WG);
  const uint32_t nb = (A.table + 1u + FXMM_WG - 1u) / FXMM_WG, nl = (A.cap + FXMM_WG - 1u) / FXMM_WG;
  hipLaunchKernelGGL(k_mm_clear, dim3(nb), wg, 0, s, A);
  hipLaunchKernelGGL(k_mm_mark, dim3(nl), wg, 0, s, A);
  hipLaunchKernelGGL(k_mm_scan, dim3(nb), wg, 0, s, A, nb);
  hipLaunchKernelGGL(k_mm_top, dim3(1), wg, 0, s, A, nb);
  hipLaunchKernelGGL(k_mm_scatter, dim3(nl), wg, 0, s, A);
  return hipGetLastError();
}

// buckets of the table for a map of `cap` landmarks: the power of two at or above it (load at most 1)
extern "C" uint32_t fxk_map_merge_table(uint32_t cap) {
  uint32_t t = 1u;
  while (t < cap && t < 0x80000000u) t <<= 1;
  return t;
}
