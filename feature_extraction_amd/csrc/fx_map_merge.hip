// fx_map_merge.hip — spatial re-association in the persistent map: the fragments of one pole, which broken tracks left as several
// landmarks, folded into one (include/fx.h fx_map_merge).
//
// The result is defined over ALL pairs of landmarks; the grid below only finds the pairs that can pass the distance gate.  Every
// choice is a minimum over a total order (the proposal key, the 64-bit atomic minimum of the acceptance) or an integer count, so
// neither the order inside a bucket nor a hash collision nor the table's size can change a byte; every fp64 value is an ordered
// chain on one lane (the build's -ffp-contract=off).  Counts come from the map's header on the device; the grids are sized by the
// map's max_landmarks and exit early.
//
// The grid is fx_map_grid.h's, where the proof of its one-cell margin stands; its first five launches are csrc/fx_map_grid.hip's
// (fxk_map_grid_build), which fx_map_localize shares.
// Launches, in stream order (FXMM_WG = 256 landmarks or buckets a workgroup; N = the header's n_landmarks):
//   (fxk_map_grid_build's five: clear, mark, scan, top, scatter; csrc/fx_map_grid.hip lists them)
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

#include "fx_map_grid.h"
#include "fx_scan_query.h"
#include "fx_launch.h"
#include "../../include/fx.h"

using namespace fxg;


static_assert(sizeof(fx_map_landmark) == 48 && sizeof(FxMapMergeCand) == 32 && sizeof(fx_map_merge_result) == 16, "include/fx.h");

namespace {
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

extern "C" __global__ __launch_bounds__(FXMM_WG) void k_mm_search(FxMapMergeArgs A) {
  const uint32_t h = blockIdx.x * FXMM_WG + threadIdx.x;
  bool proposes = false;
  if (h < n_landmarks(A) && A.bucket[h] != FXMM_NONE) {
    const fx_map_landmark R = records(A)[h];
    const double tx = floor(R.x * A.inv_edge), ty = floor(R.y * A.inv_edge);
    Best best;
    best.any = false, best.last = 0u, best.id = 0u, best.d2 = 0ull;
    grid_neighbourhood(A, tx, ty, [&](uint32_t b) { walk(A, b, h, R, best); });
    if (best.any) {
      proposes = true;
      A.prop[h] = (int32_t)best.id;
      atomicMin(&A.keep[best.id], ((unsigned long long)R.first_scan << 32) | h);
    }
  }
  count_wave(proposes, &A.st[0]);
}

extern "C" __global__ __launch_bounds__(FXMM_WG) void k_mm_link(FxMapMergeArgs A) {
  const uint32_t h = blockIdx.x * FXMM_WG + threadIdx.x;
  bool kept = false;
  if (h < n_landmarks(A)) {
    const int32_t g = A.prop[h];
    if (g >= 0 && (uint32_t)(A.keep[g] & 0xffffffffull) == h) kept = true, A.pred[h] = g, A.succ[g] = (int32_t)h;
  }
  count_wave(kept, &A.st[1]);
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
  count_wave(live, &A.st[2]);
}

extern "C" __global__ __launch_bounds__(64) void k_mm_finish(FxMapMergeArgs A) {
  if (threadIdx.x || blockIdx.x || !A.result) return;
  A.result[0] = A.st[0], A.result[1] = A.st[1], A.result[2] = A.st[2], A.result[3] = 0u;
}

extern "C" hipError_t fxk_map_merge(hipStream_t s, const FxMapMergeArgs &A) {
  const dim3 wg(FXMM_WG);
  const uint32_t nl = (A.cap + FXMM_WG - 1u) / FXMM_WG;
  const uint32_t nr = ((A.cap > A.max_carry ? A.cap : A.max_carry) + FXMM_WG - 1u) / FXMM_WG;
  (void)fxk_map_grid_build(s, A);  // k_mm_clear .. k_mm_scatter
  hipLaunchKernelGGL(k_mm_search, dim3(nl), wg, 0, s, A);
  hipLaunchKernelGGL(k_mm_link, dim3(nl), wg, 0, s, A);
  hipLaunchKernelGGL(k_mm_fold, dim3(nl), wg, 0, s, A);
  hipLaunchKernelGGL(k_mm_repoint, dim3(nr), wg, 0, s, A);
  hipLaunchKernelGGL(k_mm_finish, dim3(1), dim3(64), 0, s, A);
  return hipGetLastError();
}

// bytes of the context's scratch for a map of `cap` landmarks, and the pointers carved out of it
extern "C" size_t fxk_map_merge_scratch(FxMapMergeArgs *A, uint8_t *base) {
  const size_t cap = A->cap, nbuckets = (size_t)A->table + 1u, nb = (nbuckets + FXMM_WG - 1u) / FXMM_WG;
  FxCarve C{base, 0};
  A->cand = C.take<FxMapMergeCand>(cap);
  A->keep = C.take<unsigned long long>(cap);
  A->st = C.take<uint32_t>(FX_MAP_MERGE_ST_WORDS);
  A->count = C.take<uint32_t>(nbuckets);
  A->start = C.take<uint32_t>(nbuckets);
  A->bsum = C.take<uint32_t>(2u * nb);
  A->bucket = C.take<uint32_t>(cap);
  A->prop = C.take<int32_t>(cap);
  A->pred = C.take<int32_t>(cap);
  A->succ = C.take<int32_t>(cap);
  return C.o;
}

extern "C" uint32_t fxk_map_merge_wg(void) { return FXMM_WG; }
