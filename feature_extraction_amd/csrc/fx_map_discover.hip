// fx_map_discover.hip — the rows of localised scans that no landmark explains, yet fall on one spot of the map frame scan after
// scan, made landmarks (include/fx.h fx_map_discover): the third of fx_map_observe / fx_map_retire.
//
// The definition is all-pairs: a row against every live landmark of the segment, a free row against every free row.  Two hashed grids
// (fx_map_grid.h) only find the few that can pass a gate: G over the map's landmarks with the gate known_dist, F over the free rows'
// world points with the gate join_dist (the same build launches, reading points from an array).  Every decision is an integer or a
// minimum over a total order: an existence (known, leader), the lowest (d2 bits, id) (attachment, the scan's observation), 32-bit
// integer atomics (counts: sums, which commute), exclusive prefixes (fx_device.h's wg_scan2 / wg_scan2_blocks).  The order inside
// a bucket never shows: the fold takes the rows of its landmark by "the lowest free row above the last one", so a bucket met twice
// changes nothing either.  Every fp64 sum is an ordered chain on one lane (the build's -ffp-contract=off): the same bytes from run
// to run and with any number of contexts in flight.  The map is read as it is when the call starts: G is built first, the only
// launch that writes records, k_disc_fold, writes ids at or above n_needed, which no reader reads, and the header changes last.
//
// A free row is known by its number j among the free rows in ascending row (so ascending j is ascending row).
// Launches, in stream order (FXD_WG = 256 rows or free rows a workgroup), after fxk_map_grid_build's five over the map:
//   (a memset: the state words and the leaders' supports to 0)
//   k_disc_classify  a thread a row r < q_max_rows: the row's scan, whether the scan is used, unmatched (finite, no landmark named,
//                    a finite world point), known (a walk of G's 3 x 3 cells and far bucket: a live landmark of the segment within
//                    known_dist), else free; the free rows' exclusive prefix within the block; new_id_of_row[r] = -1
//   k_disc_top       one workgroup: the exclusive prefix of the blocks' free rows, their number, the used scans, first_id, refused
//   k_disc_stage     a thread a row: a free row's number j, its world (x, y) staged at pts[j], its (row, scan) at src[j]
//   (fxk_map_grid_build's five over pts: the grid F)
//   k_disc_lead      a thread a free row: a leader iff no free row below it lies within join_dist (a walk of F)
//   k_disc_attach    a thread a free row: the leader within join_dist of lowest (d2 bits, j), or none: an orphan
//   k_disc_keep      a thread an attached row: kept iff no row of its own scan on the same leader is lower in (d2 bits, row);
//                    the leader's support (a 32-bit atomic add)
//   k_disc_confirm   a thread a free row: a leader of min_obs kept rows is confirmed; their exclusive prefix within the block
//   k_disc_top2      one workgroup: the exclusive prefix of the blocks' confirmed leaders, their number
//   k_disc_fold      a thread a confirmed leader: its id; stored, it takes its kept rows in ascending row and adds them to fresh
//                    sums, one chain, writes new_id_of_row for each and the record and the sums
//   k_disc_finish    one lane: the result and the header
// A dry run (FX_DISC_DRY_RUN) runs all of it and skips the stores into the map.  A refused call (the segment resolves to nothing)
// runs all of it with no row unmatched.  No LDS beyond the scans' [2][4] words.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_map_grid.h"
#include "fx_scan_query.h"
#include "fx_launch.h"
#include "../../include/fx.h"

using namespace fxg;

#define FXD_WG 256
#define FXD_NWAVE (FXD_WG / 64)
// the state words (fx_device.h FX_MAP_DISCOVER_ST_WORDS): fx_map_discover_result's, then the confirmed leaders
enum { D_SCANS, D_UNMATCHED, D_KNOWN, D_FREE, D_LEADERS, D_ORPHANS, D_DUP, D_WEAK, D_ADDED, D_LOST, D_CREATED, D_NOT_STORED, D_FIRST, D_REFUSED, D_CONF };

static_assert(sizeof(fx_localization) == 112 && sizeof(fx_map_discover_options) == 32 && sizeof(fx_map_discover_result) == 64 &&
                  sizeof(fx_map_landmark) == 48 && sizeof(fx_map_header) == 88 && FX_MAP_DISCOVER_ST_WORDS * 4 == sizeof(fx_map_discover_result) &&
                  FXD_WG == FXMM_WG,
              "include/fx.h");

namespace {
__device__ __forceinline__ const fx_map_header *header_of(const FxMapDiscoverArgs &A) { return reinterpret_cast<const fx_map_header *>(A.header); }
// the segment the call works in; false: the call is refused (it resolves to nothing, or the map has no such segment)
__device__ __forceinline__ bool disc_segment(const FxMapDiscoverArgs &A, uint32_t &seg) {
  bool any;
  return wanted_segment(A.header, A.segment, seg, any) && !any && seg < header_of(A)->segments;
}
// the free rows (after k_disc_top)
__device__ __forceinline__ uint32_t free_rows(const FxMapDiscoverArgs &A) { return min(A.st[D_FREE], A.K.q_max_rows); }
// the candidates of bucket b of grid G: visit(candidate, d2 of it from (x, y)) for each within the gate
template <typename Visit>
__device__ __forceinline__ void walk_within(const FxMapMergeArgs &G, uint32_t b, double x, double y, Visit visit) {
  const uint32_t end = min(bucket_end(G, b), G.cap);
  for (uint32_t p = bucket_begin(G, b); p < end; ++p) {
    const FxMapMergeCand c = G.cand[p];
    const double dx = c.x - x, dy = c.y - y;
    const double d2 = dx * dx + dy * dy;
    if (d2 <= G.md2 && c.id < G.cap) visit(c, d2);
  }
}
__device__ __forceinline__ double cell(const FxMapMergeArgs &G, double t) { return floor(t * G.inv_edge); }
}  // namespace

extern "C" __global__ __launch_bounds__(FXD_WG) void k_disc_classify(FxMapDiscoverArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXD_NWAVE];
  const uint32_t r = blockIdx.x * FXD_WG + threadIdx.x;
  const KpView V = query_view(A.K);
  uint32_t seg, b;
  const bool go = disc_segment(A, seg);  // (uniform)
  bool unmatched = false, known = false;
  if (go && r < V.rows && V.S && scan_of_row(V.off, V.S, r, b) && scan_used(A.loc, b, A.require_flags)) {
    const float4 k = V.kp[r];
    if (finite3(k) && A.map_id_of_row[r] < 0) {
      double wx, wy, wz;
      world_point(loc_of(A.loc, b)->pose, k, wx, wy, wz);
      if (isfinite(wx) && isfinite(wy) && isfinite(wz)) {
        unmatched = true;
        grid_neighbourhood(A.G, cell(A.G, wx), cell(A.G, wy), [&](uint32_t bk) {
          if (!known) walk_within(A.G, bk, wx, wy, [&](const FxMapMergeCand &c, double) { known = known || c.segment == seg; });
        });
      }
    }
  }
  const bool is_free = unmatched && !known;
  uint32_t ea, eb, ta, tb;
  wg_scan2<FXD_NWAVE>(is_free ? 1u : 0u, 0u, s_w, ea, eb, ta, tb);
  if (r < A.K.q_max_rows) {
    A.fidx[r] = is_free ? (int32_t)ea : -1;
    if (A.new_id) A.new_id[r] = -1;
  }
  if (threadIdx.x == 0u) A.bsum_f[blockIdx.x] = ta, A.bsum_f[n_blocks + blockIdx.x] = 0u;
  count_wave(unmatched, &A.st[D_UNMATCHED]);
  count_wave(known, &A.st[D_KNOWN]);
}

extern "C" __global__ __launch_bounds__(FXD_WG) void k_disc_top(FxMapDiscoverArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXD_NWAVE];
  uint32_t n_free, unused, seg;
  wg_scan2_blocks<FXD_NWAVE>(A.bsum_f, n_blocks, s_w, n_free, unused);
  const bool go = disc_segment(A, seg);
  const uint32_t S = go ? query_scans(A.K) : 0u;
  uint32_t used = 0u;
  for (uint32_t b = threadIdx.x; b < S; b += FXD_WG) used += scan_used(A.loc, b, A.require_flags) ? 1u : 0u;
  uint32_t ea, eb, ta, tb;
  wg_scan2<FXD_NWAVE>(used, 0u, s_w, ea, eb, ta, tb);
  if (threadIdx.x == 0u) A.st[D_SCANS] = ta, A.st[D_FREE] = n_free, A.st[D_FIRST] = header_of(A)->n_needed, A.st[D_REFUSED] = go ? 0u : 1u;
}

extern "C" __global__ __launch_bounds__(FXD_WG) void k_disc_stage(FxMapDiscoverArgs A) {
  const uint32_t r = blockIdx.x * FXD_WG + threadIdx.x;
  if (r >= A.K.q_max_rows) return;
  const int32_t f = A.fidx[r];
  if (f < 0) return;
  const uint32_t j = A.bsum_f[r / FXD_WG] + (uint32_t)f;
  if (j >= A.K.q_max_rows) return;  // (never: the free rows are rows)
  const KpView V = query_view(A.K);
  uint32_t b = 0u;
  (void)scan_of_row(V.off, V.S, r, b);  // (a free row has a scan)
  double wx, wy, wz;
  world_point(loc_of(A.loc, b)->pose, V.kp[r], wx, wy, wz);
  A.pts[j] = make_double2(wx, wy);
  A.src[j] = make_uint2(r, b);
  A.fidx[r] = (int32_t)j;
}

extern "C" __global__ __launch_bounds__(FXD_WG) void k_disc_lead(FxMapDiscoverArgs A) {
  const uint32_t j = blockIdx.x * FXD_WG + threadIdx.x;
  const bool mine = j < free_rows(A);
  bool lead = mine;
  if (mine) {
    const double2 p = A.pts[j];
    grid_neighbourhood(A.F, cell(A.F, p.x), cell(A.F, p.y), [&](uint32_t bk) {
      if (lead) walk_within(A.F, bk, p.x, p.y, [&](const FxMapMergeCand &c, double) { lead = lead && !(c.id < j); });
    });
    A.lead[j] = lead ? 1u : 0u;
  }
  count_wave(lead, &A.st[D_LEADERS]);
}

extern "C" __global__ __launch_bounds__(FXD_WG) void k_disc_attach(FxMapDiscoverArgs A) {
  const uint32_t j = blockIdx.x * FXD_WG + threadIdx.x;
  const bool mine = j < free_rows(A);
  uint32_t best = FX_DISC_NONE;
  unsigned long long best_d2 = ~0ull;
  if (mine) {
    const double2 p = A.pts[j];
    grid_neighbourhood(A.F, cell(A.F, p.x), cell(A.F, p.y), [&](uint32_t bk) {
      walk_within(A.F, bk, p.x, p.y, [&](const FxMapMergeCand &c, double d2) {
        const unsigned long long k = (unsigned long long)__double_as_longlong(d2);
        if ((k < best_d2 || (k == best_d2 && c.id < best)) && A.lead[c.id]) best_d2 = k, best = c.id;
      });
    });
    A.att[j] = best;
    A.ad2[j] = best_d2;
  }
  count_wave(mine && best == FX_DISC_NONE, &A.st[D_ORPHANS]);
}

extern "C" __global__ __launch_bounds__(FXD_WG) void k_disc_keep(FxMapDiscoverArgs A) {
  const uint32_t j = blockIdx.x * FXD_WG + threadIdx.x;
  const bool mine = j < free_rows(A);
  const uint32_t l = mine ? A.att[j] : FX_DISC_NONE;
  const bool attached = l != FX_DISC_NONE;
  bool keep = attached;
  if (attached) {
    const KpView V = query_view(A.K);
    const uint2 me = A.src[j];
    const unsigned long long k = A.ad2[j];
    uint32_t q_lo, q_hi;
    scan_rows(V, me.y, q_lo, q_hi);
    for (uint32_t r = q_lo; r < q_hi; ++r) {  // the scan's other rows on the same leader
      const int32_t o = A.fidx[r];
      if (o < 0 || (uint32_t)o == j || A.att[o] != l) continue;
      const unsigned long long ko = A.ad2[o];
      keep = keep && !(ko < k || (ko == k && r < me.x));
    }
    A.kept[j] = keep ? 1u : 0u;
    if (keep) atomicAdd(&A.sup[l], 1u);
  }
  count_wave(attached && !keep, &A.st[D_DUP]);
}

extern "C" __global__ __launch_bounds__(FXD_WG) void k_disc_confirm(FxMapDiscoverArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXD_NWAVE];
  const uint32_t j = blockIdx.x * FXD_WG + threadIdx.x;
  const bool lead = j < free_rows(A) && A.lead[j] != 0u;
  const uint32_t k = lead ? A.sup[j] : 0u;
  const bool conf = lead && k >= A.min_obs;
  uint32_t ea, eb, ta, tb;
  wg_scan2<FXD_NWAVE>(conf ? 1u : 0u, conf ? 0u : k, s_w, ea, eb, ta, tb);
  if (j < A.K.q_max_rows) A.rank_c[j] = conf ? ea : FX_DISC_NONE;
  if (threadIdx.x == 0u) {
    A.bsum_c[blockIdx.x] = ta, A.bsum_c[n_blocks + blockIdx.x] = 0u;
    if (tb) atomicAdd(&A.st[D_WEAK], tb);  // the kept rows of the block's unconfirmed leaders
  }
}

extern "C" __global__ __launch_bounds__(FXD_WG) void k_disc_top2(FxMapDiscoverArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXD_NWAVE];
  uint32_t n_conf, unused;
  wg_scan2_blocks<FXD_NWAVE>(A.bsum_c, n_blocks, s_w, n_conf, unused);
  if (threadIdx.x == 0u) A.st[D_CONF] = n_conf;
}

extern "C" __global__ __launch_bounds__(FXD_WG) void k_disc_fold(FxMapDiscoverArgs A) {
  const uint32_t j = blockIdx.x * FXD_WG + threadIdx.x;
  if (j >= free_rows(A)) return;
  const uint32_t rank = A.rank_c[j];
  if (rank == FX_DISC_NONE) return;
  const uint32_t k = A.sup[j];
  const unsigned long long id = (unsigned long long)A.st[D_FIRST] + A.bsum_c[j / FXD_WG] + rank;
  if (id >= A.G.cap) {  // fx_map_update's rule: counted, not stored; its rows keep their -1
    atomicAdd(&A.st[D_LOST], k);
    atomicAdd(&A.st[D_NOT_STORED], 1u);
    return;
  }
  const float4 *kp = kp_block_rows<float4>(A.K.kp, A.K.max_scans);
  const double2 p = A.pts[j];
  const double tx = cell(A.F, p.x), ty = cell(A.F, p.y);
  double sx = 0.0, sy = 0.0, sz = 0.0, dsx = 0.0, dsy = 0.0, q = 0.0;
  uint32_t n = 0u, at = j;  // the leader is its own first kept row: no free row below it lies within join_dist of it
  while (at != FX_DISC_NONE && n < k) {
    const uint2 s = A.src[at];
    double wx, wy, wz;
    world_point(loc_of(A.loc, s.y)->pose, kp[s.x], wx, wy, wz);
    const double dx = wx - p.x, dy = wy - p.y;
    sx += wx, sy += wy, sz += wz;
    dsx += dx, dsy += dy;
    q += (dx * dx + dy * dy);
    if (A.new_id) A.new_id[s.x] = (int32_t)id;
    ++n;
    uint32_t next = FX_DISC_NONE;  // the lowest kept row of this leader above `at`: the rows within join_dist of the leader hold it
    grid_neighbourhood(A.F, tx, ty, [&](uint32_t bk) {
      walk_within(A.F, bk, p.x, p.y, [&](const FxMapMergeCand &c, double) {
        if (c.id > at && c.id < next && A.att[c.id] == j && A.kept[c.id]) next = c.id;
      });
    });
    at = next;
  }
  if (A.mode == FX_DISC_APPLY) {
    const fx_map_header *H = header_of(A);
    fx_map_landmark R;
    R.n_obs = n;
    map_record_from_sums(R, sx, sy, sz, dsx, dsy, q);
    R.first_scan = R.last_scan = H->scans ? H->scans - 1u : 0u;
    uint32_t seg = 0u;
    (void)disc_segment(A, seg);
    R.segment = seg, R.flags = FX_MAP_LM_DISCOVERED;
    reinterpret_cast<fx_map_landmark *>(A.records)[id] = R;
    double *acc = A.acc + (size_t)id * FX_MAP_ACC;
    acc[0] = sx, acc[1] = sy, acc[2] = sz, acc[3] = p.x, acc[4] = p.y, acc[5] = dsx, acc[6] = dsy, acc[7] = q;
  }
  atomicAdd(&A.st[D_ADDED], n);
  atomicAdd(&A.st[D_CREATED], 1u);
}

extern "C" __global__ __launch_bounds__(64) void k_disc_finish(FxMapDiscoverArgs A) {
  if (threadIdx.x || blockIdx.x) return;
  if (A.result) {
    for (uint32_t i = 0; i <= D_REFUSED; ++i) A.result[i] = A.st[i];
    A.result[14] = A.result[15] = 0u;
  }
  if (A.mode == FX_DISC_APPLY && !A.st[D_REFUSED]) {
    fx_map_header *H = reinterpret_cast<fx_map_header *>(A.header);
    H->n_needed += A.st[D_CONF];
    H->n_landmarks = min(H->n_needed, A.G.cap);
    H->n_obs += A.st[D_ADDED];
    if (A.st[D_NOT_STORED]) H->flags |= FX_MAP_FULL;
  }
}

extern "C" hipError_t fxk_map_discover(hipStream_t s, const FxMapDiscoverArgs &A) {
  const dim3 wg(FXD_WG);
  const uint32_t nr = (A.K.q_max_rows + FXD_WG - 1u) / FXD_WG;
  (void)fxk_map_grid_build(s, A.G);
  // the state words and the supports behind them are one region of the scratch (fxk_map_discover_scratch)
  const hipError_t e = hipMemsetAsync(A.st, 0, (FX_MAP_DISCOVER_ST_WORDS + (size_t)A.K.q_max_rows) * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  if (nr) hipLaunchKernelGGL(k_disc_classify, dim3(nr), wg, 0, s, A, nr);
  hipLaunchKernelGGL(k_disc_top, dim3(1), wg, 0, s, A, nr);
  if (nr) {
    hipLaunchKernelGGL(k_disc_stage, dim3(nr), wg, 0, s, A);
    (void)fxk_map_grid_build(s, A.F);
    hipLaunchKernelGGL(k_disc_lead, dim3(nr), wg, 0, s, A);
    hipLaunchKernelGGL(k_disc_attach, dim3(nr), wg, 0, s, A);
    hipLaunchKernelGGL(k_disc_keep, dim3(nr), wg, 0, s, A);
    hipLaunchKernelGGL(k_disc_confirm, dim3(nr), wg, 0, s, A, nr);
    hipLaunchKernelGGL(k_disc_top2, dim3(1), wg, 0, s, A, nr);
    hipLaunchKernelGGL(k_disc_fold, dim3(nr), wg, 0, s, A);
  }
  hipLaunchKernelGGL(k_disc_finish, dim3(1), dim3(64), 0, s, A);
  return hipGetLastError();
}

// bytes of the context's scratch for a map of A->G.cap landmarks and q_max_rows rows, and the pointers carved out of it: the
// landmark grid's part of the merge's layout first (the calls share the buffer: they are ordered on one stream), then the free
// rows' grid (A->F.cap = q_max_rows items, A->F.table buckets), then this call's arrays
extern "C" size_t fxk_map_discover_scratch(FxMapDiscoverArgs *A, uint8_t *base) {
  FxCarve C{base, fxk_map_merge_scratch(&A->G, base)};
  A->G.prop = A->G.pred = A->G.succ = nullptr, A->G.keep = nullptr;  // (the grid's mark leaves the merge's words alone)
  const size_t rows = A->K.q_max_rows, nb = (rows + FXD_WG - 1u) / FXD_WG;
  const size_t nbuckets = (size_t)A->F.table + 1u, nbb = (nbuckets + FXMM_WG - 1u) / FXMM_WG;
  A->F.cand = C.take<FxMapMergeCand>(rows);
  A->F.st = C.take<uint32_t>(FX_MAP_MERGE_ST_WORDS);
  A->F.count = C.take<uint32_t>(nbuckets);
  A->F.start = C.take<uint32_t>(nbuckets);
  A->F.bsum = C.take<uint32_t>(2u * nbb);
  A->F.bucket = C.take<uint32_t>(rows);
  A->st = C.take<uint32_t>(FX_MAP_DISCOVER_ST_WORDS + rows);
  A->sup = base ? A->st + FX_MAP_DISCOVER_ST_WORDS : (uint32_t *)nullptr;
  A->fidx = C.take<int32_t>(rows);
  A->bsum_f = C.take<uint32_t>(2u * nb);
  A->bsum_c = C.take<uint32_t>(2u * nb);
  A->pts = C.take<double2>(rows);
  A->src = C.take<uint2>(rows);
  A->lead = C.take<uint32_t>(rows);
  A->att = C.take<uint32_t>(rows);
  A->ad2 = C.take<unsigned long long>(rows);
  A->kept = C.take<uint32_t>(rows);
  A->rank_c = C.take<uint32_t>(rows);
  A->F.points = A->pts;
  A->F.n_points = base ? A->st + D_FREE : (const uint32_t *)nullptr;
  return C.o;
}
