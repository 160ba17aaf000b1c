// fx_map_expect.hip — per landmark, how many localised scans should have seen it and how many did (include/fx.h fx_map_expect):
// the negative evidence fx_map_retire decides on.
//
// The counts are defined over ALL (used scan, eligible landmark) pairs; the grid (fx_map_grid.h: fx_map_merge's, with max_range for
// its gate) only finds the landmarks that can be in range of a scan's sensor.  Every decision is a comparison of correctly rounded
// fp64 values (the build's -ffp-contract=off; every float is widened first), every count a 32-bit integer sum (integer atomics:
// sums commute): the same bytes from run to run and with any number of contexts in flight.  The map is only read.
//
// A pair must be counted ONCE, so unlike a nearest search (a minimum, which a bucket met twice cannot change) the walk here visits
// every bucket once: the up to nine buckets of the 3 x 3 cells are deduplicated before the walk (two cells may hash to one bucket),
// and the far bucket is disjoint from the table.  A landmark lies in exactly one bucket; a landmark of another cell that hashes into a
// walked bucket is tested like any other: the range test is exact, so it changes nothing.
//
// Launches, in stream order, after fxk_map_grid_build's five (the merge's live set: alias -1, n_obs >= 1, finite x and y):
//   (a memset: this call's counts of both kinds and the state words to 0)
//   k_exp_name   a thread a row r < q_max_rows: the row's scan, whether the scan is used, the proposal, its target through the alias
//                table (fx_scan_query.h: scan_of_row, scan_used, named_landmark), eligible (record_eligible) or stale.  Writes
//                tgt[r]: the landmark named, -1: a finite row of a used scan that names none (it can still shadow), -2: anything
//                else
//   k_exp_scan   one workgroup of FXE_WG = 256 lanes a scan: the scan's rows staged in LDS in chunks of FXE_CHUNK = 512 (x, y
//                widened, k2, the target: 28 B a row, 14 KB); the landmarks of the walked buckets flattened over the lanes, 256 a
//                round; a lane tests its landmark's eligibility on the record, the range and the box, then walks the staged rows
//                for Seen and Shadowed (all lanes read the same row: an LDS broadcast).  A scan of one chunk is staged once; a
//                longer one is staged again for every round of landmarks.  Counts: 32-bit atomics a landmark, a wavefront's sum
//                a state word
//   k_exp_emit   a thread a landmark i < max_landmarks: WRITE stores this call's counts, ADD adds the non-zero ones; one lane
//                writes the result
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_map_grid.h"
#include "fx_scan_query.h"
#include "fx_launch.h"
#include "../../include/fx.h"

using namespace fxg;

#define FXE_WG 256
#define FXE_CHUNK 512u
#define FXE_BUCKETS 10u  // 3 x 3 cells and the far bucket

static_assert(sizeof(fx_localization) == 112 && sizeof(fx_map_expect_options) == 48 && sizeof(fx_map_expect_result) == 32 &&
                  sizeof(fx_map_landmark) == 48 && sizeof(fx_map_header) == 88 && FX_MAP_EXPECT_ST_WORDS * 4 == sizeof(fx_map_expect_result),
              "include/fx.h");


namespace {
// a wavefront's sum of v into a state word
__device__ __forceinline__ void add_wave(uint32_t v, uint32_t *word) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += (uint32_t)__shfl_down((int)v, o, 64);
  if ((threadIdx.x & 63u) == 0u && v) atomicAdd(word, v);
}
}  // namespace

extern "C" __global__ __launch_bounds__(FXE_WG) void k_exp_name(FxMapExpectArgs A) {
  const uint32_t r = blockIdx.x * FXE_WG + threadIdx.x;
  const KpView V = query_view(A.K);
  const uint32_t N = n_landmarks(A.G);
  int32_t t = -2;
  bool stale = false;
  uint32_t b;
  if (r < V.rows && V.S && scan_of_row(V.off, V.S, r, b) && scan_used(A.loc, b, A.require_flags) && finite3(V.kp[r])) {
    t = -1;
    const int32_t id = A.map_id_of_row[r];
    if (id >= 0 && (uint32_t)id < N) {
      uint32_t g, seg;
      bool any_seg;
      bool ok = named_landmark(A.G.alias, N, (uint32_t)id, g) && wanted_segment(A.G.header, A.segment, seg, any_seg);
      if (ok) ok = record_eligible(records(A.G)[g], A.min_landmark_obs, any_seg, seg);
      if (ok) t = (int32_t)g;
      else stale = true;
    }
  }
  if (r < A.K.q_max_rows) A.tgt[r] = t;
  count_wave(stale, &A.st[6]);
}

extern "C" __global__ __launch_bounds__(FXE_WG) void k_exp_scan(FxMapExpectArgs A) {
  __shared__ double s_x[FXE_CHUNK], s_y[FXE_CHUNK], s_k2[FXE_CHUNK];
  __shared__ int32_t s_t[FXE_CHUNK];
  __shared__ uint32_t s_begin[FXE_BUCKETS], s_first[FXE_BUCKETS + 1u];

  const uint32_t tid = threadIdx.x, b = blockIdx.x;
  const KpView V = query_view(A.K);
  if (b >= V.S || !scan_used(A.loc, b, A.require_flags)) return;  // (uniform)
  uint32_t seg;
  bool any_seg;
  const bool some_segment = wanted_segment(A.G.header, A.segment, seg, any_seg);  // (uniform)
  const fx_pose P = loc_of(A.loc, b)->pose;
  uint32_t q_lo, q_hi;
  scan_rows(V, b, q_lo, q_hi);
  const uint32_t n_rows = q_hi - q_lo, n_chunks = (n_rows + FXE_CHUNK - 1u) / FXE_CHUNK;

  // the buckets to walk, each once, and where each one's landmarks begin in the flattened order
  if (tid == 0u) {
    uint32_t ids[FXE_BUCKETS], n = 0u;
    const double cx = floor(P.tx * A.G.inv_edge), cy = floor(P.ty * A.G.inv_edge);
    if (fabs(cx) < kReach && fabs(cy) < kReach) {
      const long long ix = (long long)cx, iy = (long long)cy;
      for (int oy = -1; oy <= 1; ++oy)
        for (int ox = -1; ox <= 1; ++ox) {
          const uint32_t k = bucket_of_cell(ix + ox, iy + oy, A.G.table);
          bool met = false;
          for (uint32_t j = 0u; j < n; ++j) met = met || ids[j] == k;
          if (!met) ids[n++] = k;
        }
    }
    ids[n++] = A.G.table;
    uint32_t total = 0u;
    for (uint32_t j = 0u; j < FXE_BUCKETS; ++j) {
      uint32_t lo = 0u, len = 0u;
      if (j < n) {
        lo = min(bucket_begin(A.G, ids[j]), A.G.cap);
        len = max(min(bucket_end(A.G, ids[j]), A.G.cap), lo) - lo;
      }
      s_begin[j] = lo, s_first[j] = total;
      total += len;
    }
    s_first[FXE_BUCKETS] = total;
  }
  if (tid == 0u) atomicAdd(&A.st[0], 1u);
  __syncthreads();
  const uint32_t total = some_segment ? s_first[FXE_BUCKETS] : 0u;

  auto stage = [&](uint32_t ch) {
    const uint32_t lo = q_lo + ch * FXE_CHUNK, n = min(FXE_CHUNK, q_hi - lo);
    for (uint32_t i = tid; i < n; i += FXE_WG) {
      const float4 k = V.kp[lo + i];
      const double kx = (double)k.x, ky = (double)k.y;
      s_x[i] = kx, s_y[i] = ky, s_k2[i] = kx * kx + ky * ky, s_t[i] = A.tgt[lo + i];
    }
  };
  if (n_chunks == 1u) {
    stage(0u);
    __syncthreads();
  }

  uint32_t c_range = 0u, c_box = 0u, c_shadow = 0u, c_exp = 0u, c_seen = 0u, c_first = 0u;
  for (uint32_t base = 0u; base < total; base += FXE_WG) {  // (uniform)
    const uint32_t j = base + tid;
    bool in_range = false, in_box = false;
    uint32_t g = 0u;
    double lx = 0.0, ly = 0.0, l2 = 0.0;
    if (j < total) {
      uint32_t k = 0u;
#pragma unroll
      for (uint32_t q = 1u; q < FXE_BUCKETS; ++q) k += s_first[q] <= j ? 1u : 0u;  // (empty buckets share a first slot: the last one at or below j holds it)
      const FxMapMergeCand c = A.G.cand[s_begin[k] + (j - s_first[k])];
      if (c.id < A.G.cap && record_eligible(records(A.G)[c.id], A.min_landmark_obs, any_seg, seg)) {
        g = c.id;
        const double dx = c.x - P.tx, dy = c.y - P.ty;
        const double d2 = dx * dx + dy * dy;
        lx = P.c * dx + P.s * dy, ly = P.c * dy - P.s * dx;
        l2 = lx * lx + ly * ly;
        in_range = A.lo2 <= d2 && d2 <= A.hi2;
        in_box = A.x_min <= lx && lx <= A.x_max && A.y_min <= ly && ly <= A.y_max;
      }
    }
    bool seen = false, shadowed = false;
    const double wl2 = A.w2 * l2;
    for (uint32_t ch = 0u; ch < n_chunks; ++ch) {  // (uniform)
      if (n_chunks > 1u) {
        __syncthreads();  // (the readers of the chunk before)
        stage(ch);
        __syncthreads();
      }
      if (!in_range) continue;
      const uint32_t n = min(FXE_CHUNK, n_rows - ch * FXE_CHUNK);
      for (uint32_t i = 0u; i < n; ++i) {
        const int32_t t = s_t[i];
        if (t == -2) continue;
        if (t == (int32_t)g) {
          seen = true;
          continue;
        }
        const double kx = s_x[i], ky = s_y[i];
        const double along = kx * lx + ky * ly, crs = kx * ly - ky * lx;
        shadowed = shadowed || (s_k2[i] < l2 && along > 0.0 && crs * crs <= wl2);
      }
    }
    if (in_range) {
      shadowed = shadowed && A.w2 > 0.0;
      const bool expected = seen || (in_box && !shadowed);
      c_range += 1u, c_box += in_box ? 1u : 0u, c_shadow += in_box && !seen && shadowed ? 1u : 0u;
      c_exp += expected ? 1u : 0u, c_seen += seen ? 1u : 0u;
      if (expected && atomicAdd(&A.cnt_e[g], 1u) == 0u) c_first += 1u;  // (the first of this call to count the landmark)
      if (seen) atomicAdd(&A.cnt_s[g], 1u);
    }
  }
  add_wave(c_range, &A.st[1]);
  add_wave(c_box, &A.st[2]);
  add_wave(c_shadow, &A.st[3]);
  add_wave(c_exp, &A.st[4]);
  add_wave(c_seen, &A.st[5]);
  add_wave(c_first, &A.st[7]);
}

extern "C" __global__ __launch_bounds__(FXE_WG) void k_exp_emit(FxMapExpectArgs A) {
  const uint32_t i = blockIdx.x * FXE_WG + threadIdx.x;
  if (i < A.G.cap) {
    const uint32_t e = A.cnt_e[i], sn = A.cnt_s[i];
    if (A.mode == FX_EXPECT_WRITE) {
      A.expected[i] = e, A.seen[i] = sn;
    } else {
      if (e) A.expected[i] += e;
      if (sn) A.seen[i] += sn;
    }
  }
  if (i == 0u && A.result)
    for (uint32_t k = 0u; k < FX_MAP_EXPECT_ST_WORDS; ++k) A.result[k] = A.st[k];
}

extern "C" hipError_t fxk_map_expect(hipStream_t s, const FxMapExpectArgs &A) {
  const dim3 wg(FXE_WG);
  (void)fxk_map_grid_build(s, A.G);
  // both kinds of counts and the state words behind them are one region of the scratch (fxk_map_expect_scratch)
  const hipError_t e = hipMemsetAsync(A.cnt_e, 0, (2u * (size_t)A.G.cap + FX_MAP_EXPECT_ST_WORDS) * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  if (A.K.q_max_rows) hipLaunchKernelGGL(k_exp_name, dim3((A.K.q_max_rows + FXE_WG - 1u) / FXE_WG), wg, 0, s, A);
  hipLaunchKernelGGL(k_exp_scan, dim3(A.K.n_scans), wg, 0, s, A);
  hipLaunchKernelGGL(k_exp_emit, dim3((A.G.cap + FXE_WG - 1u) / FXE_WG), wg, 0, s, A);
  return hipGetLastError();
}

// bytes of the context's scratch for a map of A->G.cap landmarks and q_max_rows rows, and the pointers carved out of it: the grid's
// part of the merge's layout first (the calls share the buffer: they are ordered on one stream), then this call's arrays
extern "C" size_t fxk_map_expect_scratch(FxMapExpectArgs *A, uint8_t *base) {
  FxCarve C{base, fxk_map_merge_scratch(&A->G, base)};
  A->G.prop = A->G.pred = A->G.succ = nullptr, A->G.keep = nullptr;  // (the grid's mark leaves the merge's words alone)
  const size_t cap = A->G.cap;
  A->cnt_e = C.take<uint32_t>(2u * cap + FX_MAP_EXPECT_ST_WORDS);
  A->cnt_s = base ? A->cnt_e + cap : (uint32_t *)nullptr;
  A->st = base ? A->cnt_s + cap : (uint32_t *)nullptr;
  A->tgt = C.take<int32_t>(A->K.q_max_rows);
  return C.o;
}
