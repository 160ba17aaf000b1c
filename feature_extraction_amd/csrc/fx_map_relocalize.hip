// fx_map_relocalize.hip — a scan's pose in the persistent map without a prior (include/fx.h fx_map_relocalize): pairs of keypoints
// (seeds) are laid on pairs of landmarks of the same length, and each rigid transform that results is scored by the keypoints it
// lands on a landmark.
//
// The definition is over ALL (seed, g, h) and all (keypoint, landmark) pairs; two grids (fx_map_grid.h, built by fx_map_grid.hip,
// alive together in the context's scratch) only find the landmarks that can pass a gate:
//   P, the pair grid   gate distance pd = (xb + pt)(1 + 2^-20), xb = (double)max_baseline, pt = (double)pair_tol.  A pair (g, h)
//                      passes fxc::hypothesis only if fl|fl(sqrt lq2) - fl(sqrt lt2)| <= pt with lq2 <= xb xb, so
//                      sqrt(lt2) <= (xb + pt)(1 + 2^-50) and the computed lt2 = fl(dx dx + dy dy) <= pd pd: the grid's proof then
//                      puts h in the 3 x 3 cells about g's or in the far bucket.  The walk applies no distance gate of its own:
//                      the hypothesis does.  A bucket is walked ONCE (the nine cells may hash to one bucket): hypotheses are counted.
//   Q, the score grid  gate distance id = (double)inlier_dist, as fx_map_localize's grid with its search distance.
// Both hold the merge's live set; the walks filter by the eligibility bytes k_rl_elig writes.  Every decision is an integer or a
// minimum / maximum over a total order, every fp64 value an ordered chain on one lane (the build's -ffp-contract=off): the same
// bytes from run to run and with any number of contexts in flight.  The map is only read.
//
// Launches, in stream order, after fxk_map_grid_build's five for P and five for Q:
//   k_rl_elig     a thread a landmark: eligible or not (alias -1, n_obs >= min_landmark_obs, finite x, y, z, the segment)
//   k_rl_prep     a workgroup a scan: map_id_of_row = -1 (all workgroups share the rows), the first FX_RELOC_MAX_KP finite rows in
//                 ascending row by ballot + prefix, the candidate pairs' d2 in LDS, their ranks by counting, the first max_seeds
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

#include "fx_consensus.h"
#include "fx_map_grid.h"
#include "../../include/fx.h"

using namespace fxc;
using namespace fxg;

#define FXR_WG 256
#define FXR_NWAVE (FXR_WG / 64)
#define FXR_MAX_PAIRS (FX_RELOC_MAX_KP * (FX_RELOC_MAX_KP - 1u) / 2u)

static_assert(sizeof(fx_relocalization) == 96 && sizeof(fx_relocalize_options) == 40 && sizeof(fx_pose) == 48, "include/fx.h");
static_assert(FXR_CHUNK == FXR_WG && FX_RELOC_MAX_KP == 64u && sizeof(FxRelocPartial) == 16 && sizeof(FxRelocWinner) == 48, "fx_device.h");

extern "C" hipError_t fxk_map_grid_build(hipStream_t s, const FxMapMergeArgs &A);
extern "C" size_t fxk_map_merge_scratch(FxMapMergeArgs *A, uint8_t *base);

namespace {
__device__ __forceinline__ uint32_t rl_scans(const FxMapRelocalizeArgs &A) { return min(min(A.n_scans, A.kp[0]), A.max_scans); }
__device__ __forceinline__ uint32_t rl_rows(const FxMapRelocalizeArgs &A) { return min(min(A.kp[1], A.max_total), A.q_max_rows); }
__device__ __forceinline__ unsigned long long bits_of(double v) { return (unsigned long long)__double_as_longlong(v); }

// the image of a keypoint under a transform (include/fx.h: the image expression)
__device__ __forceinline__ void image(const Hyp<double> &h, double x, double y, double &wx, double &wy) {
  wx = (h.c * x - h.s * y) + h.tx;
  wy = (h.s * x + h.c * y) + h.ty;
}
// does (wx, wy) land on an eligible landmark: d2 <= id2, d2 as in fx_map_localize's association
__device__ __forceinline__ bool lands(const FxMapRelocalizeArgs &A, double wx, double wy, double id2) {
  const FxMapMergeArgs &G = A.Q;
  bool hit = false;
  grid_neighbourhood(G, floor(wx * G.inv_edge), floor(wy * G.inv_edge), [&](uint32_t b) {
    if (hit) return;
    const uint32_t end = min(bucket_end(G, b), G.cap);
    for (uint32_t p = bucket_begin(G, b); p < end; ++p) {
      const FxMapMergeCand c = G.cand[p];
      const double dx = c.x - wx, dy = c.y - wy;
      if (dx * dx + dy * dy <= id2 && c.id < G.cap && A.elig[c.id]) {
        hit = true;
        break;
      }
    }
  });
  return hit;
}
// the eligible landmark of lowest (d2 bits, id) with d2 <= id2, -1: none
__device__ __forceinline__ int32_t nearest(const FxMapRelocalizeArgs &A, double wx, double wy, double id2) {
  const FxMapMergeArgs &G = A.Q;
  bool any = false;
  unsigned long long best = 0ull;
  uint32_t id = 0u;
  grid_neighbourhood(G, floor(wx * G.inv_edge), floor(wy * G.inv_edge), [&](uint32_t b) {
    const uint32_t end = min(bucket_end(G, b), G.cap);
    for (uint32_t p = bucket_begin(G, b); p < end; ++p) {
      const FxMapMergeCand c = G.cand[p];
      const double dx = c.x - wx, dy = c.y - wy;
      const double d2 = dx * dx + dy * dy;
      if (!(d2 <= id2) || c.id >= G.cap || !A.elig[c.id]) continue;
      const unsigned long long k = bits_of(d2);
      if (any && !(k < best || (k == best && c.id < id))) continue;
      any = true, best = k, id = c.id;
    }
  });
  return any ? (int32_t)id : -1;
}
__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int o) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
  return ((unsigned long long)hi << 32) | lo;
}
// is (score, seed, g, h) ahead of the best so far: the highest score, then the lowest (seed, g, h)
__device__ __forceinline__ bool ahead(uint32_t sc, uint32_t s, uint32_t g, uint32_t h, const FxRelocWinner &w) {
  if (sc != w.score) return sc > w.score;
  if (s != w.seed) return s < w.seed;
  if (g != w.g) return g < w.g;
  return h < w.h;
}
}  // namespace

extern "C" __global__ __launch_bounds__(FXR_WG) void k_rl_elig(FxMapRelocalizeArgs A) {
  const uint32_t i = blockIdx.x * FXR_WG + threadIdx.x;
  if (i >= A.P.cap) return;
  bool ok = false;
  if (i < n_landmarks(A.P)) {
    const fx_map_landmark R = records(A.P)[i];
    uint32_t seg = A.segment;
    bool any_seg = A.segment == FX_LOC_ANY_SEGMENT, some = true;
    if (A.segment == FX_LOC_LAST_SEGMENT) {
      const uint32_t n = reinterpret_cast<const fx_map_header *>(A.P.header)->segments;
      some = n != 0u, seg = n - 1u;
    }
    ok = some && A.P.alias[i] == -1 && R.n_obs >= A.min_landmark_obs && isfinite(R.x) && isfinite(R.y) && isfinite(R.z) &&
         (any_seg || R.segment == seg);
  }
  A.elig[i] = ok ? 1 : 0;
}

extern "C" __global__ __launch_bounds__(FXR_WG) void k_rl_prep(FxMapRelocalizeArgs A) {
  __shared__ double s_x[FX_RELOC_MAX_KP], s_y[FX_RELOC_MAX_KP];
  __shared__ unsigned long long s_key[FXR_MAX_PAIRS];  // d2 bits of a candidate pair, 0: no candidate (mb mb is never 0)
  __shared__ uint32_t s_wave[FXR_NWAVE];
  __shared__ uint32_t s_count;

  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, b = blockIdx.x;
  for (unsigned long long r = (unsigned long long)b * FXR_WG + tid; r < A.q_max_rows; r += (unsigned long long)A.n_scans * FXR_WG)
    A.map_id_of_row[r] = -1;
  if (tid == 0u) A.n_hyp[b] = 0ull, A.runner[b] = 0u, s_count = 0u;
  const uint32_t S = rl_scans(A), rows = rl_rows(A);
  uint32_t *meta = A.meta + 4u * b;
  if (b >= S) {  // (uniform)
    if (tid < 4u) meta[tid] = 0u;
    return;
  }
  const uint32_t *off = kp_block_offsets(A.kp);
  const float4 *kp = kp_block_rows<float4>(A.kp, A.max_scans);
  const uint32_t q_lo = min(off[b], rows), q_hi = max(min(off[b + 1u], rows), q_lo);

  // ---- the used keypoints: the finite rows in ascending row, the first FX_RELOC_MAX_KP kept
  uint32_t found = 0u;  // (uniform)
  for (unsigned long long r0 = q_lo; r0 < q_hi && found <= FX_RELOC_MAX_KP; r0 += FXR_WG) {
    const uint32_t i = (uint32_t)min(r0 + tid, (unsigned long long)q_hi);
    float4 k = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < q_hi) k = kp[i];
    const bool ok = i < q_hi && finite3(k);
    const unsigned long long bal = __ballot(ok);
    if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = 0u, all = 0u;
#pragma unroll
    for (uint32_t w = 0; w < FXR_NWAVE; ++w) {
      const uint32_t n = s_wave[w];
      before += w < wave ? n : 0u;
      all += n;
    }
    const uint32_t slot = found + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
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

  // ---- the candidate pairs (a, c), a < c, in lexicographic order: pair idx's d2 when mb mb <= d2 <= xb xb
  const double mbd = (double)A.min_baseline, xbd = (double)A.max_baseline;
  const double mb2 = mbd * mbd, xb2 = xbd * xbd;
  const uint32_t n_pairs = n_kp * (n_kp - (n_kp ? 1u : 0u)) / 2u;
  for (uint32_t idx = tid; idx < n_pairs; idx += FXR_WG) {
    uint32_t a, c;
    sample_ranks(idx, n_kp, a, c);
    const double dx = s_x[c] - s_x[a], dy = s_y[c] - s_y[a];
    const double d2 = dx * dx + dy * dy;
    const bool ok = mb2 <= d2 && d2 <= xb2;
    s_key[idx] = ok ? bits_of(d2) : 0ull;
    if (ok) atomicAdd(&s_count, 1u);
  }
  __syncthreads();
  // ---- rank: descending d2 bits, then ascending (a, c); the ranks below max_seeds are the seeds
  for (uint32_t idx = tid; idx < n_pairs; idx += FXR_WG) {
    const unsigned long long ki = s_key[idx];
    if (!ki) continue;
    uint32_t rank = 0u;
    for (uint32_t j = 0; j < n_pairs && rank < A.max_seeds; ++j) {
      const unsigned long long kj = s_key[j];
      rank += (kj > ki || (kj == ki && j < idx)) ? 1u : 0u;
    }
    if (rank < A.max_seeds) {
      uint32_t a, c;
      sample_ranks(idx, n_kp, a, c);
      A.seeds[(size_t)b * FX_RELOC_MAX_KP + rank] = a | (c << 8);
    }
  }
  if (tid == 0u) {
    meta[0] = n_kp, meta[1] = min(s_count, A.max_seeds), meta[2] = found > FX_RELOC_MAX_KP ? FX_RELOC_TRUNCATED : 0u, meta[3] = 0u;
  }
}

template <int PASS>
__global__ __launch_bounds__(FXR_WG) void k_rl_hyp(FxMapRelocalizeArgs A) {
  __shared__ double s_x[FX_RELOC_MAX_KP], s_y[FX_RELOC_MAX_KP];
  __shared__ unsigned long long s_best[FXR_NWAVE];
  __shared__ uint32_t s_h[FXR_NWAVE];

  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t b = A.scan0 + blockIdx.z, s = blockIdx.y, chunk = blockIdx.x;
  const uint32_t n_kp = min(A.meta[4u * b], FX_RELOC_MAX_KP), n_seeds = A.meta[4u * b + 1u];
  if (s >= n_seeds) return;  // (uniform)
  FxRelocWinner W;
  W.score = 0u;
  if (PASS == 1) {
    W = A.win[b];
    if (!W.score) return;  // (uniform) no winner: no rival
  }
  if (tid < n_kp) {
    const double *q = A.kq + ((size_t)b * FX_RELOC_MAX_KP + tid) * 3u;
    s_x[tid] = q[0], s_y[tid] = q[1];
  }
  __syncthreads();
  const uint32_t seed = A.seeds[(size_t)b * FX_RELOC_MAX_KP + s];
  const uint32_t ka = seed & 255u, kb = (seed >> 8) & 255u;
  const double idd = (double)A.inlier_dist, mbd = (double)A.min_baseline, ptd = (double)A.pair_tol;
  const double id2 = idd * idd, mb2 = mbd * mbd;
  const double qax = s_x[ka], qay = s_y[ka], qbx = s_x[kb], qby = s_y[kb];

  // the winner's images of its own seed keypoints (the rival test)
  double wax = 0.0, way = 0.0, wbx = 0.0, wby = 0.0, rax = 0.0, ray = 0.0, rbx = 0.0, rby = 0.0, g2 = 0.0;
  if (PASS == 1) {
    const uint32_t ws = A.seeds[(size_t)b * FX_RELOC_MAX_KP + W.seed];
    const uint32_t wa = ws & 255u, wb = (ws >> 8) & 255u;
    Hyp<double> T;
    T.c = W.c, T.s = W.s, T.tx = W.tx, T.ty = W.ty;
    rax = s_x[wa], ray = s_y[wa], rbx = s_x[wb], rby = s_y[wb];
    image(T, rax, ray, wax, way);
    image(T, rbx, rby, wbx, wby);
    const double two = 2.0 * idd;
    g2 = two * two;
  }

  const FxMapMergeArgs &G = A.P;
  const uint32_t p = chunk * FXR_CHUNK + tid, n_grid = min(G.st[3], G.cap);
  uint32_t best_score = 0u, best_h = FXMM_NONE, g_id = FXMM_NONE, count = 0u;
  if (p < n_grid) {
    const FxMapMergeCand g = G.cand[p];
    if (g.id < G.cap && A.elig[g.id]) {
      g_id = g.id;
      // the buckets about g, each once
      uint32_t bk[10];
      uint32_t nb = 0u;
      grid_neighbourhood(G, floor(g.x * G.inv_edge), floor(g.y * G.inv_edge), [&](uint32_t bb) {
        bool seen = false;
        for (uint32_t i = 0; i < nb; ++i) seen |= bk[i] == bb;
        if (!seen) bk[nb++] = bb;
      });
      const double4 PA = make_double4(qax, qay, g.x, g.y);
      for (uint32_t i = 0; i < nb; ++i) {
        const uint32_t end = min(bucket_end(G, bk[i]), G.cap);
        for (uint32_t p2 = bucket_begin(G, bk[i]); p2 < end; ++p2) {
          const FxMapMergeCand h = G.cand[p2];
          if (h.id == g.id || h.id >= G.cap || !A.elig[h.id]) continue;
          Hyp<double> T;
          if (!hypothesis(PA, make_double4(qbx, qby, h.x, h.y), mb2, ptd, T)) continue;
          if (PASS == 0) ++count;
          if (PASS == 1) {  // a rival moves a* or b* by more than 2 id from where the winner puts it
            double ux, uy, vx, vy;
            image(T, rax, ray, ux, uy);
            image(T, rbx, rby, vx, vy);
            const double dax = ux - wax, day = uy - way, dbx = vx - wbx, dby = vy - wby;
            if (!(dax * dax + day * day > g2 || dbx * dbx + dby * dby > g2)) continue;
          }
          uint32_t score = 0u;
          for (uint32_t k = 0; k < n_kp; ++k) {
            double wx, wy;
            image(T, s_x[k], s_y[k], wx, wy);
            score += lands(A, wx, wy, id2) ? 1u : 0u;
          }
          if (PASS == 0) {
            if (score >= 2u && (score > best_score || (score == best_score && h.id < best_h))) best_score = score, best_h = h.id;
          } else {
            best_score = max(best_score, score);
          }
        }
      }
    }
  }
  if (PASS == 1) {
#pragma unroll
    for (int o = 32; o; o >>= 1) best_score = max(best_score, (uint32_t)__shfl_xor((int)best_score, o, 64));
    if (lane == 0u && best_score) atomicMax(&A.runner[b], best_score);
    return;
  }
  // ---- the workgroup's best: the highest score, then the lowest g (a lane a g: no two lanes tie), its lowest h
  unsigned long long key = best_score ? ((unsigned long long)best_score << 32) | (0xffffffffu - g_id) : 0ull, cnt = count;
  uint32_t hh = best_h;
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const unsigned long long ok = shfl_xor64(key, o);
    const uint32_t oh = (uint32_t)__shfl_xor((int)hh, o, 64);
    cnt += shfl_xor64(cnt, o);
    if (ok > key) key = ok, hh = oh;
  }
  if (lane == 0u) {
    s_best[wave] = key, s_h[wave] = hh;
    if (cnt) atomicAdd(&A.n_hyp[b], cnt);
  }
  __syncthreads();
  if (tid == 0u) {
#pragma unroll
    for (uint32_t w = 1; w < FXR_NWAVE; ++w)
      if (s_best[w] > key) key = s_best[w], hh = s_h[w];
    FxRelocPartial r;
    r.score = (uint32_t)(key >> 32), r.g = key ? 0xffffffffu - (uint32_t)key : FXMM_NONE, r.h = hh, r.pad_ = 0u;
    A.partial[((size_t)b * A.max_seeds + s) * A.chunks + chunk] = r;
  }
}

extern "C" __global__ __launch_bounds__(FXR_WG) void k_rl_reduce(FxMapRelocalizeArgs A) {
  __shared__ FxRelocPartial s_p[FXR_WG];
  __shared__ uint32_t s_seed[FXR_WG];
  const uint32_t tid = threadIdx.x, b = blockIdx.x;
  const uint32_t n_seeds = min(A.meta[4u * b + 1u], A.max_seeds);
  const unsigned long long total = (unsigned long long)n_seeds * A.chunks;
  FxRelocWinner w;
  w.score = 0u, w.seed = w.g = w.h = FXMM_NONE;
  for (unsigned long long i = tid; i < total; i += FXR_WG) {
    const uint32_t s = (uint32_t)(i / A.chunks), c = (uint32_t)(i % A.chunks);
    const FxRelocPartial r = A.partial[((size_t)b * A.max_seeds + s) * A.chunks + c];
    if (r.score >= 2u && ahead(r.score, s, r.g, r.h, w)) w.score = r.score, w.seed = s, w.g = r.g, w.h = r.h;
  }
  FxRelocPartial mine;
  mine.score = w.score, mine.g = w.g, mine.h = w.h, mine.pad_ = 0u;
  s_p[tid] = mine, s_seed[tid] = w.seed;
  __syncthreads();
  if (tid != 0u) return;
  for (uint32_t t = 1; t < FXR_WG; ++t) {
    const FxRelocPartial r = s_p[t];
    if (r.score >= 2u && ahead(r.score, s_seed[t], r.g, r.h, w)) w.score = r.score, w.seed = s_seed[t], w.g = r.g, w.h = r.h;
  }
  w.c = 1.0, w.s = 0.0, w.tx = 0.0, w.ty = 0.0;
  if (w.score && w.g < A.P.cap && w.h < A.P.cap) {  // the same operations give the same bits
    const uint32_t seed = A.seeds[(size_t)b * FX_RELOC_MAX_KP + w.seed];
    const double *qa = A.kq + ((size_t)b * FX_RELOC_MAX_KP + (seed & 255u)) * 3u, *qb = A.kq + ((size_t)b * FX_RELOC_MAX_KP + ((seed >> 8) & 255u)) * 3u;
    const fx_map_landmark Rg = records(A.P)[w.g], Rh = records(A.P)[w.h];
    const double mbd = (double)A.min_baseline;
    Hyp<double> T;
    if (hypothesis(make_double4(qa[0], qa[1], Rg.x, Rg.y), make_double4(qb[0], qb[1], Rh.x, Rh.y), mbd * mbd, (double)A.pair_tol, T))
      w.c = T.c, w.s = T.s, w.tx = T.tx, w.ty = T.ty;
    else
      w.score = 0u;  // (cannot happen)
  } else {
    w.score = 0u;
  }
  A.win[b] = w;
}

extern "C" __global__ __launch_bounds__(64) void k_rl_finish(FxMapRelocalizeArgs A) {
  __shared__ int32_t s_lm[FX_RELOC_MAX_KP];
  __shared__ uint32_t s_valid;
  const uint32_t tid = threadIdx.x, b = blockIdx.x;
  const uint32_t S = rl_scans(A);
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
    lm = nearest(A, wx, wy, idd * idd);
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
    if (row < A.q_max_rows) A.map_id_of_row[row] = lm;
  }
}

extern "C" hipError_t fxk_map_relocalize(hipStream_t s, const FxMapRelocalizeArgs &A) {
  (void)fxk_map_grid_build(s, A.P);
  (void)fxk_map_grid_build(s, A.Q);
  hipLaunchKernelGGL(k_rl_elig, dim3((A.P.cap + FXR_WG - 1u) / FXR_WG), dim3(FXR_WG), 0, s, A);
  hipLaunchKernelGGL(k_rl_prep, dim3(A.n_scans), dim3(FXR_WG), 0, s, A);
  auto hyp = [&](int pass) {  // (a grid's z holds 65535 scans)
    FxMapRelocalizeArgs B = A;
    for (B.scan0 = 0u; B.scan0 < A.n_scans; B.scan0 += 65535u) {
      const uint32_t n = A.n_scans - B.scan0 < 65535u ? A.n_scans - B.scan0 : 65535u;
      const dim3 grid(A.chunks, A.max_seeds, n);
      if (pass == 0) hipLaunchKernelGGL(k_rl_hyp<0>, grid, dim3(FXR_WG), 0, s, B);
      else hipLaunchKernelGGL(k_rl_hyp<1>, grid, dim3(FXR_WG), 0, s, B);
    }
  };
  hyp(0);
  hipLaunchKernelGGL(k_rl_reduce, dim3(A.n_scans), dim3(FXR_WG), 0, s, A);
  hyp(1);
  hipLaunchKernelGGL(k_rl_finish, dim3(A.n_scans), dim3(64), 0, s, A);
  return hipGetLastError();
}

// bytes of the context's scratch for a map of A->P.cap landmarks and n_scans scans, and the pointers carved out of it: the pair
// grid in the merge's layout first, the score grid in the same layout behind it, then the call's own arrays
extern "C" size_t fxk_map_relocalize_scratch(FxMapRelocalizeArgs *A, uint8_t *base) {
  size_t o = fxk_map_merge_scratch(&A->P, base);
  o += fxk_map_merge_scratch(&A->Q, base ? base + o : nullptr);
  A->P.prop = A->P.pred = A->P.succ = nullptr, A->P.keep = nullptr;  // (the grid's mark leaves the merge's words alone)
  A->Q.prop = A->Q.pred = A->Q.succ = nullptr, A->Q.keep = nullptr;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += (bytes + 15u) & ~(size_t)15;
    return base ? base + at : (uint8_t *)nullptr;
  };
  const size_t n = A->n_scans, K = FX_RELOC_MAX_KP;
  A->kq = (double *)take(n * K * 3u * 8u);
  A->n_hyp = (unsigned long long *)take(n * 8u);
  A->win = (FxRelocWinner *)take(n * sizeof(FxRelocWinner));
  A->partial = (FxRelocPartial *)take(n * A->max_seeds * A->chunks * sizeof(FxRelocPartial));
  A->krow = (uint32_t *)take(n * K * 4u);
  A->seeds = (uint32_t *)take(n * K * 4u);
  A->meta = (uint32_t *)take(n * 4u * 4u);
  A->runner = (uint32_t *)take(n * 4u);
  A->elig = (uint8_t *)take(A->P.cap);
  return o;
}
