// fx_map_constellation.h — the constellation search that fx_map_relocalize (csrc/fx_map_relocalize.hip: a scan's keypoints laid on
// the map's landmarks) and fx_map_find_loop (csrc/fx_map_find_loop.hip: a segment's recent landmarks laid on its old ones, or on
// another segment's) share: include/fx.h states the seed, hypothesis, score, winner and rival clauses once, this header is their
// one statement on the device.
//
// A Search describes one search: the POINTS (a scan's used keypoints, a loop's queries) as doubles in the context's scratch, the
// two grids over the map (fx_map_grid.h) and the byte a landmark that the points may be laid on carries in `elig` (1; every other
// value is passed over).  The definition is over ALL (seed, g, h) and all (point, landmark) pairs; the grids only find the
// landmarks that can pass a gate:
//   P, the pair grid   gate distance pd = (xb + pt)(1 + 2^-20), xb = (double)max_baseline, pt = (double)pair_tol.  A pair (g, h)
//                      passes fxc::hypothesis only if fl|fl(sqrt lq2) - fl(sqrt lt2)| <= pt with lq2 <= xb xb, so
//                      sqrt(lt2) <= (xb + pt)(1 + 2^-50) and the computed lt2 = fl(dx dx + dy dy) <= pd pd: the grid's proof then
//                      puts h in the 3 x 3 cells about g's or in the far bucket.  The walk applies no distance gate of its own:
//                      the hypothesis does.  A bucket is walked ONCE (the nine cells may hash to one bucket): hypotheses are counted.
//   Q, the score grid  gate distance id = (double)inlier_dist, as fx_map_localize's grid with its search distance.
// Every decision is an integer or a minimum / maximum over a total order, every fp64 value an ordered chain on one lane (the
// build's -ffp-contract=off): the same bytes from run to run, whichever call runs the search.
#ifndef FX_MAP_CONSTELLATION_H_
#define FX_MAP_CONSTELLATION_H_
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_consensus.h"
#include "fx_map_grid.h"

#define FXR_WG 256
#define FXR_NWAVE (FXR_WG / 64)
#define FXR_MAX_PT 64u  // points of a search (FX_RELOC_MAX_KP, FX_FIND_MAX_QUERY)
#define FXR_MAX_PAIRS (FXR_MAX_PT * (FXR_MAX_PT - 1u) / 2u)

static_assert(FXR_CHUNK == FXR_WG && sizeof(FxRelocPartial) == 16 && sizeof(FxRelocWinner) == 48, "fx_device.h");

namespace fxs {
using namespace fxc;
using namespace fxg;

struct Search {
  const FxMapMergeArgs *P, *Q;   // the pair grid and the score grid
  const uint8_t *elig;           // [cap]: 1, the points may be laid on the landmark
  const double *pt;              // [n_pt][3]: the points
  uint32_t n_pt, n_seeds;
  const uint32_t *seeds;         // [max_seeds]: a | b << 8 of seed rank s
  float inlier_dist, pair_tol, min_baseline;
  uint32_t max_seeds, chunks;
  FxRelocPartial *partial;       // [max_seeds][chunks]
  FxRelocWinner *win;
  unsigned long long *n_hyp;
  uint32_t *runner;
};

__device__ __forceinline__ unsigned long long bits_of(double v) { return (unsigned long long)__double_as_longlong(v); }

// the image of a point under a transform (include/fx.h: the image expression)
__device__ __forceinline__ void image(const Hyp<double> &h, double x, double y, double &wx, double &wy) {
  wx = (h.c * x - h.s * y) + h.tx;
  wy = (h.s * x + h.c * y) + h.ty;
}
// does (wx, wy) land on an eligible landmark: d2 <= id2, d2 as in fx_map_localize's association
__device__ __forceinline__ bool lands(const FxMapMergeArgs &G, const uint8_t *elig, double wx, double wy, double id2) {
  bool hit = false;
  grid_neighbourhood(G, floor(wx * G.inv_edge), floor(wy * G.inv_edge), [&](uint32_t b) {
    if (hit) return;
    const uint32_t end = min(bucket_end(G, b), G.cap);
    for (uint32_t p = bucket_begin(G, b); p < end; ++p) {
      const FxMapMergeCand c = G.cand[p];
      const double dx = c.x - wx, dy = c.y - wy;
      if (dx * dx + dy * dy <= id2 && c.id < G.cap && elig[c.id] == 1) {
        hit = true;
        break;
      }
    }
  });
  return hit;
}
// the eligible landmark of lowest (d2 bits, id) with d2 <= id2, -1: none
__device__ __forceinline__ int32_t nearest(const FxMapMergeArgs &G, const uint8_t *elig, double wx, double wy, double id2) {
  bool any = false;
  unsigned long long best = 0ull;
  uint32_t id = 0u;
  grid_neighbourhood(G, floor(wx * G.inv_edge), floor(wy * G.inv_edge), [&](uint32_t b) {
    const uint32_t end = min(bucket_end(G, b), G.cap);
    for (uint32_t p = bucket_begin(G, b); p < end; ++p) {
      const FxMapMergeCand c = G.cand[p];
      const double dx = c.x - wx, dy = c.y - wy;
      const double d2 = dx * dx + dy * dy;
      if (!(d2 <= id2) || c.id >= G.cap || elig[c.id] != 1) continue;
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
// the eligible landmarks h != g of the pair grid's buckets about g, each bucket once: visit(h)
template <typename Visit>
__device__ __forceinline__ void pairs_about(const FxMapMergeArgs &G, const uint8_t *elig, const FxMapMergeCand &g, Visit visit) {
  uint32_t bk[10];
  uint32_t nb = 0u;
  grid_neighbourhood(G, floor(g.x * G.inv_edge), floor(g.y * G.inv_edge), [&](uint32_t bb) {
    bool seen = false;
    for (uint32_t i = 0; i < nb; ++i) seen |= bk[i] == bb;
    if (!seen) bk[nb++] = bb;
  });
  for (uint32_t i = 0; i < nb; ++i) {
    const uint32_t end = min(bucket_end(G, bk[i]), G.cap);
    for (uint32_t p2 = bucket_begin(G, bk[i]); p2 < end; ++p2) {
      const FxMapMergeCand h = G.cand[p2];
      if (h.id == g.id || h.id >= G.cap || elig[h.id] != 1) continue;
      visit(h);
    }
  }
}

// The seeds of n_pt points whose x and y are in LDS (a whole workgroup of FXR_WG threads; s_key holds FXR_MAX_PAIRS words, *s_count
// is 0 and the points are visible on entry): the candidate pairs (a, c), a < c, in lexicographic order with mb mb <= d2 <= xb xb,
// ranked by descending d2 bits, then ascending (a, c); the ranks below max_seeds go to seeds[rank] = a | c << 8.  On return
// *s_count is the number of candidates (the barrier between the two loops).
__device__ __forceinline__ void rank_seeds(const double *s_x, const double *s_y, uint32_t n_pt, float min_baseline, float max_baseline,
                                           uint32_t max_seeds, uint32_t *seeds, unsigned long long *s_key, uint32_t *s_count) {
  const uint32_t tid = threadIdx.x;
  const double mbd = (double)min_baseline, xbd = (double)max_baseline;
  const double mb2 = mbd * mbd, xb2 = xbd * xbd;
  const uint32_t n_pairs = n_pt * (n_pt - (n_pt ? 1u : 0u)) / 2u;
  for (uint32_t idx = tid; idx < n_pairs; idx += FXR_WG) {
    uint32_t a, c;
    sample_ranks(idx, n_pt, a, c);
    const double dx = s_x[c] - s_x[a], dy = s_y[c] - s_y[a];
    const double d2 = dx * dx + dy * dy;
    const bool ok = mb2 <= d2 && d2 <= xb2;
    s_key[idx] = ok ? bits_of(d2) : 0ull;  // 0: no candidate (mb mb is never 0)
    if (ok) atomicAdd(s_count, 1u);
  }
  __syncthreads();
  for (uint32_t idx = tid; idx < n_pairs; idx += FXR_WG) {
    const unsigned long long ki = s_key[idx];
    if (!ki) continue;
    uint32_t rank = 0u;
    for (uint32_t j = 0; j < n_pairs && rank < max_seeds; ++j) {
      const unsigned long long kj = s_key[j];
      rank += (kj > ki || (kj == ki && j < idx)) ? 1u : 0u;
    }
    if (rank < max_seeds) {
      uint32_t a, c;
      sample_ranks(idx, n_pt, a, c);
      seeds[rank] = a | (c << 8);
    }
  }
}

// A workgroup of the hypothesis kernel: seed s, FXR_CHUNK slots of P from chunk * FXR_CHUNK, a lane a landmark g.  The lane walks
// the h about g, forms the hypothesis a -> g, b -> h and scores it: the points come from LDS, each image walks Q's 3 x 3 cells.
//   PASS 0  the lane keeps its best (score, lowest h); the workgroup's best (score, lowest g, lowest h) goes to `partial`, the
//           hypotheses counted go to n_hyp (64-bit integer atomic add)
//   PASS 1  a hypothesis is scored only when it is a rival of the winner; the best score among them goes to `runner` by a 32-bit
//           integer atomic max
template <int PASS>
__device__ __forceinline__ void hyp_block(const Search &S, uint32_t s, uint32_t chunk) {
  __shared__ double s_x[FXR_MAX_PT], s_y[FXR_MAX_PT];
  __shared__ unsigned long long s_best[FXR_NWAVE];
  __shared__ uint32_t s_h[FXR_NWAVE];

  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n_pt = min(S.n_pt, FXR_MAX_PT);
  if (s >= S.n_seeds) return;  // (uniform)
  FxRelocWinner W;
  W.score = 0u;
  if (PASS == 1) {
    W = *S.win;
    if (!W.score) return;  // (uniform) no winner: no rival
  }
  if (tid < n_pt) {
    const double *q = S.pt + (size_t)tid * 3u;
    s_x[tid] = q[0], s_y[tid] = q[1];
  }
  __syncthreads();
  const uint32_t seed = S.seeds[s];
  const uint32_t ka = seed & 255u, kb = (seed >> 8) & 255u;
  const double idd = (double)S.inlier_dist, mbd = (double)S.min_baseline, ptd = (double)S.pair_tol;
  const double id2 = idd * idd, mb2 = mbd * mbd;
  const double qax = s_x[ka], qay = s_y[ka], qbx = s_x[kb], qby = s_y[kb];

  // the winner's images of its own seed points (the rival test)
  double wax = 0.0, way = 0.0, wbx = 0.0, wby = 0.0, rax = 0.0, ray = 0.0, rbx = 0.0, rby = 0.0, g2 = 0.0;
  if (PASS == 1) {
    const uint32_t ws = S.seeds[W.seed];
    const uint32_t wa = ws & 255u, wb = (ws >> 8) & 255u;
    Hyp<double> T;
    T.c = W.c, T.s = W.s, T.tx = W.tx, T.ty = W.ty;
    rax = s_x[wa], ray = s_y[wa], rbx = s_x[wb], rby = s_y[wb];
    image(T, rax, ray, wax, way);
    image(T, rbx, rby, wbx, wby);
    const double two = 2.0 * idd;
    g2 = two * two;
  }

  const FxMapMergeArgs &G = *S.P;
  const uint32_t p = chunk * FXR_CHUNK + tid, n_grid = min(G.st[3], G.cap);
  uint32_t best_score = 0u, best_h = FXMM_NONE, g_id = FXMM_NONE, count = 0u;
  if (p < n_grid) {
    const FxMapMergeCand g = G.cand[p];
    if (g.id < G.cap && S.elig[g.id] == 1) {
      g_id = g.id;
      const double4 PA = make_double4(qax, qay, g.x, g.y);
      pairs_about(G, S.elig, g, [&](const FxMapMergeCand &h) {
        Hyp<double> T;
        if (!hypothesis(PA, make_double4(qbx, qby, h.x, h.y), mb2, ptd, T)) return;
        if (PASS == 0) ++count;
        if (PASS == 1) {  // a rival moves a* or b* by more than 2 id from where the winner puts it
          double ux, uy, vx, vy;
          image(T, rax, ray, ux, uy);
          image(T, rbx, rby, vx, vy);
          const double dax = ux - wax, day = uy - way, dbx = vx - wbx, dby = vy - wby;
          if (!(dax * dax + day * day > g2 || dbx * dbx + dby * dby > g2)) return;
        }
        uint32_t score = 0u;
        for (uint32_t k = 0; k < n_pt; ++k) {
          double wx, wy;
          image(T, s_x[k], s_y[k], wx, wy);
          score += lands(*S.Q, S.elig, wx, wy, id2) ? 1u : 0u;
        }
        if (PASS == 0) {
          if (score >= 2u && (score > best_score || (score == best_score && h.id < best_h))) best_score = score, best_h = h.id;
        } else {
          best_score = max(best_score, score);
        }
      });
    }
  }
  if (PASS == 1) {
#pragma unroll
    for (int o = 32; o; o >>= 1) best_score = max(best_score, (uint32_t)__shfl_xor((int)best_score, o, 64));
    if (lane == 0u && best_score) atomicMax(S.runner, best_score);
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
    if (cnt) atomicAdd(S.n_hyp, cnt);
  }
  __syncthreads();
  if (tid == 0u) {
#pragma unroll
    for (uint32_t w = 1; w < FXR_NWAVE; ++w)
      if (s_best[w] > key) key = s_best[w], hh = s_h[w];
    FxRelocPartial r;
    r.score = (uint32_t)(key >> 32), r.g = key ? 0xffffffffu - (uint32_t)key : FXMM_NONE, r.h = hh, r.pad_ = 0u;
    S.partial[(size_t)s * S.chunks + chunk] = r;
  }
}

// One workgroup: the partials' best by (score, lowest seed, lowest g, lowest h) and the winner's transform, to *S.win (score 0: no
// winner)
__device__ __forceinline__ void reduce_block(const Search &S) {
  __shared__ FxRelocPartial s_p[FXR_WG];
  __shared__ uint32_t s_seed[FXR_WG];
  const uint32_t tid = threadIdx.x;
  const uint32_t n_seeds = min(S.n_seeds, S.max_seeds);
  const unsigned long long total = (unsigned long long)n_seeds * S.chunks;
  FxRelocWinner w;
  w.score = 0u, w.seed = w.g = w.h = FXMM_NONE;
  for (unsigned long long i = tid; i < total; i += FXR_WG) {
    const uint32_t s = (uint32_t)(i / S.chunks), c = (uint32_t)(i % S.chunks);
    const FxRelocPartial r = S.partial[(size_t)s * S.chunks + c];
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
  const FxMapMergeArgs &G = *S.P;
  if (w.score && w.g < G.cap && w.h < G.cap) {  // the same operations give the same bits
    const uint32_t seed = S.seeds[w.seed];
    const double *qa = S.pt + (size_t)(seed & 255u) * 3u, *qb = S.pt + (size_t)((seed >> 8) & 255u) * 3u;
    const fx_map_landmark Rg = records(G)[w.g], Rh = records(G)[w.h];
    const double mbd = (double)S.min_baseline;
    Hyp<double> T;
    if (hypothesis(make_double4(qa[0], qa[1], Rg.x, Rg.y), make_double4(qb[0], qb[1], Rh.x, Rh.y), mbd * mbd, (double)S.pair_tol, T))
      w.c = T.c, w.s = T.s, w.tx = T.tx, w.ty = T.ty;
    else
      w.score = 0u;  // (cannot happen)
  } else {
    w.score = 0u;
  }
  *S.win = w;
}
}  // namespace fxs
#endif
