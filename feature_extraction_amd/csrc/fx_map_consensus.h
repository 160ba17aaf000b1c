// fx_map_consensus.h — the consensus of one workgroup over correspondences between points under a prior and map landmarks, fp64:
// the pool's ranking, the hypothesis stage, the refit and the final inlier set that fx_map_localize (a scan's rows against the map,
// csrc/fx_map_localize.hip) and fx_map_join_segments (a segment's landmarks against another segment's, csrc/fx_map_join.hip) share.
// include/fx.h states the clauses once under fx_map_localize; this is their one statement on the device.  The two callers differ
// in where the correspondences come from: the gather is the caller's.
//
// One 256-thread workgroup, shaped like k_register:
//   gather      the caller's: fills xy, d2, dz and row of the slots [0, min(found, FXC_MAP_MAX_CORR)) in the order that defines
//               "the first 1024" and returns found (uniform); the slots are visible to the workgroup when it returns
//   rank        the pool: the H correspondences of lowest (d2 bits, slot), by counting in LDS (rows / ids ascend with the slot)
//   hypotheses  the samples dealt to the threads by stride; a thread walks the correspondences once (all lanes read the same LDS
//               address, a broadcast); (count, lowest sample) reduced by shuffles, then over the wavefronts in LDS
//   refit       thread 0 runs the sequential fp64 sums; the membership tests between them are dealt to all threads
// The hypothesis, the agreement test and the refit are fx_consensus.h's, which fx_register.hip instantiates in fp32.
// LDS: 1024 x (32 B of xy + 8 B of d2 bits + 8 B of t_z - q_z + 4 B row + 4 B flags) + the pool = 57.9 KB.
#ifndef FX_MAP_CONSENSUS_H_
#define FX_MAP_CONSENSUS_H_
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fx_consensus.h"

#define FXC_MAP_WG 256
#define FXC_MAP_NWAVE (FXC_MAP_WG / 64)
#define FXC_MAP_MAX_CORR 1024u
#define FXC_MAP_MAX_HYP 128u
#define FXC_MAP_IDX_BITS 13  // samples of a pool of 128: 8128 < 2^13

static_assert(FXC_MAP_MAX_HYP * (FXC_MAP_MAX_HYP - 1u) / 2u < (1u << FXC_MAP_IDX_BITS), "sample index bits");
static_assert(FXC_MAP_MAX_CORR < (1u << (32 - FXC_MAP_IDX_BITS)), "count bits");

namespace fxc {
struct MapConsensusLds {
  double4 xy[FXC_MAP_MAX_CORR];             // (qx, qy, tx, ty): the point under the prior, the landmark
  unsigned long long d2[FXC_MAP_MAX_CORR];  // d2 bits of the association
  double dz[FXC_MAP_MAX_CORR];              // t_z - q_z
  uint32_t row[FXC_MAP_MAX_CORR];           // the caller's name of the correspondence: a row, a landmark id
  uint32_t flag[FXC_MAP_MAX_CORR];          // bit 0 / 1 = member of the first / second inlier set
  uint32_t pool[FXC_MAP_MAX_HYP];           // pool rank -> correspondence
  uint32_t wave[FXC_MAP_NWAVE];
  Fit fit;
  uint32_t final;  // the flag bit of the final inlier set
};
// n_corr and truncated: every thread.  The rest: thread 0 of a call that returned true.
struct MapConsensusOut {
  uint32_t n_corr;
  bool truncated;  // the gather found more than FXC_MAP_MAX_CORR
  double dc, ds, dtx, dty, dtz;
  float rms;
  uint32_t n_inliers, hyp_a, hyp_b;  // hyp_a, hyp_b: row[] of the winning sample
};

// false (uniform): fewer than 2 correspondences, or no sample passed the gates with 2 agreeing.  true: O is filled, and
// (L.flag[i] & L.final) != 0 marks the final inlier set among the slots [0, O.n_corr), visible to the workgroup.
template <typename Gather>
__device__ __forceinline__ bool map_consensus(MapConsensusLds &L, Gather gather, float inlier_dist, float min_baseline, uint32_t hyp_corr,
                                              MapConsensusOut &O) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t found = gather(L);  // (uniform)
  const uint32_t n_corr = min(found, FXC_MAP_MAX_CORR);
  O.n_corr = n_corr, O.truncated = found > FXC_MAP_MAX_CORR;
  const uint32_t H = min(n_corr, hyp_corr);

  // ---- rank the pool: correspondence i has rank #{j : (d2_j, j) < (d2_i, i)} (rows ascend with i); ranks below H are the pool
  for (uint32_t i = tid; i < n_corr; i += FXC_MAP_WG) {
    const unsigned long long di = L.d2[i];
    uint32_t rank = 0u;
    for (uint32_t j = 0; j < n_corr && rank < H; ++j) {
      const unsigned long long dj = L.d2[j];
      rank += (dj < di || (dj == di && j < i)) ? 1u : 0u;
    }
    if (rank < H) L.pool[rank] = i;
  }
  __syncthreads();

  // ---- hypotheses: key = count << 13 | (8191 - sample), the maximum wins: most agreeing, then the lowest sample
  const double idd = (double)inlier_dist, mbd = (double)min_baseline;
  const double mb2 = mbd * mbd, gate = 2.0 * idd, id2 = idd * idd;
  const uint32_t n_samples = H * (H - (H ? 1u : 0u)) / 2u;
  uint32_t best = 0u;
  for (uint32_t idx = tid; idx < n_samples; idx += FXC_MAP_WG) {
    uint32_t a, c;
    sample_ranks(idx, H, a, c);
    Hyp<double> h;
    if (!hypothesis(L.xy[L.pool[a]], L.xy[L.pool[c]], mb2, gate, h)) continue;
    uint32_t count = 0u;
    for (uint32_t i = 0; i < n_corr; ++i) count += agrees(h, L.xy[i], id2) ? 1u : 0u;
    if (count >= 2u) best = max(best, (count << FXC_MAP_IDX_BITS) | (((1u << FXC_MAP_IDX_BITS) - 1u) - idx));
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o, 64));
  if (lane == 0u) L.wave[wave] = best;
  __syncthreads();
  best = max(max(L.wave[0], L.wave[1]), max(L.wave[2], L.wave[3]));
  if (!best) return false;  // (uniform)

  // ---- the winner's agreeing set (bit 0): the same operations give the same bits
  uint32_t wa, wb;
  sample_ranks(((1u << FXC_MAP_IDX_BITS) - 1u) - (best & ((1u << FXC_MAP_IDX_BITS) - 1u)), H, wa, wb);
  const uint32_t n0 = best >> FXC_MAP_IDX_BITS;
  Hyp<double> h0;
  (void)hypothesis(L.xy[L.pool[wa]], L.xy[L.pool[wb]], mb2, gate, h0);
  for (uint32_t i = tid; i < n_corr; i += FXC_MAP_WG) L.flag[i] = agrees(h0, L.xy[i], id2) ? 1u : 0u;
  __syncthreads();
  if (tid == 0u) {
    Fit f;
    f.c = h0.c, f.s = h0.s;
    fit_set(L.xy, L.flag, n_corr, 1u, n0, f);
    L.fit = f;
  }
  __syncthreads();
  // ---- the set the first fit agrees with (bit 1)
  {
    const Fit f = L.fit;
    for (uint32_t i = tid; i < n_corr; i += FXC_MAP_WG) L.flag[i] |= residual2(f, L.xy[i]) <= id2 ? 2u : 0u;
  }
  __syncthreads();
  if (tid == 0u) {
    Fit f = L.fit;
    uint32_t n1 = 0u;
    for (uint32_t i = 0; i < n_corr; ++i) n1 += (L.flag[i] >> 1) & 1u;
    uint32_t bit = 1u, n = n0;
    if (n1 >= 2u) {
      bit = 2u, n = n1;
      fit_set(L.xy, L.flag, n_corr, bit, n, f);
    }
    double sz = 0.0, sr = 0.0;
    for (uint32_t i = 0; i < n_corr; ++i)
      if (L.flag[i] & bit) {
        sz += L.dz[i];
        sr += residual2(f, L.xy[i]);
      }
    O.dc = f.c, O.ds = f.s, O.dtx = f.tx, O.dty = f.ty, O.dtz = sz / (double)n;
    O.rms = (float)sqrt(sr / (double)n);
    O.n_inliers = n;
    O.hyp_a = L.row[L.pool[wa]], O.hyp_b = L.row[L.pool[wb]];
    L.final = bit;
  }
  __syncthreads();
  return true;
}
}  // namespace fxc
#endif
