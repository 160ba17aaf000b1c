// fx_register.hip — scan-to-scan rigid motion from descriptor matches (include/fx.h fx_register_matches).
//
// Per pair of row ranges: the matched keypoints (query row i -> m[i].train_row) vote on a rotation about z plus a translation,
// (c, s, tx, ty), and the winning vote is refitted by least squares.  Every decision is an integer or an ordered chain of
// correctly rounded operations (the build's -ffp-contract=off; hipcc's correctly rounded fp32 divide and sqrt): the fp32
// hypothesis stage is the one numpy float32 evaluates, the fp64 refit sums run on ONE lane in ascending query row.  No atomics,
// no global scratch, nothing in completion order: the same bits from run to run and with any number of contexts in flight.
//
// Launches: k_register_init (the inlier words to 0, when the caller wants them) and k_register, one 256-thread workgroup a pair:
//   gather      the pair's correspondences into LDS, compacted in query-row order by ballot + prefix (at most FXR_MAX_CORR)
//   rank        the pool: the H correspondences of lowest (dist2 bits, row), by counting in LDS
//   hypotheses  the samples (a, b), a < b, of pool ranks dealt to the threads by stride; a thread builds its sample's transform
//               in registers and walks the correspondences once — all lanes read the same LDS address, a broadcast —, counting
//               in an integer; (count, lowest sample) is reduced over the wavefront by shuffles and over the four wavefronts in LDS
//   refit       thread 0 runs the sequential fp64 sums; the membership tests between them are dealt to all threads
// The hypothesis, the agreement test and the refit are fx_consensus.h's: fx_map_localize.hip runs the same clauses in fp64.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fx_consensus.h"
#include "fx_device.h"
#include "fx_launch.h"
#include "../../include/fx.h"

using namespace fxc;

#define FXR_WG 256
#define FXR_NWAVE (FXR_WG / 64)
#define FXR_MAX_CORR 1024u
#define FXR_MAX_HYP 128u
#define FXR_IDX_BITS 13  // samples of a pool of 128: 8128 < 2^13

static_assert(sizeof(fx_registration) == 64 && sizeof(fx_register_options) == 20, "include/fx.h");
static_assert(FXR_MAX_HYP * (FXR_MAX_HYP - 1u) / 2u < (1u << FXR_IDX_BITS), "sample index bits");

namespace {
// the (x, y, z, elevation) rows of a keypoint block and how many of them it stores (include/fx.h fx_pack_keypoint_block)
struct KpView {
  const float4 *kp;
  uint32_t stored;
};
__device__ __forceinline__ KpView kp_view(const uint32_t *block, uint32_t max_scans, uint32_t max_total) {
  KpView v;
  v.kp = kp_block_rows<float4>(block, max_scans);
  v.stored = min(block[1], max_total);
  return v;
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void k_register_init(uint32_t *inlier, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) inlier[i] = 0u;
}

extern "C" __global__ __launch_bounds__(FXR_WG) void k_register(FxRegisterArgs A) {
  __shared__ float4 s_xy[FXR_MAX_CORR];    // (qx, qy, tx, ty)
  __shared__ float2 s_z[FXR_MAX_CORR];     // (qz, tz)
  __shared__ uint32_t s_d2[FXR_MAX_CORR];  // dist2 bits; after the ranking: bit 0 / 1 = member of the first / second inlier set
  __shared__ uint32_t s_row[FXR_MAX_CORR];
  __shared__ uint32_t s_pool[FXR_MAX_HYP];  // pool rank -> correspondence
  __shared__ uint32_t s_wave[FXR_NWAVE];
  __shared__ Fit s_fit;
  __shared__ uint32_t s_final;  // the flag bit of the final inlier set

  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, p = blockIdx.x;
  const fx_match_pair pr = reinterpret_cast<const fx_match_pair *>(A.pairs)[p];
  const fx_match *m = reinterpret_cast<const fx_match *>(A.matches);
  const KpView Q = kp_view(A.q_kp, A.q_max_scans, A.q_max_total), T = kp_view(A.t_kp, A.t_max_scans, A.t_max_total);
  uint32_t q_lo, q_hi;
  clip_range(pr.q_row0, pr.q_rows, A.q_max_rows, q_lo, q_hi);

  // ---- gather: the correspondences in ascending query row, the first FXR_MAX_CORR kept
  uint32_t found = 0u;  // (uniform)
  for (unsigned long long r0 = q_lo; r0 < q_hi && found <= FXR_MAX_CORR; r0 += FXR_WG) {
    const uint32_t i = (uint32_t)min(r0 + tid, (unsigned long long)q_hi);
    bool ok = i < q_hi && i < Q.stored;
    fx_match mi;
    float4 kq, kt;
    if (ok) {
      mi = m[i];
      ok = mi.pair == p && mi.train_row >= 0 && (uint32_t)mi.train_row < T.stored && (mi.flags & A.require_flags) == A.require_flags;
    }
    if (ok) {
      kq = Q.kp[i], kt = T.kp[mi.train_row];
      ok = finite3(kq) && finite3(kt);
    }
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
    if (ok && slot < FXR_MAX_CORR) {
      s_xy[slot] = make_float4(kq.x, kq.y, kt.x, kt.y);
      s_z[slot] = make_float2(kq.z, kt.z);
      s_d2[slot] = __float_as_uint(mi.dist2);
      s_row[slot] = i;
    }
    found += all;
    __syncthreads();  // (s_wave is written again next round)
  }
  const uint32_t n_corr = min(found, FXR_MAX_CORR);
  uint32_t flags = found > FXR_MAX_CORR ? FX_REG_TRUNCATED : 0u;
  const uint32_t H = min(n_corr, A.hyp_corr);

  // ---- rank the pool: correspondence i has rank #{j : (d2_j, j) < (d2_i, i)} (rows ascend with i); ranks below H are the pool
  for (uint32_t i = tid; i < n_corr; i += FXR_WG) {
    const uint32_t di = s_d2[i];
    uint32_t rank = 0u;
    for (uint32_t j = 0; j < n_corr && rank < H; ++j) {
      const uint32_t dj = s_d2[j];
      rank += (dj < di || (dj == di && j < i)) ? 1u : 0u;
    }
    if (rank < H) s_pool[rank] = i;
  }
  __syncthreads();

  // ---- hypotheses: key = count << 13 | (8191 - sample), the maximum wins: most agreeing, then the lowest sample
  const float mb2 = A.min_baseline * A.min_baseline, gate = 2.0f * A.inlier_dist, id2 = A.inlier_dist * A.inlier_dist;
  const uint32_t n_samples = H * (H - (H ? 1u : 0u)) / 2u;
  uint32_t best = 0u;
  for (uint32_t idx = tid; idx < n_samples; idx += FXR_WG) {
    uint32_t a, b;
    sample_ranks(idx, H, a, b);
    Hyp<float> h;
    if (!hypothesis(s_xy[s_pool[a]], s_xy[s_pool[b]], mb2, gate, h)) continue;
    uint32_t count = 0u;
    for (uint32_t i = 0; i < n_corr; ++i) count += agrees(h, s_xy[i], id2) ? 1u : 0u;
    if (count >= 2u) best = max(best, (count << FXR_IDX_BITS) | (((1u << FXR_IDX_BITS) - 1u) - idx));
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o, 64));
  __syncthreads();  // (s_d2's readers are done: it becomes the flag array)
  if (lane == 0u) s_wave[wave] = best;
  __syncthreads();
  best = max(max(s_wave[0], s_wave[1]), max(s_wave[2], s_wave[3]));

  fx_registration *out = reinterpret_cast<fx_registration *>(A.out) + p;
  if (!best) {  // (uniform) fewer than 2 correspondences, or no sample passed the gates with 2 agreeing
    if (tid == 0u) {
      fx_registration r;
      r.c = 1.0, r.s = 0.0, r.tx = 0.0, r.ty = 0.0, r.tz = 0.0;
      r.rms = INFINITY;
      r.n_corr = n_corr, r.n_inliers = 0u, r.flags = flags | FX_REG_NO_HYPOTHESIS;
      r.hyp_a = r.hyp_b = 0xffffffffu;
      *out = r;
    }
    return;
  }

  // ---- the winner's agreeing set (bit 0), again in fp32: the same operations give the same bits
  uint32_t wa, wb;
  sample_ranks(((1u << FXR_IDX_BITS) - 1u) - (best & ((1u << FXR_IDX_BITS) - 1u)), H, wa, wb);
  const uint32_t n0 = best >> FXR_IDX_BITS;
  Hyp<float> h0;
  (void)hypothesis(s_xy[s_pool[wa]], s_xy[s_pool[wb]], mb2, gate, h0);
  for (uint32_t i = tid; i < n_corr; i += FXR_WG) s_d2[i] = agrees(h0, s_xy[i], id2) ? 1u : 0u;
  __syncthreads();
  if (tid == 0u) {
    Fit f;
    f.c = (double)h0.c, f.s = (double)h0.s;
    fit_set(s_xy, s_d2, n_corr, 1u, n0, f);
    s_fit = f;
  }
  __syncthreads();
  // ---- the set the first fit agrees with (bit 1), fp64
  const double id2d = (double)A.inlier_dist * (double)A.inlier_dist;
  {
    const Fit f = s_fit;
    for (uint32_t i = tid; i < n_corr; i += FXR_WG) s_d2[i] |= residual2(f, s_xy[i]) <= id2d ? 2u : 0u;
  }
  __syncthreads();
  if (tid == 0u) {
    Fit f = s_fit;
    uint32_t n1 = 0u;
    for (uint32_t i = 0; i < n_corr; ++i) n1 += (s_d2[i] >> 1) & 1u;
    uint32_t bit = 1u, n = n0;
    if (n1 >= 2u) {
      bit = 2u, n = n1;
      fit_set(s_xy, s_d2, n_corr, bit, n, f);
    }
    double sz = 0.0, sr = 0.0;
    for (uint32_t i = 0; i < n_corr; ++i)
      if (s_d2[i] & bit) {
        const float2 z = s_z[i];
        sz += ((double)z.y - (double)z.x);
        sr += residual2(f, s_xy[i]);
      }
    fx_registration r;
    r.c = f.c, r.s = f.s, r.tx = f.tx, r.ty = f.ty, r.tz = sz / (double)n;
    r.rms = (float)sqrt(sr / (double)n);
    r.n_corr = n_corr, r.n_inliers = n, r.flags = flags | (n >= A.min_inliers ? FX_REG_VALID : 0u);
    r.hyp_a = s_row[s_pool[wa]], r.hyp_b = s_row[s_pool[wb]];
    *out = r;
    s_final = bit;
  }
  __syncthreads();
  if (A.inlier) {
    const uint32_t bit = s_final;
    for (uint32_t i = tid; i < n_corr; i += FXR_WG)
      if (s_d2[i] & bit) A.inlier[s_row[i]] = 1u;
  }
}

extern "C" hipError_t fxk_register(hipStream_t s, const FxRegisterArgs &A, uint32_t n_pairs) {
  if (A.inlier && A.q_max_rows) hipLaunchKernelGGL(k_register_init, dim3((A.q_max_rows + 255u) / 256u), dim3(256), 0, s, A.inlier, A.q_max_rows);
  if (n_pairs) hipLaunchKernelGGL(k_register, dim3(n_pairs), dim3(FXR_WG), 0, s, A);
  return hipGetLastError();
}
