// fx_match.hip — descriptor matching between CSR blocks across azimuth shifts (include/fx.h fx_match_descriptors_csr).
//
// d2(q, t, s) = sum over the 1980 bins c of (q[c] - t[(c + 165 s) mod 1980])^2: PCL's 3DSC draws a random azimuth reference per
// keypoint, so two descriptors of one pole differ by a rotation of the 12 azimuth sectors, a cyclic shift of the bin index
// by 165 (bin = l * 165 + k * 15 + j, l the sector).  Evaluated as |q|^2 + |t|^2 - 2 q.t_s with every sum in fp64 over the
// exact fp32 x fp32 products and one rounding to fp32 at the end: within 2^-23 d2 + 2^-40 (|q|^2 + |t|^2) + 2^-150 of the exact
// value (subnormal results are kept, a value from 2^128 - 2^103 on is +inf).
// Every sum runs over a row's stored entries in their stored order, by one lane: nothing depends on the launch or on what
// else runs, and identical rows give |q|^2 = |t|^2 = q.t_0 bit for bit, so their dist2 is exactly 0.
//
// Launches: k_match_norms (a thread a row: |row|^2 over the bins, NaN when the row stores a NaN or an infinity), k_match_init
// (every output record to "no match", the mutual table to all ones), k_match, and with `mutual` k_match_mutual.
//
// k_match: one workgroup per (pair, tile of 64 query rows): eight wavefronts, each taking a query row a round for up to
// eight rounds.  The query row is scattered dense into LDS TWICE back to back (q2[c] = q2[c + 1980] = q[c]; un-written
// after its round): the bin that meets train bin c under shift s is q[(c - 165 s) mod 1980] = q2[c + 165 (12 - s)], twelve
// reads at fixed offsets from one address.  The pair's train rows are
// staged in LDS as (col, val) entries, tiles of up to 64 rows / FXM_TILE_ENTRIES entries; each LANE takes one train row of
// the tile and walks its entries, accumulating the twelve dots: no reduction across lanes inside a row.  A lane keeps the
// best and the second-best row it has seen; one butterfly over the wavefront at the end picks the row's record
// (ties: lowest train row, then lowest shift).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fx_device.h"
#include "fx_launch.h"
#include "../../include/fx.h"

#define FXM_WG 512
#define FXM_NWAVE (FXM_WG / 64)
#define FXM_ROUNDS 8u                       // query rows a wavefront takes, one after the other
#define FXM_SECTOR 165u                    // bins of one azimuth sector
#define FXM_Q_WORDS (2u * FX_DESC_BINS)    // a query row in LDS, twice
#define FXM_TILE_ROWS 64u
#define FXM_TILE_ENTRIES 3072u             // >= FX_DESC_FLOATS: any one row fits
#define FXM_LDS_BYTES (FXM_NWAVE * FXM_Q_WORDS * 4u + FXM_TILE_ENTRIES * 8u + FXM_TILE_ROWS * 8u + 72u * 4u)

static_assert(sizeof(fx_match) == 32 && sizeof(fx_match_pair) == 16 && sizeof(fx_match_options) == 16, "include/fx.h");
static_assert(sizeof(FxMatchPairDev) == 32, "FxMatchPairDev");
static_assert(FXM_TILE_ENTRIES >= FX_DESC_FLOATS && (FXM_NWAVE * FXM_Q_WORDS * 4u) % 16u == 0u, "tile");

namespace {
// A CSR block's sections; rows = the rows it stores, never more than its layout has room for.
struct CsrView {
  const uint32_t *rp, *col, *val;
  uint32_t rows, cap;
  // row r's entries [e0, e1), held inside the block whatever row_ptr says
  __device__ __forceinline__ uint32_t begin(uint32_t r) const { return min(rp[r], cap); }
};
__device__ __forceinline__ CsrView csr_view(const uint32_t *block, uint32_t max_rows, uint32_t cap) {
  CsrView v;
  v.rp = block + 4;
  v.col = v.rp + csr_rp_words(max_rows);
  v.val = v.col + csr_cap_words(cap);
  v.rows = min(block[3], max_rows);
  v.cap = cap;
  return v;
}
// (d, row) order of candidates; row < 0: none
__device__ __forceinline__ bool cand_less(float da, int32_t ra, float db, int32_t rb) {
  if (ra < 0) return false;
  if (rb < 0) return true;
  return da < db || (da == db && ra < rb);
}
// LDS written by some lanes of a wavefront, read by others of the same wavefront
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
}  // namespace

extern "C" __global__ __launch_bounds__(256) void k_match_norms(const uint32_t *block, uint32_t max_rows, uint32_t cap, double *norm) {
  const CsrView V = csr_view(block, max_rows, cap);
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= V.rows) return;
  const uint32_t e0 = V.begin(r), e1 = max(V.begin(r + 1u), e0);
  double a = 0.0;
  bool nan = false;
  for (uint32_t e = e0; e < e1; ++e) {
    const float v = __uint_as_float(V.val[e]);
    nan = nan || !(fabsf(v) < INFINITY);  // NaN, +Inf, -Inf
    if (V.col[e] < FX_DESC_BINS) {
      const double d = (double)v;
      a += d * d;
    }
  }
  norm[r] = nan ? (double)NAN : a;
}

extern "C" __global__ __launch_bounds__(256) void k_match_init(fx_match *out, uint32_t q_max_rows, unsigned long long *mut, uint32_t mut_n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < q_max_rows) {
    fx_match m;
    m.train_row = -1, m.shift = 0u, m.dist2 = INFINITY, m.second_row = -1, m.dist2_second = INFINITY, m.flags = 0u;
    m.pair = 0xffffffffu, m.reserved = 0u;
    out[i] = m;
  }
  if (i < mut_n) mut[i] = ~0ull;
}

template <int NS>
__global__ __launch_bounds__(FXM_WG) void k_match(FxMatchArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  float *s_q = reinterpret_cast<float *>(smem) + wave * FXM_Q_WORDS;
  uint2 *s_ent = reinterpret_cast<uint2 *>(smem + FXM_NWAVE * FXM_Q_WORDS * 4u);
  double *s_tn = reinterpret_cast<double *>(s_ent + FXM_TILE_ENTRIES);
  uint32_t *s_rp = reinterpret_cast<uint32_t *>(s_tn + FXM_TILE_ROWS);  // [65] entry offsets of the tile's rows, [66] rows, [67] first entry

  const uint2 item = A.items[blockIdx.x];
  const FxMatchPairDev pr = A.pairs[item.x];
  const CsrView Q = csr_view(A.q_block, A.q_max_rows, A.q_cap), T = csr_view(A.t_block, A.t_max_rows, A.t_cap);
  uint32_t q_lo, q_end, t_lo, t_end;
  clip_range(pr.q_row0, pr.q_rows, Q.rows, q_lo, q_end);
  clip_range(pr.t_row0, pr.t_rows, T.rows, t_lo, t_end);
  const unsigned long long q_first = (unsigned long long)q_lo + (unsigned long long)item.y * (FXM_NWAVE * FXM_ROUNDS);
  if (q_first >= q_end) return;  // (the work list is built from the ranges before they are clipped)
  for (uint32_t i = lane; i < FXM_Q_WORDS / 4u; i += 64u) reinterpret_cast<float4 *>(s_q)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  wave_lds_sync();

  // A pair whose train rows fit one tile (the usual case: a scan's few dozen keypoints) stages them once; the wavefronts then
  // run their rounds without meeting again.  Otherwise every round walks the tiles, all wavefronts together.
  bool staged_all = false;
  for (uint32_t round = 0; round < FXM_ROUNDS; ++round) {
    const unsigned long long q_round = q_first + (unsigned long long)round * FXM_NWAVE;
    if (q_round >= q_end) break;  // (uniform)
    const bool active = q_round + wave < q_end;
    const uint32_t qr = (uint32_t)q_round + wave;
    double qn = (double)NAN;
    uint32_t qe0 = 0u, qe1 = 0u;
    if (active) {
      qn = A.q_norm[qr];
      qe0 = Q.begin(qr), qe1 = max(Q.begin(qr + 1u), qe0);
      for (uint32_t e = qe0 + lane; e < qe1; e += 64u) {
        const uint32_t c = Q.col[e];
        if (c < FX_DESC_BINS) s_q[c] = s_q[c + FX_DESC_BINS] = __uint_as_float(Q.val[e]);
      }
    }
    wave_lds_sync();
    const bool live = active && qn == qn;  // (a row that stores a non-finite word never matches)

    float b_d = INFINITY, c_d = INFINITY;  // this lane's best and second-best train row so far
    int32_t b_row = -1, c_row = -1;
    uint32_t b_s = 0u;
    for (uint32_t r0 = t_lo; r0 < t_end;) {
      if (!staged_all) {
        __syncthreads();  // (the previous tile's readers)
        if (wave == 0u) {
          const uint32_t base = T.begin(r0), r = r0 + lane;
          uint32_t rel = 0u;
          bool fits = false;
          if (r < t_end) {
            rel = max(T.begin(r + 1u), base) - base;
            fits = rel <= FXM_TILE_ENTRIES;
            s_tn[lane] = A.t_norm[r];
          }
          const unsigned long long m = __ballot(fits);
          const uint32_t n = max(1u, (uint32_t)__ffsll((long long)~m) - 1u);  // the leading run of rows that fit (64 when all do)
          s_rp[lane + 1u] = min(rel, FXM_TILE_ENTRIES);
          if (lane == 0u) s_rp[0] = 0u, s_rp[66] = min(n, FXM_TILE_ROWS), s_rp[67] = base;
        }
        __syncthreads();
        const uint32_t n = s_rp[66], base = s_rp[67], cnt = s_rp[n];
        for (uint32_t i = tid; i < cnt; i += FXM_WG) s_ent[i] = make_uint2(T.col[base + i], T.val[base + i]);
        __syncthreads();
        staged_all = r0 == t_lo && r0 + n >= t_end;
      }
      const uint32_t n = s_rp[66];
      if (live && lane < n) {
        const double tn = s_tn[lane];
        if (tn == tn) {
          double dot[NS];
#pragma unroll
          for (int s = 0; s < NS; ++s) dot[s] = 0.0;
          const uint32_t e1 = s_rp[lane + 1u];
          for (uint32_t e = s_rp[lane]; e < e1; ++e) {
            const uint2 en = s_ent[e];
            if (en.x < FX_DESC_BINS) {
              const double v = (double)__uint_as_float(en.y);
              const float *p = s_q + en.x;
              // (fma: the product of two fp32 values is exact in fp64, so this is the sum k_match_norms forms with mul + add)
#pragma unroll
              for (int s = 0; s < NS; ++s) dot[s] = fma(v, (double)p[FXM_SECTOR * (12u - (uint32_t)s)], dot[s]);
            }
          }
          const double sum = qn + tn;
          float f = 0.f;
          uint32_t fs = 0u;
#pragma unroll
          for (int s = 0; s < NS; ++s) {
            const double d = sum - 2.0 * dot[s];
            const float g = (float)(d > 0.0 ? d : 0.0);
            if (s == 0 || g < f) f = g, fs = (uint32_t)s;
          }
          const int32_t row = (int32_t)(r0 + lane);
          if (A.mutual) atomicMin(&A.mut[pr.mut_off + (r0 + lane - t_lo)], ((unsigned long long)__float_as_uint(f) << 32) | qr);
          if (b_row < 0 || f < b_d) {  // (a lane's rows come in rising order: a tie keeps the lower row)
            c_d = b_d, c_row = b_row;
            b_d = f, b_row = row, b_s = fs;
          } else if (c_row < 0 || f < c_d) {
            c_d = f, c_row = row;
          }
        }
      }
      r0 += n;
    }
    if (!active) continue;
    // the row's best over the wavefront, then the best of what is left without that train row
    float g_d = b_d;
    int32_t g_row = b_row;
    uint32_t g_s = b_s;
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const float od = __shfl_xor(g_d, o, 64);
      const int32_t orow = __shfl_xor(g_row, o, 64);
      const uint32_t os = (uint32_t)__shfl_xor((int)g_s, o, 64);
      if (cand_less(od, orow, g_d, g_row)) g_d = od, g_row = orow, g_s = os;
    }
    float h_d = b_row == g_row ? c_d : b_d;
    int32_t h_row = b_row == g_row ? c_row : b_row;
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const float od = __shfl_xor(h_d, o, 64);
      const int32_t orow = __shfl_xor(h_row, o, 64);
      if (cand_less(od, orow, h_d, h_row)) h_d = od, h_row = orow;
    }
    if (lane == 0u) {
      fx_match m;
      m.train_row = g_row, m.shift = g_row >= 0 ? g_s : 0u, m.dist2 = g_row >= 0 ? g_d : INFINITY;
      m.second_row = h_row, m.dist2_second = h_row >= 0 ? h_d : INFINITY;
      bool ok = g_row >= 0 && m.dist2 <= A.max_dist2;
      if (ok && A.max_ratio < 1.f) ok = m.dist2 <= (A.max_ratio * A.max_ratio) * m.dist2_second;
      m.flags = ok ? 0x1u : 0u;
      m.pair = item.x, m.reserved = 0u;
      reinterpret_cast<fx_match *>(A.out)[qr] = m;
    }
    // un-write the query row: the array is all zeros again for the next round
    for (uint32_t e = qe0 + lane; e < qe1; e += 64u) {
      const uint32_t c = Q.col[e];
      if (c < FX_DESC_BINS) s_q[c] = s_q[c + FX_DESC_BINS] = 0.f;
    }
    wave_lds_sync();
  }
}

// FX_MATCH_MUTUAL: the query row is the minimiser of (dist2, query row) its train row saw
extern "C" __global__ __launch_bounds__(256) void k_match_mutual(FxMatchArgs A) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= A.q_max_rows) return;
  fx_match *out = reinterpret_cast<fx_match *>(A.out);
  const fx_match m = out[i];
  if (m.pair == 0xffffffffu || m.train_row < 0) return;
  const FxMatchPairDev pr = A.pairs[m.pair];
  uint32_t t_lo, t_end;
  clip_range(pr.t_row0, pr.t_rows, min(A.t_block[3], A.t_max_rows), t_lo, t_end);
  const uint32_t t = (uint32_t)m.train_row;
  if (t < t_lo || t >= t_end) return;
  if (A.mut[pr.mut_off + (t - t_lo)] == (((unsigned long long)__float_as_uint(m.dist2) << 32) | i)) out[i].flags = m.flags | 0x2u;
}

extern "C" {
// norms: the query block's at A.q_norm, the train block's at A.t_norm (one pass when they are the same array)
hipError_t fxk_match(hipStream_t s, const FxMatchArgs &A, uint32_t n_items, uint32_t mut_n, uint32_t shifts) {
  hipError_t e = hipFuncSetAttribute((const void *)k_match<12>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FXM_LDS_BYTES);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void *)k_match<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FXM_LDS_BYTES);
  if (e != hipSuccess) return e;
  if (A.q_max_rows)
    hipLaunchKernelGGL(k_match_norms, dim3((A.q_max_rows + 255u) / 256u), dim3(256), 0, s, A.q_block, A.q_max_rows, A.q_cap,
                       const_cast<double *>(A.q_norm));
  if (A.t_norm != A.q_norm && A.t_max_rows)
    hipLaunchKernelGGL(k_match_norms, dim3((A.t_max_rows + 255u) / 256u), dim3(256), 0, s, A.t_block, A.t_max_rows, A.t_cap,
                       const_cast<double *>(A.t_norm));
  const uint32_t n_init = A.q_max_rows > mut_n ? A.q_max_rows : mut_n;
  if (n_init)
    hipLaunchKernelGGL(k_match_init, dim3((n_init + 255u) / 256u), dim3(256), 0, s, reinterpret_cast<fx_match *>(A.out), A.q_max_rows, A.mut,
                       mut_n);
  if (n_items) {
    if (shifts == 1u)
      hipLaunchKernelGGL(k_match<1>, dim3(n_items), dim3(FXM_WG), FXM_LDS_BYTES, s, A);
    else
      hipLaunchKernelGGL(k_match<12>, dim3(n_items), dim3(FXM_WG), FXM_LDS_BYTES, s, A);
    if (A.mutual) hipLaunchKernelGGL(k_match_mutual, dim3((A.q_max_rows + 255u) / 256u), dim3(256), 0, s, A);
  }
  return hipGetLastError();
}
uint32_t fxk_match_tile_rows(void) { return FXM_NWAVE * FXM_ROUNDS; }
}  // extern "C"
