// fx_splice.hip — one keypoint block and one CSR block built from scans of two existing block pairs: A's selected scans, then B's,
// as fx_pack_keypoint_block and fx_pack_descriptors_csr would have written them for a batch of exactly those scans (include/fx.h
// fx_splice_blocks).
//
// Integer operations only: rows, col and val move as words and bits, offsets and row ends are re-based by subtraction.  The same
// bytes from run to run.  Every count comes from the sources' headers on the device; the grid is sized by the destination's
// layout and strides.
//
// What makes it two launches and no scan: a source's selected scans are ONE contiguous run of its keypoint rows, [r0, r0 + n), and
// while those rows exist in its CSR block they are one contiguous run of its col / val entries, [rp[r0], rp[r0 + n)).  The
// destination's offsets are the source's minus r0 (B's plus A's rows) and its row ends the source's minus rp[r0] (B's plus A's
// entries).  Whether a row is stored is a local test of its own end; the ends rise, so the rows that pass are a leading run and
// counting them is a sum.
//
// Launches, in stream order:
//   k_splice_plan  one workgroup.  One lane resolves both headers (the sentinel, the clipping, the two runs); all lanes OR the flags
//                  of the scans that will be written and count the rows that will be stored; the plan words go to the scratch.
//   k_splice_move  flat, grid-stride, a thread a 16-byte vector OF THE DESTINATION: the offset and flag sections, the keypoint rows
//                  and the zero tail, row_ptr, then col and val below nnz_stored; one lane writes the two headers.  A source run
//                  starts at any word, so a vector's four words are read as words (B's entries begin where A's end: in general
//                  not co-aligned with their source) and stored as one aligned vector; only the vector that holds the end of
//                  row_ptr, col or val is stored by words, so that no byte of a section's padding is touched.
// Every index into a source is bounded by that source's own layout whatever its header and offsets hold: a garbage block gives an
// unspecified block, never an access outside the blocks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fx_device.h"
#include "fx_launch.h"
#include "../../include/fx.h"

#define FXS_WG 256
#define FXS_PLAN_WG 1024

// The plan words.  Per source (A at 0, B at PS_WORDS):
enum {
  PS_S0 = 0,  // first selected scan
  PS_NSEL,    // selected scans
  PS_R0,      // first row of the run
  PS_NROWS,   // rows of the run
  PS_K,       // rows the source stores
  PS_EXIST,   // leading rows of the run that exist in the source's CSR block
  PS_RP0,     // the source's row_ptr[r0] (0 when no row exists)
  PS_NEED,    // entries of the existing rows
  PS_STORED,  // rows of the run the destination stores
  PS_START,   // first entry of the run in the source's col / val
  PS_LEN,     // entries to move
  PS_WORDS = 12
};
// and of the call:
enum {
  PG_NB = 2 * PS_WORDS,  // scans written: min(n, dst_max_scans)
  PG_TOTAL,              // keypoint rows written
  PG_OR,                 // row 0's flags word
  PG_ROWS,               // the CSR header's rows
  PG_NNZ,                // nnz_stored
  PG_NEEDED,             // nnz_needed
  PG_END
};
static_assert(PG_END <= FX_SPLICE_PLAN_WORDS, "fx_device.h");

__device__ __forceinline__ const uint32_t *kp_block_flags(const uint32_t *block, uint32_t max_scans) { return block + 4u + 4u * kp_block_off_rows(max_scans); }
__device__ __forceinline__ const uint32_t *csr_col(const uint32_t *block, uint32_t max_rows) { return block + 4u + csr_rp_words(max_rows); }
__device__ __forceinline__ uint32_t *csr_col(uint32_t *block, uint32_t max_rows) { return block + 4u + csr_rp_words(max_rows); }

// kp_offset[scan] of a source relative to its run, inside [0, rows of the run] whatever the block holds
__device__ __forceinline__ uint32_t run_off(const FxSpliceSrc &X, const uint32_t *ps, uint32_t scan) {
  const uint32_t o = min(kp_block_offsets(X.kp)[scan], ps[PS_K]);
  return min(max(o, ps[PS_R0]) - ps[PS_R0], ps[PS_NROWS]);
}
// kp_offset[j] of the virtual batch, j <= its scans
__device__ __forceinline__ uint64_t virt_off(const FxSpliceArgs &A, const uint32_t *p, uint32_t j) {
  const uint32_t *pa = p, *pb = p + PS_WORDS;
  if (j <= pa[PS_NSEL]) return run_off(A.a, pa, pa[PS_S0] + j);
  return (uint64_t)pa[PS_NROWS] + run_off(A.b, pb, pb[PS_S0] + (j - pa[PS_NSEL]));
}
// word i of the destination's offset section: clipped to max_total, the total beyond the batch
__device__ __forceinline__ uint32_t dst_off_word(const FxSpliceArgs &A, const uint32_t *p, uint32_t i) {
  return (uint32_t)min(virt_off(A, p, min(i, p[PG_NB])), (uint64_t)A.dst_max_total);
}
// word i of its flag section: the source's word, FX_FLAG_KP_OVERFLOW when the scan keeps fewer rows than it has, 0 beyond the batch
__device__ __forceinline__ uint32_t dst_flag_word(const FxSpliceArgs &A, const uint32_t *p, uint32_t i) {
  if (i >= p[PG_NB]) return 0u;
  const uint32_t *pa = p, *pb = p + PS_WORDS;
  const uint32_t f = i < pa[PS_NSEL] ? kp_block_flags(A.a.kp, A.a.max_scans)[pa[PS_S0] + i]
                                     : kp_block_flags(A.b.kp, A.b.max_scans)[pb[PS_S0] + (i - pa[PS_NSEL])];
  const uint64_t v0 = virt_off(A, p, i), v1 = virt_off(A, p, i + 1u), mt = A.dst_max_total;
  return f | (min(v1, mt) - min(v0, mt) < v1 - v0 ? FX_FLAG_KP_OVERFLOW : 0u);
}

// one source's header into its plan words (one lane)
__device__ void plan_source(const FxSpliceSrc &X, bool with_csr, uint32_t *ps) {
  const uint32_t S = min(X.kp[0], X.max_scans), K = min(X.kp[1], X.max_total);
  const bool last = X.scan0 == FX_SPLICE_LAST_SCAN;
  const uint32_t s0 = last ? (S ? S - 1u : 0u) : min(X.scan0, S);
  const uint32_t nsel = last && !S ? 0u : min(X.n_scans, S - s0);
  const uint32_t *off = kp_block_offsets(X.kp);
  const uint32_t r0 = min(off[s0], K), r1 = max(r0, min(off[s0 + nsel], K));  // (s0 + nsel <= S <= max_scans: inside the section)
  ps[PS_S0] = s0, ps[PS_NSEL] = nsel, ps[PS_R0] = r0, ps[PS_NROWS] = r1 - r0, ps[PS_K] = K;
  uint32_t exist = 0u, rp0 = 0u, need = 0u;
  if (with_csr) {
    const uint32_t rs = min(X.csr[3], X.max_rows);  // row r exists iff r < rows_stored
    exist = min(max(rs, r0), r1) - r0;
    if (exist) {  // (r0 < rs <= max_rows: row_ptr[r0 .. r0 + exist] are inside the section)
      rp0 = X.csr[4u + r0];
      need = X.csr[4u + r0 + exist] - rp0;
    }
  }
  ps[PS_EXIST] = exist, ps[PS_RP0] = rp0, ps[PS_NEED] = need;
  ps[PS_STORED] = ps[PS_START] = ps[PS_LEN] = 0u;
}
// the entries [row_ptr[r0], row_ptr[r0 + stored)) of a source, clipped to its capacity and to `room` entries of the destination
__device__ void plan_entries(const FxSpliceSrc &X, uint32_t room, uint32_t *ps) {
  if (!ps[PS_STORED]) return;
  const uint32_t start = min(ps[PS_RP0], X.cap), end = min(X.csr[4u + ps[PS_R0] + ps[PS_STORED]], X.cap);
  ps[PS_START] = start, ps[PS_LEN] = min(max(end, start) - start, room);
}

// this lane's share of the rows v < n of a run whose end, base + row_ptr[v + 1] - rp0, is within cap (rp: the run's row_ptr).  The
// loads of eight rounds are issued together: one workgroup does the count, and a load a round would make it a chain of latencies.
__device__ __forceinline__ uint32_t count_fit(const uint32_t *rp, uint32_t n, uint32_t rp0, uint32_t base, uint32_t cap, uint32_t tid) {
  uint32_t c = 0u;
  size_t v = tid;
  for (; v + 7u * FXS_PLAN_WG < n; v += 8u * FXS_PLAN_WG) {
    uint32_t e[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) e[j] = rp[v + j * FXS_PLAN_WG + 1u];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) c += (uint64_t)base + (e[j] - rp0) <= (uint64_t)cap ? 1u : 0u;
  }
  for (; v < n; v += FXS_PLAN_WG) c += (uint64_t)base + (rp[v + 1u] - rp0) <= (uint64_t)cap ? 1u : 0u;
  return c;
}

extern "C" __global__ __launch_bounds__(FXS_PLAN_WG) void k_splice_plan(FxSpliceArgs A) {
  __shared__ uint32_t s_p[FX_SPLICE_PLAN_WORDS], s_w[2 * (FXS_PLAN_WG / 64)], s_or;
  const uint32_t tid = threadIdx.x;
  uint32_t *pa = s_p, *pb = s_p + PS_WORDS;
  if (tid == 0) {
    for (uint32_t i = 0; i < FX_SPLICE_PLAN_WORDS; ++i) s_p[i] = 0u;
    s_or = 0u;
    plan_source(A.a, A.dst_csr != nullptr, pa);
    plan_source(A.b, A.dst_csr != nullptr, pb);
    const uint64_t n = (uint64_t)pa[PS_NSEL] + pb[PS_NSEL];
    s_p[PG_NB] = (uint32_t)min(n, (uint64_t)A.dst_max_scans);
    s_or = n > A.dst_max_scans ? FX_FLAG_KP_OVERFLOW : 0u;  // (more scans than the block has room for: cut, and said so)
    s_p[PG_ROWS] = (uint32_t)min((uint64_t)pa[PS_NROWS] + pb[PS_NROWS], (uint64_t)0xffffffffu);
    s_p[PG_NEEDED] = pa[PS_NEED] + pb[PS_NEED];
  }
  __syncthreads();
  // row 0's flags: the OR of the flag words that will be written
  uint32_t acc = 0u;
  for (size_t i = tid; i < s_p[PG_NB]; i += FXS_PLAN_WG) acc |= dst_flag_word(A, s_p, (uint32_t)i);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) acc |= (uint32_t)__shfl_xor((int)acc, d, 64);
  if ((tid & 63u) == 0u && acc) atomicOr(&s_or, acc);
  // the rows the destination stores: virtual row v iff every row u <= v exists in its source, u < dst_max_rows and ends within
  // dst_cap.  The ends rise, so per source the rows that pass are a leading run: count them.  B's rows follow A's: they take part
  // only when every row of A exists, and count only when every row of A passed.
  uint32_t na = 0u, nb = 0u;
  if (A.dst_csr) {
    na = count_fit(A.a.csr + 4u + pa[PS_R0], min(pa[PS_EXIST], A.dst_max_rows), pa[PS_RP0], 0u, A.dst_cap, tid);
    if (pa[PS_EXIST] == pa[PS_NROWS] && A.dst_max_rows > pa[PS_NROWS])
      nb = count_fit(A.b.csr + 4u + pb[PS_R0], min(pb[PS_EXIST], A.dst_max_rows - pa[PS_NROWS]), pb[PS_RP0], pa[PS_NEED], A.dst_cap, tid);
  }
  uint32_t ea, eb, stored_a, stored_b;
  wg_scan2<FXS_PLAN_WG / 64>(na, nb, s_w, ea, eb, stored_a, stored_b);
  if (tid == 0) {
    pa[PS_STORED] = stored_a, pb[PS_STORED] = stored_a == pa[PS_NROWS] ? stored_b : 0u;
    if (A.dst_csr) {
      plan_entries(A.a, A.dst_cap, pa);
      plan_entries(A.b, A.dst_cap - pa[PS_LEN], pb);
    }
    s_p[PG_NNZ] = pa[PS_LEN] + pb[PS_LEN];
    s_p[PG_TOTAL] = dst_off_word(A, s_p, s_p[PG_NB]);
    s_p[PG_OR] = s_or;
  }
  __syncthreads();
  if (tid < FX_SPLICE_PLAN_WORDS) A.plan[tid] = s_p[tid];
}

// four consecutive words of the run [s, s + len) that continues as [t, ...): word w < len from s, else from t
__device__ __forceinline__ uint4 gather4(const uint32_t *s, uint32_t len, const uint32_t *t, uint32_t w) {
  uint32_t x[4];
  if (w + 3u < len || w >= len) {
    const uint32_t *q = w >= len ? t + (w - len) : s + w;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) x[j] = q[j];
  } else {  // (the seam: A's last words and B's first)
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) x[j] = w + j < len ? s[w + j] : t[w + j - len];
  }
  return make_uint4(x[0], x[1], x[2], x[3]);
}

extern "C" __global__ __launch_bounds__(FXS_WG) void k_splice_move(FxSpliceArgs A) {
  const uint32_t *p = A.plan, *pa = p, *pb = p + PS_WORDS;
  const size_t g = (size_t)blockIdx.x * FXS_WG + threadIdx.x, gs = (size_t)gridDim.x * FXS_WG;
  const uint32_t off_rows = kp_block_off_rows(A.dst_max_scans), flag_rows = kp_block_flag_rows(A.dst_max_scans);
  uint4 *dv = reinterpret_cast<uint4 *>(A.dst_kp);
  // the offset and the flag section, padding words included (as the pack writes them)
  for (size_t q = g; q < (size_t)off_rows + flag_rows; q += gs) {
    uint32_t x[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
      x[j] = q < off_rows ? dst_off_word(A, p, 4u * (uint32_t)q + j) : dst_flag_word(A, p, 4u * (uint32_t)(q - off_rows) + j);
    dv[1u + q] = make_uint4(x[0], x[1], x[2], x[3]);
  }
  // the keypoint rows: A's run, B's run, zeros
  {
    const uint4 *ra = kp_block_rows<uint4>(A.a.kp, A.a.max_scans) + pa[PS_R0], *rb = kp_block_rows<uint4>(A.b.kp, A.b.max_scans) + pb[PS_R0];
    uint4 *rows = dv + kp_block_first_row(A.dst_max_scans);
    const uint32_t total = p[PG_TOTAL], n_a = pa[PS_NROWS];  // (total <= A's rows + B's rows)
    for (size_t k = g; k < A.dst_max_total; k += gs) rows[k] = k >= total ? make_uint4(0u, 0u, 0u, 0u) : k < n_a ? ra[k] : rb[k - n_a];
  }
  if (g == 0) dv[0] = make_uint4(p[PG_NB], p[PG_TOTAL], p[PG_OR], A.dst_max_total);
  if (!A.dst_csr) return;
  // row_ptr[0 .. dst_max_rows]: 0, the stored rows' ends re-based, then nnz_stored
  {
    const uint32_t *rpa = A.a.csr + 4u + pa[PS_R0], *rpb = A.b.csr + 4u + pb[PS_R0];
    const uint32_t sa = pa[PS_STORED], ns = sa + pb[PS_STORED], nnz = p[PG_NNZ];
    uint32_t *rp = A.dst_csr + 4u;
    const size_t n_rp = (size_t)A.dst_max_rows + 1u;
    for (size_t q = g; 4u * q < n_rp; q += gs) {
      uint32_t x[4];
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const size_t r = 4u * q + j;
        x[j] = r == 0u ? 0u : r > ns ? nnz : r <= sa ? rpa[r] - pa[PS_RP0] : pa[PS_NEED] + (rpb[r - sa] - pb[PS_RP0]);
      }
      if (4u * q + 3u < n_rp) {
        reinterpret_cast<uint4 *>(rp)[q] = make_uint4(x[0], x[1], x[2], x[3]);
      } else {
        for (uint32_t j = 0; 4u * q + j < n_rp; ++j) rp[4u * q + j] = x[j];
      }
    }
  }
  if (g == 0) reinterpret_cast<uint4 *>(A.dst_csr)[0] = make_uint4(p[PG_ROWS], p[PG_NNZ], p[PG_NEEDED], pa[PS_STORED] + pb[PS_STORED]);
  // col, then val: the entries below nnz_stored
  {
    const uint32_t nnz = p[PG_NNZ], la = pa[PS_LEN];
    const size_t nv = ((size_t)nnz + 3u) / 4u;
    const uint32_t *ca = csr_col(A.a.csr, A.a.max_rows) + pa[PS_START], *cb = csr_col(A.b.csr, A.b.max_rows) + pb[PS_START];
    const uint32_t *va = ca + csr_cap_words(A.a.cap), *vb = cb + csr_cap_words(A.b.cap);
    uint32_t *col = csr_col(A.dst_csr, A.dst_max_rows), *val = col + csr_cap_words(A.dst_cap);
    for (size_t q = g; q < 2u * nv; q += gs) {
      const bool v = q >= nv;
      const uint32_t w = 4u * (uint32_t)(v ? q - nv : q);
      uint32_t *d = (v ? val : col) + w;
      if (w + 3u < nnz) {
        *reinterpret_cast<uint4 *>(d) = gather4(v ? va : ca, la, v ? vb : cb, w);
      } else {  // (the last vector: by words, nothing at or beyond nnz_stored)
        for (uint32_t j = 0; w + j < nnz; ++j) d[j] = w + j < la ? (v ? va : ca)[w + j] : (v ? vb : cb)[w + j - la];
      }
    }
  }
}

extern "C" hipError_t fxk_splice(hipStream_t s, const FxSpliceArgs &A, uint32_t max_grid) {
  size_t vecs = (size_t)kp_block_first_row(A.dst_max_scans) + A.dst_max_total;
  if (A.dst_csr) vecs += csr_rp_words(A.dst_max_rows) / 4u + 2u * (csr_cap_words(A.dst_cap) / 4u);
  size_t grid = (vecs + FXS_WG - 1u) / FXS_WG;
  grid = grid < 1u ? 1u : grid > max_grid ? max_grid : grid;
  hipLaunchKernelGGL(k_splice_plan, dim3(1), dim3(FXS_PLAN_WG), 0, s, A);
  hipLaunchKernelGGL(k_splice_move, dim3((uint32_t)grid), dim3(FXS_WG), 0, s, A);
  return hipGetLastError();
}
