// fx_deskew.hip — the keypoints of a block moved by the sensor's own motion between the moment each was swept and the moment the
// scan is stamped (include/fx.h fx_deskew_keypoint_block): a block of the same layout comes out, and every call that reads a
// keypoint block takes it unchanged.
//
// One launch behind a memset of the n_scans records.  k_deskew is flat and grid-stride, a lane a 16-byte row OF THE BLOCK (row 0,
// the kp_offset and flag rows, then the max_total rows of the keypoint area), and the lanes g < n_scans also write record g's
// flags and motion:
//   a row of the keypoint area finds its scan through csrc/fx_scan_query.h's scan_of_row and re-derives the scan's choice of a
//   motion from at most two records (scan_motion); a finite row of a MOVED scan with w != 0 is written through the correction,
//   counts itself in rows_moved and offers its shift to max_shift; every other row of the block is copied as the four words it is.
// In place (dst == src) a copied row is not written at all: every lane then writes nothing but its own row, and the words other
// lanes read (row 0, kp_offset) are written by nobody.
// Every fp64 value is an ordered chain of + - * / sqrt floor on one lane (the build's -ffp-contract=off), the interpolated motion
// is csrc/fx_rigid.h's loop_transform, the turn's polynomial is include/fx.h's FX_DESKEW_TURN_K.  The two reductions are 32-bit
// integer atomics (a sum, and a maximum on the bit pattern of a float that is never negative): order-free, the same bytes from
// run to run.
// Every index is bounded by the layout the caller gave, whatever the block's header and offsets hold: S <= max_scans and
// S <= n_scans bound the offsets and the records read, the grid bounds the rows.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fx_device.h"
#include "fx_launch.h"
#include "fx_rigid.h"
#include "fx_scan_query.h"
#include "../../include/fx.h"

#define FXD_WG 256
#define FXD_NONE 0xffffffffu

static_assert(sizeof(fx_deskew_scan) == 16 && sizeof(fx_deskew_options) == 40 && sizeof(fx_registration) == 64, "include/fx.h");

using fxa::Rigid;

namespace {
// include/fx.h "Usable motion"
__device__ __forceinline__ bool usable(const fx_registration &R, uint32_t require_flags) {
  return (R.flags & require_flags) == require_flags && isfinite(R.c) && isfinite(R.s) && isfinite(R.tx) && isfinite(R.ty) && isfinite(R.tz) &&
         R.c > 0.0;
}
// "The motion of scan b" < S: the record's index and the scan's flags; FXD_NONE with FX_DESKEW_NO_MOTION
__device__ __forceinline__ uint32_t scan_motion(const FxDeskewArgs &A, uint32_t S, uint32_t b, uint32_t &flags) {
  const fx_registration *m = reinterpret_cast<const fx_registration *>(A.motions);
  flags = FX_DESKEW_MOVED;
  if (A.source == FX_DESKEW_PER_SCAN) {
    if (usable(m[b], A.require_flags)) return b;
  } else {
    if (b >= 1u && usable(m[b - 1u], A.require_flags)) return b - 1u;
    flags |= FX_DESKEW_NEXT_LINK;
    if (b + 1u < S && usable(m[b], A.require_flags)) return b;
  }
  flags = FX_DESKEW_NO_MOTION;
  return FXD_NONE;
}
// "Turn of a row": atan2(y, x) in turns by the odd polynomial FX_DESKEW_TURN_K on the first octant
__device__ __forceinline__ double turn_of(double x, double y) {
  const double k[6] = FX_DESKEW_TURN_K;
  const double ax = fabs(x), ay = fabs(y);
  const double hi = ay > ax ? ay : ax, lo = ay > ax ? ax : ay;
  if (!(hi > 0.0)) return 0.0;
  const double a = lo / hi, t = a * a;
  const double g = a * (k[0] + t * (k[1] + t * (k[2] + t * (k[3] + t * (k[4] + t * k[5])))));
  const double q = ay > ax ? 0.25 - g : g;
  const double h = x < 0.0 ? 0.5 - q : q;
  return y < 0.0 ? -h : h;
}
// "Sweep fraction": the signed share a of a scan period between the row's capture and the scan's stamp
__device__ __forceinline__ double sweep_share(const FxDeskewArgs &A, double x, double y) {
  const double u = A.direction * (turn_of(x, y) - A.start_turn);
  double phi = u - floor(u);
  if (phi >= 1.0) phi = 0.0;
  return (phi - A.ref_fraction) * A.sweep_fraction;
}
}  // namespace

extern "C" __global__ __launch_bounds__(FXD_WG) void k_deskew(FxDeskewArgs A) {
  const uint32_t first = kp_block_first_row(A.max_scans);
  const size_t n_rows = (size_t)first + A.max_total, n = max(n_rows, (size_t)A.n_scans);
  const uint32_t S = min(min(A.n_scans, A.src[0]), A.max_scans), rows = min(A.src[1], A.max_total);
  const uint32_t *off = kp_block_offsets(A.src);
  const fx_registration *m = reinterpret_cast<const fx_registration *>(A.motions);
  const uint4 *sv = reinterpret_cast<const uint4 *>(A.src);
  uint4 *dv = reinterpret_cast<uint4 *>(A.dst);
  fx_deskew_scan *out = reinterpret_cast<fx_deskew_scan *>(A.out);
  const bool in_place = A.dst == A.src;
  for (size_t g = (size_t)blockIdx.x * FXD_WG + threadIdx.x; g < n; g += (size_t)gridDim.x * FXD_WG) {
    if (g < A.n_scans) {  // record g: its flags and its motion (rows_moved and max_shift: the memset, then the rows' atomics)
      const uint32_t b = (uint32_t)g;
      uint32_t flags = FX_DESKEW_NO_SCAN, motion = FXD_NONE;
      if (b < S) motion = scan_motion(A, S, b, flags);
      out[b].flags = flags, out[b].motion = motion;
    }
    if (g >= n_rows) continue;
    const uint4 v = sv[g];
    uint4 o = v;
    bool moved = false;
    uint32_t b = 0u;
    if (g >= first && g - first < rows && S && scan_of_row(off, S, (uint32_t)(g - first), b)) {
      const float xf = __uint_as_float(v.x), yf = __uint_as_float(v.y), zf = __uint_as_float(v.z);
      uint32_t flags;
      const uint32_t p = isfinite(xf) && isfinite(yf) && isfinite(zf) ? scan_motion(A, S, b, flags) : FXD_NONE;
      if (p != FXD_NONE) {
        const double x = (double)xf, y = (double)yf, z = (double)zf;
        const double a = sweep_share(A, x, y), w = fabs(a);
        if (w != 0.0) {  // "Correction"
          const fx_registration &M = m[p];
          Rigid G;
          G.c = M.c, G.s = M.s, G.tx = M.tx, G.ty = M.ty, G.tz = M.tz;
          if (a < 0.0) {  // (the row was swept after the stamp: M's inverse)
            G.s = -M.s;
            G.tx = -(M.c * M.tx + M.s * M.ty);
            G.ty = (M.s * M.tx - M.c * M.ty);
            G.tz = -M.tz;
          }
          const Rigid T = fxa::loop_transform(G, 0.0, 0.0, w);
          const float xo = (float)((T.c * x - T.s * y) + T.tx), yo = (float)((T.s * x + T.c * y) + T.ty), zo = (float)(z + T.tz);
          o = make_uint4(__float_as_uint(xo), __float_as_uint(yo), __float_as_uint(zo), v.w);
          moved = true;
          const double dx = (double)xo - x, dy = (double)yo - y;
          const float shift = (float)sqrt(dx * dx + dy * dy);
          atomicAdd(&out[b].rows_moved, 1u);
          atomicMax(reinterpret_cast<uint32_t *>(&out[b].max_shift), __float_as_uint(shift));
        }
      }
    }
    if (moved || !in_place) dv[g] = o;
  }
}

extern "C" hipError_t fxk_deskew(hipStream_t s, const FxDeskewArgs &A, uint32_t max_grid) {
  const size_t n_rows = (size_t)kp_block_first_row(A.max_scans) + A.max_total, n = n_rows > A.n_scans ? n_rows : A.n_scans;
  size_t grid = (n + FXD_WG - 1u) / FXD_WG;
  grid = grid < 1u ? 1u : grid > max_grid ? max_grid : grid;
  const hipError_t e = hipMemsetAsync(A.out, 0, (size_t)A.n_scans * sizeof(fx_deskew_scan), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_deskew, dim3((uint32_t)grid), dim3(FXD_WG), 0, s, A);
  return hipGetLastError();
}
