// fx_consensus.h — the two-correspondence consensus and the closed-form refit that fx_register_matches (fp32 hypotheses over
// float keypoints, csrc/fx_register.hip) and fx_map_localize (fp64 hypotheses over world points and landmarks,
// csrc/fx_map_localize.hip) share: include/fx.h states the clauses once, this header is their one statement on the device.
// T is the type the hypothesis stage computes in, Pt the (qx, qy, tx, ty) record of a correspondence (float4 or double4); the
// refit is fp64 whatever Pt is.  Every function is an ordered chain of correctly rounded operations (the build's
// -ffp-contract=off; hipcc's correctly rounded divide and sqrt).
#ifndef FX_CONSENSUS_H_
#define FX_CONSENSUS_H_
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace fxc {
__device__ __forceinline__ float fxc_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double fxc_sqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float fxc_abs(float v) { return fabsf(v); }
__device__ __forceinline__ double fxc_abs(double v) { return fabs(v); }

template <typename T>
struct Hyp {
  T c, s, tx, ty;
};
// The transform of the sample (A, B) of (qx, qy, tx, ty) correspondences, in the header's operation order; false: gated out.
template <typename T, typename Pt>
__device__ __forceinline__ bool hypothesis(Pt A, Pt B, T mb2, T gate, Hyp<T> &h) {
  const T dqx = B.x - A.x, dqy = B.y - A.y, dtx = B.z - A.z, dty = B.w - A.w;
  const T lq2 = dqx * dqx + dqy * dqy, lt2 = dtx * dtx + dty * dty;
  if (!(lq2 >= mb2 && lt2 >= mb2)) return false;
  if (fxc_abs(fxc_sqrt(lq2) - fxc_sqrt(lt2)) > gate) return false;
  const T dot = dqx * dtx + dqy * dty, crs = dqx * dty - dqy * dtx;
  const T nrm = fxc_sqrt(dot * dot + crs * crs);
  if (!(nrm > (T)0)) return false;
  h.c = dot / nrm, h.s = crs / nrm;
  const T mqx = (A.x + B.x) * (T)0.5, mqy = (A.y + B.y) * (T)0.5, mtx = (A.z + B.z) * (T)0.5, mty = (A.w + B.w) * (T)0.5;
  h.tx = mtx - (h.c * mqx - h.s * mqy);
  h.ty = mty - (h.s * mqx + h.c * mqy);
  return true;
}
template <typename T, typename Pt>
__device__ __forceinline__ bool agrees(const Hyp<T> &h, Pt P, T id2) {
  const T rx = ((h.c * P.x - h.s * P.y) + h.tx) - P.z, ry = ((h.s * P.x + h.c * P.y) + h.ty) - P.w;
  return rx * rx + ry * ry <= id2;
}
// sample index -> pool ranks (a, b), a < b, lexicographic
__device__ __forceinline__ void sample_ranks(uint32_t idx, uint32_t H, uint32_t &a, uint32_t &b) {
  a = 0u;
  while (idx >= H - 1u - a) idx -= H - 1u - a, ++a;
  b = a + 1u + idx;
}

struct Fit {
  double c, s, tx, ty;
};
// squared xy residual of a correspondence under a transform, fp64
template <typename Pt>
__device__ __forceinline__ double residual2(const Fit &f, Pt P) {
  const double qx = (double)P.x, qy = (double)P.y;
  const double rx = ((f.c * qx - f.s * qy) + f.tx) - (double)P.z, ry = ((f.s * qx + f.c * qy) + f.ty) - (double)P.w;
  return rx * rx + ry * ry;
}
// Least-squares rotation about z + translation over the correspondences whose flag word carries `bit`, sequential in their
// order; f.c / f.s on entry are kept when the centred sums vanish.  n >= 1 members.
template <typename Pt>
__device__ void fit_set(const Pt *s_xy, const uint32_t *s_flag, uint32_t n_corr, uint32_t bit, uint32_t n, Fit &f) {
  double sqx = 0.0, sqy = 0.0, stx = 0.0, sty = 0.0;
  for (uint32_t i = 0; i < n_corr; ++i)
    if (s_flag[i] & bit) {
      const Pt P = s_xy[i];
      sqx += (double)P.x, sqy += (double)P.y, stx += (double)P.z, sty += (double)P.w;
    }
  const double dn = (double)n;
  const double qcx = sqx / dn, qcy = sqy / dn, tcx = stx / dn, tcy = sty / dn;
  double Sdot = 0.0, Scrs = 0.0;
  for (uint32_t i = 0; i < n_corr; ++i)
    if (s_flag[i] & bit) {
      const Pt P = s_xy[i];
      const double ux = (double)P.x - qcx, uy = (double)P.y - qcy, vx = (double)P.z - tcx, vy = (double)P.w - tcy;
      Sdot += (ux * vx + uy * vy);
      Scrs += (ux * vy - uy * vx);
    }
  const double nrm = sqrt(Sdot * Sdot + Scrs * Scrs);
  if (nrm > 0.0) f.c = Sdot / nrm, f.s = Scrs / nrm;
  f.tx = tcx - (f.c * qcx - f.s * qcy);
  f.ty = tcy - (f.s * qcx + f.c * qcy);
}
}  // namespace fxc
#endif
