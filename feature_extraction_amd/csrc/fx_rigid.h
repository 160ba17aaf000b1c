// fx_rigid.h — a rigid motion of the plane with a lift (c, s, tx, ty, tz) in fp64 and include/fx.h's "Interpolated transform"
// (fx_map_close_loop): the one statement on the device, for the loop's landmarks, last_pose and poses (csrc/fx_map_loop.hip) and
// for the rows fx_deskew_keypoint_block moves (csrc/fx_deskew.hip).  An ordered chain of + - * / sqrt on one lane (the build's
// -ffp-contract=off): the calls cannot drift apart.
#ifndef FX_RIGID_H_
#define FX_RIGID_H_
#include <hip/hip_runtime.h>
#include <math.h>

namespace fxa {
struct Rigid {
  double c, s, tx, ty, tz;
};
// include/fx.h "Interpolated transform": the one statement on the device, for the landmarks, last_pose and the poses.  alpha in (0, 1]
__device__ __forceinline__ Rigid loop_transform(const Rigid &T, double px, double py, double alpha) {
  if (alpha == 1.0) return T;
  const double cu = (1.0 - alpha) + alpha * T.c, su = alpha * T.s;
  const double nrm = sqrt(cu * cu + su * su);
  Rigid o;
  o.c = cu / nrm, o.s = su / nrm;
  const double gx = (T.c * px - T.s * py) + T.tx, gy = (T.s * px + T.c * py) + T.ty;
  const double hx = px + alpha * (gx - px), hy = py + alpha * (gy - py);
  o.tx = hx - (o.c * px - o.s * py);
  o.ty = hy - (o.s * px + o.c * py);
  o.tz = alpha * T.tz;
  return o;
}
}  // namespace fxa
#endif
