// gnc_pose.hpp -- the pose step of the GNC global registration (include/glim_amd.h "GNC"): ONE function, host and device.  gnc.hip's solve kernel
// calls it once per iteration; tests/cpp/test_gnc_pose.cpp compiles it with a plain C++ compiler and runs the same statements on the CPU.
// The arithmetic rules are ransac_pose.hpp's (FP64, contraction off, sqrt and fabs only, a fixed sweep count), and so are the two rotation steps.
#pragma once
#include "ransac_pose.hpp"

namespace glim_amd {
namespace gnc_pose {

// The closed-form minimiser of sum w |t - (R s + t0)|^2 from the 16 weighted moments about the unweighted centroids cs, ct:
//   W = sum w, a = sum w p, b = sum w q, M[3 i + j] = sum w p_i q_j          (p = s - cs, q = t - ct)
//   H = M - a b^T / W                                                         (the moments about the weighted centroids)
//   R     dof 6: ransac_pose::horn_rotation(H); dof 4: ransac_pose::yaw_rotation(H[1] - H[3], H[0] + H[4])
//   t0 = (ct + b / W) - R (cs + a / W)
// T: row-major 3 x 4 [R | t0], always written.  Returns false when W or an entry of T is not finite (W = 0 among them: the division sees to it).
GLIM_AMD_RP_HD inline bool pose_from_moments(double W, const double* a, const double* b, const double* M, const double* cs, const double* ct, int dof,
                                             double* T) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double H[9], R[9], ps[3], qs[3];
  GLIM_AMD_RP_UNROLL
  for (int i = 0; i < 3; i++) {
    GLIM_AMD_RP_UNROLL
    for (int j = 0; j < 3; j++) H[3 * i + j] = M[3 * i + j] - (a[i] * b[j]) / W;
    ps[i] = cs[i] + a[i] / W;
    qs[i] = ct[i] + b[i] / W;
  }
  if (dof == 4) {
    ransac_pose::yaw_rotation(H[1] - H[3], H[0] + H[4], R);
  } else {
    ransac_pose::horn_rotation(H, R);
  }
  bool finite = fabs(W) <= 1.7976931348623157e308;  // (false for NaN)
  GLIM_AMD_RP_UNROLL
  for (int r = 0; r < 3; r++) {
    T[4 * r] = R[3 * r], T[4 * r + 1] = R[3 * r + 1], T[4 * r + 2] = R[3 * r + 2];
    T[4 * r + 3] = qs[r] - ((R[3 * r] * ps[0] + R[3 * r + 1] * ps[1]) + R[3 * r + 2] * ps[2]);
  }
  GLIM_AMD_RP_UNROLL
  for (int i = 0; i < 12; i++) finite = finite && (fabs(T[i]) <= 1.7976931348623157e308);
  return finite;
}

}  // namespace gnc_pose
}  // namespace glim_amd
