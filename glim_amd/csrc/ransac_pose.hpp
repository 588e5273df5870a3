// ransac_pose.hpp -- the three-point pose solver of the RANSAC global registration (include/glim_amd.h "RANSAC"): ONE function, host and
// device.  ransac.hip's hypothesis kernel calls it with one lane per hypothesis; tests/cpp/test_ransac_pose.cpp compiles it with a plain C++
// compiler and runs the same statements on the CPU.  Its two rotation steps (yaw_rotation, horn_rotation) are functions of their own because the GNC
// pose step (gnc_pose.hpp) takes the same ones.  The header includes nothing of the project.
//
// Every floating-point statement is FP64 with contraction off and the fused operations written out (fma); the only library functions are sqrt
// and fabs (correctly rounded everywhere), no trigonometry: the 4-DoF rotation is (cos, sin) = (C, S) / sqrt(C^2 + S^2), which is the rotation
// by yaw = atan2(S, C) without ever forming the angle.  There is no data-dependent loop exit (the Jacobi iteration runs a fixed number of
// sweeps), so the statements executed do not depend on the lane or on the data.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define GLIM_AMD_RP_HD __host__ __device__
#else
#define GLIM_AMD_RP_HD
#endif
#if defined(__clang__)
#define GLIM_AMD_RP_UNROLL _Pragma("unroll")
#else
#define GLIM_AMD_RP_UNROLL
#endif

namespace glim_amd {
namespace ransac_pose {

// status of a hypothesis (rules 1 and 2 are the sampler's: ransac.hip)
enum { OK = 0, NO_MATCH = 1, REPEATED = 2, EDGE_LENGTH = 3, DEGENERATE = 4 };
constexpr int JACOBI_SWEEPS = 8;           // cyclic sweeps over the six off-diagonal pairs of the 4 x 4 matrix; quadratic convergence: 5 reach FP64
constexpr double COLLINEAR_RATIO = 1e-6;   // sigma_2 < COLLINEAR_RATIO * sigma_1 of the centred source triangle: degenerate

// rotation about z by atan2(S, C), formed as (cos, sin) = (C, S) / |(C, S)|; the identity when both are 0.  R: row-major 3 x 3.
GLIM_AMD_RP_HD inline void yaw_rotation(double S, double C, double* R) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double h = sqrt(C * C + S * S);
  const double c = h > 0.0 ? C / h : 1.0, sn = h > 0.0 ? S / h : 0.0;
  R[0] = c, R[1] = -sn, R[2] = 0.0;
  R[3] = sn, R[4] = c, R[5] = 0.0;
  R[6] = 0.0, R[7] = 0.0, R[8] = 1.0;
}

// Horn 1987: the rotation that maximises sum (R a) . b for H[3 i + j] = sum a[i] b[j], as the eigenvector of the largest eigenvalue of the symmetric
// 4 x 4 matrix N(H) by JACOBI_SWEEPS cyclic Jacobi sweeps.  R: row-major 3 x 3.
GLIM_AMD_RP_HD inline void horn_rotation(const double* H, double* R) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  // N (symmetric, quaternion order w x y z)
  double N[4][4], V[4][4];
  N[0][0] = (H[0] + H[4]) + H[8];
  N[0][1] = H[5] - H[7];
  N[0][2] = H[6] - H[2];
  N[0][3] = H[1] - H[3];
  N[1][1] = (H[0] - H[4]) - H[8];
  N[1][2] = H[1] + H[3];
  N[1][3] = H[6] + H[2];
  N[2][2] = (H[4] - H[0]) - H[8];
  N[2][3] = H[5] + H[7];
  N[3][3] = (H[8] - H[0]) - H[4];
  GLIM_AMD_RP_UNROLL
  for (int i = 0; i < 4; i++) {
    GLIM_AMD_RP_UNROLL
    for (int j = 0; j < 4; j++) {
      if (j < i) N[i][j] = N[j][i];
      V[i][j] = i == j ? 1.0 : 0.0;
    }
  }
  for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
    GLIM_AMD_RP_UNROLL
    for (int p = 0; p < 3; p++) {
      GLIM_AMD_RP_UNROLL
      for (int q = p + 1; q < 4; q++) {
        // the rotation that annihilates N[p][q] (Rutishauser); the identity when it is already 0
        const double apq = N[p][q];
        const bool live = apq != 0.0;
        const double theta = live ? (N[q][q] - N[p][p]) / (2.0 * apq) : 0.0;
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double tn = live ? tt : 0.0;
        const double c = 1.0 / sqrt(tn * tn + 1.0), sn = tn * c;
        GLIM_AMD_RP_UNROLL
        for (int k = 0; k < 4; k++) {  // columns p, q
          const double kp = N[k][p], kq = N[k][q];
          N[k][p] = c * kp - sn * kq;
          N[k][q] = sn * kp + c * kq;
        }
        GLIM_AMD_RP_UNROLL
        for (int k = 0; k < 4; k++) {  // rows p, q
          const double pk = N[p][k], qk = N[q][k];
          N[p][k] = c * pk - sn * qk;
          N[q][k] = sn * pk + c * qk;
        }
        GLIM_AMD_RP_UNROLL
        for (int k = 0; k < 4; k++) {
          const double kp = V[k][p], kq = V[k][q];
          V[k][p] = c * kp - sn * kq;
          V[k][q] = sn * kp + c * kq;
        }
      }
    }
  }
  // the column of the largest diagonal entry (the first of equals), selected without indexing by a run-time value
  double best = N[0][0], qw = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
  GLIM_AMD_RP_UNROLL
  for (int j = 1; j < 4; j++) {
    const bool take = N[j][j] > best;
    best = take ? N[j][j] : best;
    qw = take ? V[0][j] : qw;
    qx = take ? V[1][j] : qx;
    qy = take ? V[2][j] : qy;
    qz = take ? V[3][j] : qz;
  }
  const double qn = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
  qw /= qn, qx /= qn, qy /= qn, qz /= qn;
  const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
  const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
  R[0] = 1.0 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
  R[3] = txy + twz, R[4] = 1.0 - (txx + tzz), R[5] = tyz - twx;
  R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1.0 - (txx + tyy);
}

// s, t: three source points and their three target points, x y z each.  T: row-major 3 x 4 [R | t] with t_k ~ R s_k + t (written on OK only).
// Returns OK, EDGE_LENGTH or DEGENERATE:
//   DEGENERATE   a coordinate is not finite (decided first: the edge-length rule is stated for finite lengths);
//   EDGE_LENGTH  for an edge (a, b) in the order (0,1), (1,2), (2,0): d_s = |s_a - s_b|, d_t = |t_a - t_b|, each sqrt((dx^2 + dy^2) + dz^2);
//                rejected unless min(d_s, d_t) >= (1 - poly_error_thresh) * max(d_s, d_t);
//   DEGENERATE   sigma_1 = 0 or sigma_2 < 1e-6 sigma_1, the singular values of the centred source triangle, in closed form:
//                sigma_1^2 + sigma_2^2 = p = sum |c_k|^2, sigma_1^2 sigma_2^2 = q = |e_1 x e_2|^2 / 3 (e = edges from s_0; the third is 0).
// dof 6: Horn's closed form, the eigenvector of the largest eigenvalue of the 4 x 4 matrix N(H), H = sum c_s c_t^T, by cyclic Jacobi.
// dof 4: rotation about z by atan2(S, C), S = sum (x_s y_t - y_s x_t), C = sum (x_s x_t + y_s y_t) over the centred pairs (identity when both are 0).
// Translation: t = centroid_t - R centroid_s.
GLIM_AMD_RP_HD inline int solve_pose(const double* s, const double* t, double poly_error_thresh, int dof, double* T) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  bool finite = true;
  GLIM_AMD_RP_UNROLL
  for (int i = 0; i < 9; i++) finite = finite && (fabs(s[i]) <= 1.7976931348623157e308) && (fabs(t[i]) <= 1.7976931348623157e308);  // (false for NaN)
  if (!finite) return DEGENERATE;
  bool edges_ok = true;
  GLIM_AMD_RP_UNROLL
  for (int a = 0; a < 3; a++) {
    const int b = (a + 1) % 3;
    const double sx = s[3 * a] - s[3 * b], sy = s[3 * a + 1] - s[3 * b + 1], sz = s[3 * a + 2] - s[3 * b + 2];
    const double tx = t[3 * a] - t[3 * b], ty = t[3 * a + 1] - t[3 * b + 1], tz = t[3 * a + 2] - t[3 * b + 2];
    const double ds = sqrt((sx * sx + sy * sy) + sz * sz), dt = sqrt((tx * tx + ty * ty) + tz * tz);
    const double lo = ds < dt ? ds : dt, hi = ds < dt ? dt : ds;
    edges_ok = edges_ok && (lo >= (1.0 - poly_error_thresh) * hi);
  }
  if (!edges_ok) return EDGE_LENGTH;
  // centroids ((a + b) + c) / 3 and centred points
  double cs[3], ct[3], a[9], b[9];
  GLIM_AMD_RP_UNROLL
  for (int k = 0; k < 3; k++) {
    cs[k] = ((s[k] + s[3 + k]) + s[6 + k]) / 3.0;
    ct[k] = ((t[k] + t[3 + k]) + t[6 + k]) / 3.0;
  }
  GLIM_AMD_RP_UNROLL
  for (int i = 0; i < 9; i++) {
    a[i] = s[i] - cs[i % 3];
    b[i] = t[i] - ct[i % 3];
  }
  {
    const double e1x = s[3] - s[0], e1y = s[4] - s[1], e1z = s[5] - s[2], e2x = s[6] - s[0], e2y = s[7] - s[1], e2z = s[8] - s[2];
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double q = ((nx * nx + ny * ny) + nz * nz) / 3.0;
    double p = 0.0;
    GLIM_AMD_RP_UNROLL
    for (int i = 0; i < 9; i++) p = fma(a[i], a[i], p);
    const double disc = p * p - 4.0 * q;
    const double s1 = 0.5 * (p + sqrt(disc > 0.0 ? disc : 0.0));  // sigma_1^2
    if (!(s1 > 0.0)) return DEGENERATE;
    const double s2 = q / s1;  // sigma_2^2
    if (s2 < (COLLINEAR_RATIO * COLLINEAR_RATIO) * s1) return DEGENERATE;
  }
  double R[9];
  if (dof == 4) {
    double S = 0.0, C = 0.0;
    GLIM_AMD_RP_UNROLL
    for (int k = 0; k < 3; k++) {
      S = S + (a[3 * k] * b[3 * k + 1] - a[3 * k + 1] * b[3 * k]);
      C = C + (a[3 * k] * b[3 * k] + a[3 * k + 1] * b[3 * k + 1]);
    }
    yaw_rotation(S, C, R);
  } else {
    // H[i][j] = sum_k a_k[i] b_k[j]
    double H[9];
    GLIM_AMD_RP_UNROLL
    for (int i = 0; i < 3; i++) {
      GLIM_AMD_RP_UNROLL
      for (int j = 0; j < 3; j++) H[3 * i + j] = (a[i] * b[j] + a[3 + i] * b[3 + j]) + a[6 + i] * b[6 + j];
    }
    horn_rotation(H, R);
  }
  GLIM_AMD_RP_UNROLL
  for (int r = 0; r < 3; r++) {
    T[4 * r] = R[3 * r], T[4 * r + 1] = R[3 * r + 1], T[4 * r + 2] = R[3 * r + 2];
    T[4 * r + 3] = ct[r] - ((R[3 * r] * cs[0] + R[3 * r + 1] * cs[1]) + R[3 * r + 2] * cs[2]);
  }
  return OK;
}

}  // namespace ransac_pose
}  // namespace glim_amd
