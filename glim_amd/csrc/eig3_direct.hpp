// eig3_direct.hpp -- closed-form eigen-decomposition of a symmetric 3x3 matrix, all three pairs: the solver the reference calls as
// Eigen::SelfAdjointEigenSolver<Matrix3d>::computeDirect (bundle_adjustment_modal.cpp:181), stated step by step like the oracle's
// restatement of it (oracle/vgicp_oracle.c: eig3_roots, eig3_extract_kernel and the driver after them).  covariance.hip holds its own
// device form of the smallest-eigenvector part, pinned bit for bit by existing tests; this header does not touch it.
//
// Plain C++ as well as HIP: a stand-alone host program may include it without the HIP toolchain (tests/test_plane_ba.py).  No FMA
// contraction anywhere; what differs between host and device is the last place of atan2 / cos / sin only.
#pragma once

#include <math.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define GLIM_AMD_EIG_HD __host__ __device__
#else
#define GLIM_AMD_EIG_HD
#endif

namespace glim_amd {
namespace eig3 {

GLIM_AMD_EIG_HD inline void roots(const double m[3][3], double r[3]) {
#pragma clang fp contract(off)
  const double s_inv3 = 1.0 / 3.0;
  const double s_sqrt3 = sqrt(3.0);
  const double c0 = m[0][0] * m[1][1] * m[2][2] + 2.0 * m[1][0] * m[2][0] * m[2][1] - m[0][0] * m[2][1] * m[2][1] - m[1][1] * m[2][0] * m[2][0] -
                    m[2][2] * m[1][0] * m[1][0];
  const double c1 = m[0][0] * m[1][1] - m[1][0] * m[1][0] + m[0][0] * m[2][2] - m[2][0] * m[2][0] + m[1][1] * m[2][2] - m[2][1] * m[2][1];
  const double c2 = m[0][0] + m[1][1] + m[2][2];
  const double c2_over_3 = c2 * s_inv3;
  double a_over_3 = (c2 * c2_over_3 - c1) * s_inv3;
  if (a_over_3 < 0.0) a_over_3 = 0.0;
  const double half_b = 0.5 * (c0 + c2_over_3 * (2.0 * c2_over_3 * c2_over_3 - c1));
  double q = a_over_3 * a_over_3 * a_over_3 - half_b * half_b;
  if (q < 0.0) q = 0.0;
  const double rho = sqrt(a_over_3);
  const double theta = atan2(sqrt(q), half_b) * s_inv3;
  const double cos_theta = cos(theta);
  const double sin_theta = sin(theta);
  r[0] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
  r[1] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
  r[2] = c2_over_3 + 2.0 * rho * cos_theta;
}

GLIM_AMD_EIG_HD inline void cross(const double* a, const double* b, double* c) {
#pragma clang fp contract(off)
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// null vector of a rank-2 symmetric matrix; `rep` receives the representative column
GLIM_AMD_EIG_HD inline void extract_kernel(const double mat[3][3], double* res, double* rep) {
#pragma clang fp contract(off)
  int i0 = 0;
  double best = fabs(mat[0][0]);
  for (int i = 1; i < 3; i++)
    if (fabs(mat[i][i]) > best) {
      best = fabs(mat[i][i]);
      i0 = i;
    }
  const int i1 = (i0 + 1) % 3, i2 = (i0 + 2) % 3;
  double col0[3], col1[3], col2[3];
  for (int r = 0; r < 3; r++) {
    col0[r] = mat[r][i0];
    col1[r] = mat[r][i1];
    col2[r] = mat[r][i2];
  }
  rep[0] = col0[0];
  rep[1] = col0[1];
  rep[2] = col0[2];
  double c0[3], c1[3];
  cross(col0, col1, c0);
  cross(col0, col2, c1);
  const double n0 = c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2];
  const double n1 = c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2];
  if (n0 > n1) {
    const double s = sqrt(n0);
    res[0] = c0[0] / s;
    res[1] = c0[1] / s;
    res[2] = c0[2] / s;
  } else {
    const double s = sqrt(n1);
    res[0] = c1[0] / s;
    res[1] = c1[1] / s;
    res[2] = c1[2] / s;
  }
}

// m9: row-major symmetric 3x3 (the lower triangle is read).  evals: ascending.  evecs: evecs[3 * k + r] = component r of eigenvector k.
GLIM_AMD_EIG_HD inline void direct(const double* m9, double* evals, double* evecs) {
#pragma clang fp contract(off)
  const double eps = 2.220446049250313e-16;
  double sm[3][3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) sm[r][c] = (r >= c) ? m9[3 * r + c] : m9[3 * c + r];
  const double shift = (sm[0][0] + (sm[1][1] + sm[2][2])) / 3.0;
  for (int i = 0; i < 3; i++) sm[i][i] -= shift;
  double scale = 0.0;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++)
      if (fabs(sm[r][c]) > scale) scale = fabs(sm[r][c]);
  if (scale > 0.0)
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) sm[r][c] /= scale;

  double ev[3];
  roots(sm, ev);

  double V[3][3];  // V[k] = eigenvector k
  if ((ev[2] - ev[0]) <= eps) {
    for (int c = 0; c < 3; c++)
      for (int r = 0; r < 3; r++) V[c][r] = (r == c) ? 1.0 : 0.0;
  } else {
    double tmp[3][3];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) tmp[r][c] = sm[r][c];
    double d0 = ev[2] - ev[1];
    const double d1 = ev[1] - ev[0];
    int k = 0, l = 2;
    if (d0 > d1) {
      k = 2;
      l = 0;
      d0 = d1;
    }
    const double evk = (k == 2) ? ev[2] : ev[0];
    for (int i = 0; i < 3; i++) tmp[i][i] -= evk;
    // (k and l are 0 / 2 or 2 / 0: written out so that V is never indexed by a run-time value on the device)
    double vk[3], vl[3];
    extract_kernel(tmp, vk, vl);
    if (d0 <= 2.0 * eps * d1) {
      const double dot = vk[0] * vl[0] + vk[1] * vl[1] + vk[2] * vl[2];
      for (int r = 0; r < 3; r++) vl[r] -= dot * vl[r];
      const double nn = sqrt(vl[0] * vl[0] + vl[1] * vl[1] + vl[2] * vl[2]);
      for (int r = 0; r < 3; r++) vl[r] /= nn;
    } else {
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) tmp[r][c] = sm[r][c];
      const double evl = (l == 2) ? ev[2] : ev[0];
      for (int i = 0; i < 3; i++) tmp[i][i] -= evl;
      double dummy[3];
      extract_kernel(tmp, vl, dummy);
    }
    for (int r = 0; r < 3; r++) {
      V[0][r] = (k == 0) ? vk[r] : vl[r];
      V[2][r] = (k == 0) ? vl[r] : vk[r];
    }
    double c1[3];
    cross(V[2], V[0], c1);
    const double nn = sqrt(c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2]);
    for (int r = 0; r < 3; r++) V[1][r] = c1[r] / nn;
  }
  for (int i = 0; i < 3; i++) evals[i] = ev[i] * scale + shift;
  for (int c = 0; c < 3; c++)
    for (int r = 0; r < 3; r++) evecs[3 * c + r] = V[c][r];
}

}  // namespace eig3
}  // namespace glim_amd
