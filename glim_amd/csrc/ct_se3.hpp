// ct_se3.hpp -- SE(3) in FP64 with gtsam::Pose3's conventions, host and device: what the continuous-time GICP factor's bucket pose table
// (gicp.hip's host table, ct_align.hip's pose table kernel) and the terms of the CT frame alignment (ct_lm_step.hpp) are made of.  Each routine
// is defined here, once.  The header includes nothing of the project, so a plain C++ compiler takes it (tests/cpp/test_ct_lm_step.cpp).
//
// gtsam's right-perturbation Jacobians: between(X, Y) = X^-1 Y, H_X = -Ad((X^-1 Y)^-1), H_Y = I; compose(A, B): H_A = Ad(B^-1), H_B = I;
// Expmap(xi): ExpmapDerivative(xi) = J_r(xi); Logmap(T): LogmapDerivative = J_r(Log T)^-1.  Coefficients with a cancelling numerator switch to
// their Taylor series below 0.02 rad, where the first dropped term is, of the coefficient, 1.3e-14 for a (th^6 / 5040), 3.2e-15 for b, 1.1e-15 for c
// and 5e-18 for the log factor (127 th^8 / 604800; it was 1.3e-13 before 31 th^6 / 15120 was added) -- each inside the gates of
// tests/golden/se3_range.npz once multiplied by the W or W^2 it scales; the coefficients of Q switch at 1 rad (se3_jr_blocks).  Poses are row-major 3 x 4, tangents (omega, v), 6 x 6 matrices row-major.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define GLIM_AMD_SE3_HD __host__ __device__
#else
#define GLIM_AMD_SE3_HD
#endif
#if defined(__clang__)
#define GLIM_AMD_SE3_UNROLL _Pragma("unroll")  // small fixed loops over per-thread matrices: unrolled, the matrices stay in registers on the device
#else
#define GLIM_AMD_SE3_UNROLL
#endif

namespace glim_amd {
namespace ct_se3 {

struct Mat6 {
  double m[36];
};
constexpr double CT_SERIES = 0.02;
constexpr double CT_Q_SERIES = 1.0;  // se3_jr_blocks: the coefficients of Q are series below this
constexpr double CT_LOG_SYM = 0.3;  // se3_log: sin(th) below which, past a quarter turn, the axis comes from the symmetric part of R
constexpr int CT_POSE_STRIDE = 84;  // doubles per bucket in the pose table: T_k (12, row-major 3x4) | D0_k (36) | D1_k (36), row-major 6x6

GLIM_AMD_SE3_HD inline void ct_hat(const double* w, double* W) {
  W[0] = 0.0; W[1] = -w[2]; W[2] = w[1];
  W[3] = w[2]; W[4] = 0.0; W[5] = -w[0];
  W[6] = -w[1]; W[7] = w[0]; W[8] = 0.0;
}
GLIM_AMD_SE3_HD inline void mm3(const double* A, const double* B, double* C) {
  GLIM_AMD_SE3_UNROLL
  for (int r = 0; r < 3; r++)
    GLIM_AMD_SE3_UNROLL
    for (int c = 0; c < 3; c++) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
// the rotation of a row-major 3 x 4 pose
GLIM_AMD_SE3_HD inline void rot_of(const double* T12, double* R) {
  GLIM_AMD_SE3_UNROLL
  for (int r = 0; r < 3; r++)
    GLIM_AMD_SE3_UNROLL
    for (int k = 0; k < 3; k++) R[3 * r + k] = T12[4 * r + k];
}
// [[A, 0], [B, A]] from row-major 3 x 3 blocks: the shape of the se(3) Jacobians and of the adjoint below
GLIM_AMD_SE3_HD inline Mat6 block6(const double* A, const double* B) {
  Mat6 M{};
  GLIM_AMD_SE3_UNROLL
  for (int r = 0; r < 3; r++)
    GLIM_AMD_SE3_UNROLL
    for (int k = 0; k < 3; k++) {
      M.m[6 * r + k] = M.m[6 * (r + 3) + k + 3] = A[3 * r + k];
      M.m[6 * (r + 3) + k] = B[3 * r + k];
    }
  return M;
}
GLIM_AMD_SE3_HD inline void inv3(const double* A, double* B) {
  const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
  const double id = 1.0 / (A[0] * c00 + A[1] * c01 + A[2] * c02);
  B[0] = c00 * id; B[1] = (A[2] * A[7] - A[1] * A[8]) * id; B[2] = (A[1] * A[5] - A[2] * A[4]) * id;
  B[3] = c01 * id; B[4] = (A[0] * A[8] - A[2] * A[6]) * id; B[5] = (A[2] * A[3] - A[0] * A[5]) * id;
  B[6] = c02 * id; B[7] = (A[1] * A[6] - A[0] * A[7]) * id; B[8] = (A[0] * A[4] - A[1] * A[3]) * id;
}
// sum_{k >= 0} (-1)^k t2^k / (2 k + k0)! for t2 <= 1, ten terms nested: (1 - t2 / ((k0 + 1) (k0 + 2)) (1 - t2 / ((k0 + 3) (k0 + 4)) (...))) / k0!
GLIM_AMD_SE3_HD inline double alt_series(double t2, int k0) {
  double s = 1.0, f = 1.0;
  GLIM_AMD_SE3_UNROLL
  for (int k = 9; k >= 1; k--) s = 1.0 - s * t2 / (double)((2 * k + k0 - 1) * (2 * k + k0));
  GLIM_AMD_SE3_UNROLL
  for (int k = 2; k <= k0; k++) f *= (double)k;
  return s / f;
}
// (1 - cos th) / th^2 and (th - sin th) / th^3
GLIM_AMD_SE3_HD inline void so3_coeffs(double th, double& b, double& c) {
  const double t2 = th * th;
  if (th < CT_SERIES) {
    b = 0.5 - t2 / 24.0 + t2 * t2 / 720.0;
    c = 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0;
  } else {
    b = (1.0 - cos(th)) / t2;
    c = (th - sin(th)) / (t2 * th);
  }
}
// Pose3::Expmap: T = [Exp(w) | V(w) v], V = I + b W + c W^2.  Not deskew.hip's se3_exp, on purpose: that one repeats the oracle's operation order
// bit for bit, this one uses series coefficients near zero.
GLIM_AMD_SE3_HD inline void se3_exp(const double* xi, double* T12) {
  double W[9], W2[9];
  ct_hat(xi, W);
  mm3(W, W, W2);
  const double th = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
  const double t2 = th * th;
  const double a = th < CT_SERIES ? 1.0 - t2 / 6.0 + t2 * t2 / 120.0 : sin(th) / th;
  double b, c;
  so3_coeffs(th, b, c);
  GLIM_AMD_SE3_UNROLL
  for (int r = 0; r < 3; r++) {
    double tr = 0.0;
    GLIM_AMD_SE3_UNROLL
    for (int k = 0; k < 3; k++) {
      const double I = r == k ? 1.0 : 0.0;
      T12[4 * r + k] = I + a * W[3 * r + k] + b * W2[3 * r + k];
      tr += (I + b * W[3 * r + k] + c * W2[3 * r + k]) * xi[3 + k];
    }
    T12[4 * r + 3] = tr;
  }
}
// Pose3::Logmap: w = Log(R), v = V(w)^-1 t.  The angle is atan2(|vee|, (tr - 1) / 2) throughout.  The axis comes from vee = (R - R^T)v / 2 while
// that is well conditioned: its error grows like eps / (pi - th), and at the exact half turn vee is 0 and the old product th / sin(th) * vee was 0
// -- a zero residual.  With cos(th) < 0 and |vee| = sin(th) < CT_LOG_SYM the axis is the largest column of the symmetric part
// (R + R^T) / 2 - cos(th) I = (1 - cos th) n n^T, normalised, with the sign of vee (vee = 0: first non-zero component positive).
// CT_LOG_SYM is measured against the 200-bit reference of tests/se3_reference.py and the gates of tests/golden/se3_range.npz (omega: 3.9e-15 at
// |omega| ~ 3; v: 1.7e-15 at |t| ~ 0.5).  On the host, over 39 axes, the vee path's worst error / gate in (omega, v) is 0.23 / 0.11 at pi - th = 1,
// 0.31 / 0.36 at 0.5, 0.39 / 0.47 at 0.3, 0.48 / 0.52 at 0.25, 0.64 / 0.73 at 0.2, 0.89 / 0.99 at 0.14, then past the gate: 6.2e-15 in omega at 0.1,
// 6.6e-14 at 0.01, 6.2e-13 at 1e-3, 1.2e-10 at 1e-6, 7.5e-5 at 1e-12.  On an MI355X (contracted products, the device's atan2 and sin) it missed at
// pi - th = 0.1416 by 1.2 to 1.5 times where the host stood at 0.8.  0.3 is the last step at which the host keeps half the gate, which that factor
// needs.  The symmetric path stays at 0.11 / 0.18 of the gate from pi - th = 1 to the half turn.  Outside the cap the bits are the vee path's as
// they always were.
GLIM_AMD_SE3_HD inline void se3_log(const double* T12, double* xi) {
  double R[9];
  rot_of(T12, R);
  const double vx = 0.5 * (R[7] - R[5]), vy = 0.5 * (R[2] - R[6]), vz = 0.5 * (R[3] - R[1]);
  const double s = sqrt(vx * vx + vy * vy + vz * vz), cth = 0.5 * (R[0] + R[4] + R[8] - 1.0);
  const double th = atan2(s, cth);
  const double t2 = th * th;
  if (cth < 0.0 && s < CT_LOG_SYM) {
    const int j = R[0] >= R[4] ? (R[0] >= R[8] ? 0 : 2) : (R[4] >= R[8] ? 1 : 2);
    double n[3];
    GLIM_AMD_SE3_UNROLL
    for (int r = 0; r < 3; r++) n[r] = 0.5 * (R[3 * r + j] + R[3 * j + r]) - (r == j ? cth : 0.0);
    const double d = n[0] * vx + n[1] * vy + n[2] * vz;
    const bool neg = d < 0.0 || (d == 0.0 && (n[0] != 0.0 ? n[0] < 0.0 : n[1] != 0.0 ? n[1] < 0.0 : n[2] < 0.0));
    const double g = (neg ? -th : th) / sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    xi[0] = g * n[0];
    xi[1] = g * n[1];
    xi[2] = g * n[2];
  } else {
    const double f = th < CT_SERIES ? 1.0 + t2 / 6.0 + 7.0 * t2 * t2 / 360.0 + 31.0 * t2 * t2 * t2 / 15120.0 : th / sin(th);
    xi[0] = f * vx;
    xi[1] = f * vy;
    xi[2] = f * vz;
  }
  double W[9], W2[9], V[9], Vi[9];
  ct_hat(xi, W);
  mm3(W, W, W2);
  double b, c;
  so3_coeffs(th, b, c);
  GLIM_AMD_SE3_UNROLL
  for (int u = 0; u < 9; u++) V[u] = (u % 4 == 0 ? 1.0 : 0.0) + b * W[u] + c * W2[u];
  inv3(V, Vi);
  GLIM_AMD_SE3_UNROLL
  for (int r = 0; r < 3; r++) xi[3 + r] = Vi[3 * r] * T12[3] + Vi[3 * r + 1] * T12[7] + Vi[3 * r + 2] * T12[11];
}
// the blocks of Pose3::ExpmapDerivative, [[Jw, 0], [Q, Jw]] (Jw = Rot3::ExpmapDerivative, Q = computeQforExpmapDerivative)
GLIM_AMD_SE3_HD inline void se3_jr_blocks(const double* xi, double* Jw, double* Q) {
  double W[9], V[9], W2[9];
  ct_hat(xi, W);
  ct_hat(xi + 3, V);
  mm3(W, W, W2);
  const double th = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]), t2 = th * th;
  double b, c;
  so3_coeffs(th, b, c);
  GLIM_AMD_SE3_UNROLL
  for (int u = 0; u < 9; u++) Jw[u] = (u % 4 == 0 ? 1.0 : 0.0) - b * W[u] + c * W2[u];
  // ca = (th - sin) / th^3, cb = (1 - th^2 / 2 - cos) / th^4, cc = -(cb - 3 cd) / 2 with cd = (th - sin - th^3 / 6) / th^5.  The numerators cancel to
  // th^3 / 6, th^4 / 24 and th^5 / 120 of terms of size th and 1, so the closed forms are off by about eps / th^2 of |v| in Q: measured against the
  // 200-bit table (tests/test_se3_range.py) 1e-13 |v| at 0.02 and 5e-15 |v| at 0.1 against a gate of 1.5e-15 |v|.  Below CT_Q_SERIES = 1 they are
  // their alternating series, ten terms (the tenth is < 1e-18 of the first at th = 1)
  double ca, cb, cc;
  if (th < CT_Q_SERIES) {
    ca = alt_series(t2, 3);
    cb = -alt_series(t2, 4);
    cc = -0.5 * (cb + 3.0 * alt_series(t2, 5));
  } else {
    const double t3 = t2 * th, t4 = t2 * t2, t5 = t4 * th, sn = sin(th), cs = cos(th);
    ca = (th - sn) / t3;
    cb = (1.0 - t2 / 2.0 - cs) / t4;
    cc = -0.5 * (cb - 3.0 * (th - sn - t3 / 6.0) / t5);
  }
  double WV[9], VW[9], WVW[9], WWV[9], VWW[9], WVWW[9], WWVW[9];
  mm3(W, V, WV);
  mm3(V, W, VW);
  mm3(WV, W, WVW);
  mm3(W2, V, WWV);
  mm3(V, W2, VWW);
  mm3(WVW, W, WVWW);
  mm3(W, WVW, WWVW);
  GLIM_AMD_SE3_UNROLL
  for (int u = 0; u < 9; u++)
    Q[u] = -0.5 * V[u] + ca * (WV[u] + VW[u] - WVW[u]) + cb * (WWV[u] + VWW[u] - 3.0 * WVW[u]) + cc * (WVWW[u] + WWVW[u]);
}
// Pose3::ExpmapDerivative
GLIM_AMD_SE3_HD inline Mat6 se3_jr(const double* xi) {
  double Jw[9], Q[9];
  se3_jr_blocks(xi, Jw, Q);
  return block6(Jw, Q);
}
// Pose3::LogmapDerivative at Log = xi: the block inverse of se3_jr(xi), [[Jw^-1, 0], [-Jw^-1 Q Jw^-1, Jw^-1]]
GLIM_AMD_SE3_HD inline Mat6 se3_jr_inv(const double* xi) {
  double Jw[9], Q[9], Ji[9], T[9], QJ[9];
  se3_jr_blocks(xi, Jw, Q);
  inv3(Jw, Ji);
  mm3(Q, Ji, T);
  mm3(Ji, T, QJ);
  GLIM_AMD_SE3_UNROLL
  for (double& v : QJ) v = -v;
  return block6(Ji, QJ);
}
// Pose3::AdjointMap: [[R, 0], [hat(t) R, R]]
GLIM_AMD_SE3_HD inline Mat6 se3_ad(const double* T12) {
  const double t[3] = {T12[3], T12[7], T12[11]};
  double R[9], H[9], HR[9];
  rot_of(T12, R);
  ct_hat(t, H);
  mm3(H, R, HR);
  return block6(R, HR);
}
GLIM_AMD_SE3_HD inline Mat6 mm6(const Mat6& A, const Mat6& B) {
  Mat6 C{};
  GLIM_AMD_SE3_UNROLL
  for (int r = 0; r < 6; r++)
    GLIM_AMD_SE3_UNROLL
    for (int c = 0; c < 6; c++) {
      double s = 0.0;
      GLIM_AMD_SE3_UNROLL
      for (int k = 0; k < 6; k++) s += A.m[6 * r + k] * B.m[6 * k + c];
      C.m[6 * r + c] = s;
    }
  return C;
}
GLIM_AMD_SE3_HD inline void se3_compose(const double* A, const double* B, double* C) {
  GLIM_AMD_SE3_UNROLL
  for (int r = 0; r < 3; r++) {
    GLIM_AMD_SE3_UNROLL
    for (int c = 0; c < 4; c++) C[4 * r + c] = A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c] + A[4 * r + 2] * B[8 + c];
    C[4 * r + 3] += A[4 * r + 3];
  }
}
GLIM_AMD_SE3_HD inline void se3_inverse(const double* A, double* B) {
  GLIM_AMD_SE3_UNROLL
  for (int r = 0; r < 3; r++) {
    GLIM_AMD_SE3_UNROLL
    for (int c = 0; c < 3; c++) B[4 * r + c] = A[4 * c + r];
    B[4 * r + 3] = -(A[r] * A[3] + A[4 + r] * A[7] + A[8 + r] * A[11]);
  }
}

// ---- the bucket pose table of the continuous-time factor: T_k = X Exp(t_k Log(X^-1 Y)) with D0_k = d T_k / d X, D1_k = d T_k / d Y ----
// what every bucket of one (X, Y) shares: vel = Log(X^-1 Y), H_log = J_r(vel)^-1, H_b1 = -Ad((X^-1 Y)^-1)
struct CtPoseShared {
  double vel[6];
  Mat6 Jlog, Hb1;
};
GLIM_AMD_SE3_HD inline void ct_pose_shared(const double* X, const double* Y, CtPoseShared& s) {
  double Xi[12], delta[12], Dinv[12];
  se3_inverse(X, Xi);
  se3_compose(Xi, Y, delta);
  se3_log(delta, s.vel);
  se3_inverse(delta, Dinv);
  s.Jlog = se3_jr_inv(s.vel);
  s.Hb1 = se3_ad(Dinv);
  GLIM_AMD_SE3_UNROLL
  for (double& v : s.Hb1.m) v = -v;
}
// bucket t_k: T_k | D0_k | D1_k into o (CT_POSE_STRIDE doubles)
GLIM_AMD_SE3_HD inline void ct_pose_bucket(const double* X, const CtPoseShared& s, double tk, double* o) {
  double xi[6], E[12], Ei[12];
  GLIM_AMD_SE3_UNROLL
  for (int u = 0; u < 6; u++) xi[u] = tk * s.vel[u];
  se3_exp(xi, E);
  se3_inverse(E, Ei);
  se3_compose(X, E, o);
  Mat6 G = mm6(se3_jr(xi), s.Jlog);  // H_compose_2 H_exp t_k H_log
  GLIM_AMD_SE3_UNROLL
  for (double& v : G.m) v *= tk;
  const Mat6 G0 = mm6(G, s.Hb1);
  const Mat6 Ad = se3_ad(Ei);
  GLIM_AMD_SE3_UNROLL
  for (int u = 0; u < 36; u++) {
    o[12 + u] = Ad.m[u] + G0.m[u];
    o[48 + u] = G.m[u];
  }
}
// the whole table at (X, Y): CT_POSE_STRIDE doubles per entry of `table`
GLIM_AMD_SE3_HD inline void ct_pose_table(const double* table, size_t n, const double* X, const double* Y, double* out) {
  CtPoseShared s;
  ct_pose_shared(X, Y, s);
  for (size_t k = 0; k < n; k++) ct_pose_bucket(X, s, table[k], out + k * CT_POSE_STRIDE);
}

// ---- the terms of a pose graph (ct_lm_step.hpp, bundle_lm_step.hpp): residual and Jacobian; what is done with them is the caller's ----
// a prior P on X: r = Log(P^-1 X); returns d r / d X = J_r(r)^-1
GLIM_AMD_SE3_HD inline Mat6 prior_residual(const double* P, const double* X, double* r) {
  double Pi[12], E[12];
  se3_inverse(P, Pi);
  se3_compose(Pi, X, E);
  se3_log(E, r);
  return se3_jr_inv(r);
}
// a measurement D of X^-1 Y: r = Log(D^-1 X^-1 Y); J (6 x 12, row-major) = [d r / d X | d r / d Y] = [-J_r(r)^-1 Ad((X^-1 Y)^-1) | J_r(r)^-1]
GLIM_AMD_SE3_HD inline void between_residual(const double* D, const double* X, const double* Y, double* r, double* J) {
  double Xi[12], XY[12], Di[12], E[12], YX[12];
  se3_inverse(X, Xi);
  se3_compose(Xi, Y, XY);
  se3_inverse(D, Di);
  se3_compose(Di, XY, E);
  se3_log(E, r);
  se3_inverse(XY, YX);
  const Mat6 Ji = se3_jr_inv(r);
  const Mat6 JA = mm6(Ji, se3_ad(YX));
  GLIM_AMD_SE3_UNROLL
  for (int m = 0; m < 6; m++)
    GLIM_AMD_SE3_UNROLL
    for (int c = 0; c < 6; c++) {
      J[12 * m + c] = -JA.m[6 * m + c];
      J[12 * m + 6 + c] = Ji.m[6 * m + c];
    }
}

// ---- the test window of this header: one routine by number on flat arrays (glim_amd_debug_se3_eval on the device, tests/cpp/test_se3_range.cpp
// on the host).  op: in -> out in doubles.  0 exp: xi 6 -> T 12; 1 log: T 12 -> xi 6; 2 jr: xi 6 -> 36; 3 jr_inv: xi 6 -> 36; 4 ad: T 12 -> 36;
// 5 prior_residual: P | X 24 -> r | J 6 + 36; 6 between_residual: D | X | Y 36 -> r | J 6 + 72; 7 ct_pose_bucket: X | Y | t_k 25 -> T_k | D0_k | D1_k 84
constexpr int SE3_EVAL_OPS = 8;
GLIM_AMD_SE3_HD inline int se3_eval_in(int op) { return op == 0 || op == 2 || op == 3 ? 6 : op == 1 || op == 4 ? 12 : op == 5 ? 24 : op == 6 ? 36 : 25; }
GLIM_AMD_SE3_HD inline int se3_eval_out(int op) { return op == 0 ? 12 : op == 1 ? 6 : op == 5 ? 42 : op == 6 ? 78 : op == 7 ? CT_POSE_STRIDE : 36; }
GLIM_AMD_SE3_HD inline void se3_eval(int op, const double* in, double* out) {
  Mat6 M;
  switch (op) {
    case 0: se3_exp(in, out); return;
    case 1: se3_log(in, out); return;
    case 2: M = se3_jr(in); break;
    case 3: M = se3_jr_inv(in); break;
    case 4: M = se3_ad(in); break;
    case 5: M = prior_residual(in, in + 12, out); out += 6; break;
    case 6: between_residual(in, in + 12, in + 24, out, out + 6); return;
    default: {
      CtPoseShared s;
      ct_pose_shared(in, in + 12, s);
      ct_pose_bucket(in, s, in[24], out);
      return;
    }
  }
  GLIM_AMD_SE3_UNROLL
  for (int u = 0; u < 36; u++) out[u] = M.m[u];
}

}  // namespace ct_se3
}  // namespace glim_amd
