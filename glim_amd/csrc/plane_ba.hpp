// plane_ba.hpp -- algebra of the plane / edge eigenvalue-minimisation factors (gtsam_points::PlaneEVMFactor / EdgeEVMFactor) over per-frame
// moments.  An eigenvalue of the covariance of transformed points, its gradient and its second derivative under T Exp(xi) are exact
// functions of ten numbers per frame -- n, sum p, sum p p^T --, so a factor is reduced over its points ONCE (plane_ba.hip, creation) and
// every error() / linearize() afterwards costs O(frames^2) and reads no point.
//
// Plain C++ as well as HIP: the same functions run in the kernels of plane_ba.hip and, through ba_linearize_host below, in a stand-alone
// host program (tests/test_plane_ba.py builds one, plain and under the address / undefined-behaviour sanitizers).  No FMA contraction.
//
// Per-frame moments (BA_MOM doubles): [0] n   [1..3] c = the frame's first point, frame-local   [4..6] v = sum (p - c)
//                                     [7..12] P = sum (p - c)(p - c)^T as 00 01 02 11 12 22
// Centring on c keeps |p - c| <= 2 r however far the sub-map's origin is from the ball.  World-side sums are taken about
// tau_0 = R_0 c_0 + t_0 for the same reason: the covariance does not depend on the origin, and only tau - m enters the derivatives.
#pragma once

#include <float.h>
#include <stddef.h>

#include "eig3_direct.hpp"

#define GLIM_AMD_BA_HD GLIM_AMD_EIG_HD

namespace glim_amd {
namespace ba {

constexpr int BA_MOM = 13;
constexpr int BA_MAX_FRAMES = 128;
constexpr int BA_HEAD = 32;  // head of the linearisation workspace, see ba_head
constexpr unsigned int BA_DEGENERATE = 1u;

// workspace of one linearisation (doubles): head | g (6 K) | D (36 K, the diagonal blocks) | vectors ((e * 3 + t) * 6 K + 6 f + a:
// t = 0 the mean term's S, t = 1, 2 the two W_k, k != e ascending)
GLIM_AMD_BA_HD inline size_t ba_workspace_doubles(int K) { return (size_t)BA_HEAD + (size_t)K * (6 + 36 + 36); }
// head: [0] cost  [1] status  [2..4] eigenvalues  [5] N  [6] 2 / N^2  [7 + 2 e + j] coefficient of W_{e, j}  [11..19] eigenvectors (3 k + r)
// [20..22] m (about tau_0)  [23] number of eigenvalue indices (1 plane, 2 edge)

GLIM_AMD_BA_HD inline void ba_tau(const double* mom, const double* T, double* tau) {
#pragma clang fp contract(off)
  for (int r = 0; r < 3; r++) tau[r] = ((T[4 * r] * mom[1] + T[4 * r + 1] * mom[2]) + T[4 * r + 2] * mom[3]) + T[4 * r + 3];
}

// the frame's part of sum q (3) and sum q q^T (6: 00 01 02 11 12 22), about tau_ref
GLIM_AMD_BA_HD inline void ba_frame_sums(const double* mom, const double* T, const double* tau_ref, double* out9) {
#pragma clang fp contract(off)
  const double n = mom[0];
  const double* v = mom + 4;
  const double P[3][3] = {{mom[7], mom[8], mom[9]}, {mom[8], mom[10], mom[11]}, {mom[9], mom[11], mom[12]}};
  double tau[3], Rv[3], RP[3][3];
  ba_tau(mom, T, tau);
  for (int r = 0; r < 3; r++) {
    tau[r] -= tau_ref[r];
    Rv[r] = (T[4 * r] * v[0] + T[4 * r + 1] * v[1]) + T[4 * r + 2] * v[2];
    for (int c = 0; c < 3; c++) RP[r][c] = (T[4 * r] * P[0][c] + T[4 * r + 1] * P[1][c]) + T[4 * r + 2] * P[2][c];
  }
  for (int r = 0; r < 3; r++) out9[r] = Rv[r] + n * tau[r];
  int o = 3;
  for (int a = 0; a < 3; a++)
    for (int b = a; b < 3; b++) {
      const double rprt = (RP[a][0] * T[4 * b] + RP[a][1] * T[4 * b + 1]) + RP[a][2] * T[4 * b + 2];
      out9[o++] = ((rprt + Rv[a] * tau[b]) + tau[a] * Rv[b]) + (n * tau[a]) * tau[b];
    }
}

// N (the point count) and the nine sums over all frames -> the head of the workspace.  kind: 0 plane (lambda_0), 1 edge (lambda_0 + lambda_1).
GLIM_AMD_BA_HD inline void ba_head(double N, const double* sums9, int kind, double* head) {
#pragma clang fp contract(off)
  double m[3], C[9];
  for (int r = 0; r < 3; r++) m[r] = sums9[r] / N;
  const int idx[3][3] = {{3, 4, 5}, {4, 6, 7}, {5, 7, 8}};
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) C[3 * a + b] = sums9[idx[a][b]] / N - m[a] * m[b];
  double lam[3], U[9];
  eig3::direct(C, lam, U);
  const int ne = kind == 0 ? 1 : 2;
  unsigned int status = 0u;
  const double floor_ = 1e-12 * (lam[2] > DBL_MIN ? lam[2] : DBL_MIN);
  const double cS = 2.0 / (N * N);
  for (int e = 0; e < 2; e++) {
    int j = 0;
    for (int k = 0; k < 3; k++) {
      if (k == e) continue;
      const double gap = lam[e] - lam[k];
      double w = 0.0;
      // edge: the (e, k) = (0, 1) and (1, 0) terms are the same W W^T with opposite coefficients; their sum is zero, so neither is formed
      if (e < ne && !(ne == 2 && k < 2)) {
        if (fabs(gap) <= floor_ || !(gap == gap)) status |= BA_DEGENERATE;
        else w = cS / gap;
      }
      head[7 + 2 * e + j] = w;
      j++;
    }
  }
  head[0] = kind == 0 ? lam[0] : lam[0] + lam[1];
  head[1] = (double)status;
  for (int i = 0; i < 3; i++) head[2 + i] = lam[i];
  head[5] = N;
  head[6] = cS;
  for (int i = 0; i < 9; i++) head[11 + i] = U[i];
  for (int i = 0; i < 3; i++) head[20 + i] = m[i];
  head[23] = (double)ne;
}

GLIM_AMD_BA_HD inline void ba_cross(const double* a, const double* b, double* c) {
#pragma clang fp contract(off)
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// frame f's gradient (6), diagonal block (36) and rank-1 vectors into the workspace `ws` (layout above); tangent order [rotation, translation]
GLIM_AMD_BA_HD inline void ba_frame_terms(int f, int K, const double* mom, const double* T, const double* tau_ref, const double* head, double* ws) {
#pragma clang fp contract(off)
  const double n = mom[0], N = head[5];
  const double* cf = mom + 1;
  const double* v = mom + 4;
  const double P[3][3] = {{mom[7], mom[8], mom[9]}, {mom[8], mom[10], mom[11]}, {mom[9], mom[11], mom[12]}};
  const int ne = (int)head[23];
  double tau[3];
  ba_tau(mom, T, tau);
  for (int r = 0; r < 3; r++) tau[r] = (tau[r] - tau_ref[r]) - head[20 + r];  // tau - m
  // c_k = R^T u_k, alpha_k, A_k, B_k for all three eigenvectors
  double c[3][3], A[3], B[3][3];
  for (int k = 0; k < 3; k++) {
    const double* u = head + 11 + 3 * k;
    for (int r = 0; r < 3; r++) c[k][r] = (T[r] * u[0] + T[4 + r] * u[1]) + T[8 + r] * u[2];
    const double alpha = (u[0] * tau[0] + u[1] * tau[1]) + u[2] * tau[2];
    A[k] = ((c[k][0] * v[0] + c[k][1] * v[1]) + c[k][2] * v[2]) + n * alpha;
    for (int r = 0; r < 3; r++) B[k][r] = (((P[r][0] * c[k][0] + P[r][1] * c[k][1]) + P[r][2] * c[k][2]) + alpha * v[r]) + A[k] * cf[r];
  }
  double s[3], Pt[3][3];
  for (int r = 0; r < 3; r++) s[r] = v[r] + n * cf[r];
  for (int a = 0; a < 3; a++)
    for (int b = a; b < 3; b++) Pt[a][b] = Pt[b][a] = ((P[a][b] + v[a] * cf[b]) + cf[a] * v[b]) + (n * cf[a]) * cf[b];
  double* g = ws + BA_HEAD + 6 * f;
  double* D = ws + BA_HEAD + 6 * (size_t)K + 36 * (size_t)f;
  double* vec = ws + BA_HEAD + 42 * (size_t)K;
  const double two_N = 2.0 / N;
  for (int i = 0; i < 6; i++) g[i] = 0.0;
  for (int i = 0; i < 36; i++) D[i] = 0.0;
  for (int e = 0; e < ne; e++) {
    const double* ce = c[e];
    double x[3];
    ba_cross(B[e], ce, x);
    for (int r = 0; r < 3; r++) {
      g[r] += two_N * x[r];
      g[3 + r] += two_N * (A[e] * ce[r]);
    }
    // hat(c) Pt hat(c)^T: column b of Pt hat(c)^T is -(Pt row) x ... written as M = sum over (p x c)(p x c)^T = hat(c) Pt hat(c)^T
    const double h[3][3] = {{0.0, -ce[2], ce[1]}, {ce[2], 0.0, -ce[0]}, {-ce[1], ce[0], 0.0}};
    double hP[3][3];
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) hP[a][b] = (h[a][0] * Pt[0][b] + h[a][1] * Pt[1][b]) + h[a][2] * Pt[2][b];
    double sx[3];
    ba_cross(s, ce, sx);
    for (int a = 0; a < 3; a++)
      for (int b = a; b < 3; b++) {
        const double m = two_N * ((hP[a][0] * h[b][0] + hP[a][1] * h[b][1]) + hP[a][2] * h[b][2]);
        D[6 * a + b] += m;
        if (b != a) D[6 * b + a] += m;
        const double t = two_N * (n * (ce[a] * ce[b]));
        D[6 * (3 + a) + 3 + b] += t;
        if (b != a) D[6 * (3 + b) + 3 + a] += t;
      }
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) {
        const double o = two_N * (sx[a] * ce[b]);
        D[6 * a + 3 + b] += o;
        D[6 * (3 + b) + a] += o;
      }
    double* S = vec + (size_t)(e * 3) * 6 * K + 6 * f;
    for (int r = 0; r < 3; r++) {
      S[r] = sx[r];
      S[3 + r] = n * ce[r];
    }
    int j = 0;
    for (int k = 0; k < 3; k++) {
      if (k == e) continue;
      double x1[3], x2[3];
      ba_cross(B[e], c[k], x1);
      ba_cross(B[k], ce, x2);
      double* W = vec + (size_t)(e * 3 + 1 + j) * 6 * K + 6 * f;
      for (int r = 0; r < 3; r++) {
        W[r] = x1[r] + x2[r];
        W[3 + r] = A[e] * c[k][r] + A[k] * ce[r];
      }
      j++;
    }
  }
}

// entry (i, j) of H (6 K x 6 K) from the workspace: one expression per entry, so that H(i, j) and H(j, i) are the same bits
GLIM_AMD_BA_HD inline double ba_hessian_entry(int i, int j, int K, const double* ws) {
#pragma clang fp contract(off)
  const double* head = ws;
  const int ne = (int)head[23];
  const int fi = i / 6, fj = j / 6;
  double h = fi == fj ? ws[BA_HEAD + 6 * (size_t)K + 36 * (size_t)fi + 6 * (i - 6 * fi) + (j - 6 * fj)] : 0.0;
  const double* vec = ws + BA_HEAD + 42 * (size_t)K;
  for (int e = 0; e < ne; e++) {
    const double* S = vec + (size_t)(e * 3) * 6 * K;
    h -= head[6] * (S[i] * S[j]);
    for (int t = 0; t < 2; t++) {
      const double* W = vec + (size_t)(e * 3 + 1 + t) * 6 * K;
      h += head[7 + 2 * e + t] * (W[i] * W[j]);
    }
  }
  return h;
}

// The whole linearisation on the host, through the functions the kernels call.  moments: K x BA_MOM, poses: K x 12 (3x4 row-major).
// ws: ba_workspace_doubles(K).  g: 6 K, H: 6 K x 6 K row-major (either may be null: error() only).  Returns the status word, or ~0u when
// fewer than three points are held.
inline unsigned int ba_linearize_host(int K, int kind, const double* moments, const double* poses, double* ws, double* cost, double* g, double* H) {
  double tau0[3], sums[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, N = 0.0;
  ba_tau(moments, poses, tau0);
  for (int f = 0; f < K; f++) {
    double part[9];
    ba_frame_sums(moments + (size_t)BA_MOM * f, poses + 12 * (size_t)f, tau0, part);
    for (int i = 0; i < 9; i++) sums[i] += part[i];
    N += moments[(size_t)BA_MOM * f];
  }
  if (N < 3.0) return ~0u;
  ba_head(N, sums, kind, ws);
  *cost = ws[0];
  if (g && H) {
    for (int f = 0; f < K; f++) ba_frame_terms(f, K, moments + (size_t)BA_MOM * f, poses + 12 * (size_t)f, tau0, ws, ws);
    for (int i = 0; i < 6 * K; i++) {
      g[i] = ws[BA_HEAD + i];
      for (int j = 0; j < 6 * K; j++) H[(size_t)i * 6 * K + j] = ba_hessian_entry(i, j, K, ws);
    }
  }
  return (unsigned int)ws[1];
}

// moments of points given with a frame index each, on the host, in the order the device sums them only up to rounding (the device sums
// blocks of 256 by a tree): used by the stand-alone program, never by the library
inline void ba_moments_host(long n, const double* points3, const int* frame, int K, double* moments) {
  for (int f = 0; f < K; f++) {
    double* m = moments + (size_t)BA_MOM * f;
    for (int i = 0; i < BA_MOM; i++) m[i] = 0.0;
    bool first = true;
    for (long i = 0; i < n; i++) {
      if (frame[i] != f) continue;
      const double* p = points3 + 3 * i;
      if (first) {
        m[1] = p[0], m[2] = p[1], m[3] = p[2];
        first = false;
      }
      const double d[3] = {p[0] - m[1], p[1] - m[2], p[2] - m[3]};
      m[0] += 1.0;
      for (int r = 0; r < 3; r++) m[4 + r] += d[r];
      int o = 7;
      for (int a = 0; a < 3; a++)
        for (int b = a; b < 3; b++) m[o++] += d[a] * d[b];
    }
  }
}

}  // namespace ba
}  // namespace glim_amd
