// nav_terms.hpp -- the velocity and bias variables of the global-graph optimisation and the three terms GLIM's IMU graphs are made of beside
// the pose terms (include/glim_amd.h "Graph optimisation with velocity and bias variables"), ONCE, for host and device.  bundle_lm_step.hpp's
// item, assembly and step functions call what is here; bundle_align.hip runs the item functions a thread per term; tests/cpp/test_nav_graph_step.cpp
// compiles the header with a plain C++ compiler; tests/nav_graph_restatement.py restates it in NumPy.  Plain C++ apart from the host/device macro.
//
//   nodes      the N six-wide blocks of the system are nodes with a kind.  POSE: 12 doubles, retraction X Exp(delta) (lm::retract).  BIAS: 6
//              doubles in gtsam's ConstantBias::vector() order (acc, gyro), retraction b + delta.  VELOCITY: 3 doubles (world frame), retraction
//              v + delta[0..3); its rows 3..5 are touched by nothing: lambda on the diagonal, +0.0 on the right-hand side, a zero step.  A node's
//              value travels as a row of 12 doubles; a vector kind uses the leading 6 / 3, the rest is +0.0 and stays +0.0.
//   products   every term adds J^T L J, J^T L r and r^T L r with term_products' convention at its own sizes (products below): L r and L J first,
//              sums ascending from +0.0, the upper triangle of L read.
//   prior      vector prior (node k of kind BIAS or VELOCITY, value p[6], information 6 x 6): r = x_k - p, J = I.  For a VELOCITY the leading
//              3 x 3 of L and 3 of p are read.  (PriorFactor<Vector3>, PriorFactor<ConstantBias>: sub_mapping.cpp:226-227.)
//   between    vector between (nodes i != j of one vector kind, measurement d[6], information): r = (x_j - x_i) - d, J = [-I | I].
//              (BetweenFactor<ConstantBias>, BetweenFactor<Vector3>: sub_mapping.cpp:235, 240.)
//   imu        (POSE i, VELOCITY vi, POSE j, VELOCITY vj, BIAS b) is gtsam::ImuFactor (sub_mapping.cpp:237).  gtsam's source is not in the
//              reference tree: what follows is UPSTREAM RECALL of PreintegrationBase::computeError (biasCorrectedDelta, NavState::retract of
//              the corrected delta, NavState::localCoordinates) without Coriolis term and body_P_sensor.  Per term: dt > 0, gravity g
//              (n_gravity), bias_hat[6], delta[9] = (theta, dp, dv) the preintegrated measurement at bias_hat, H_bias (9 x 6, its derivative by
//              (acc, gyro)), the information 9 x 9 in (rot, pos, vel) order, a mode.  With db = b - bias_hat:
//                (., dp_c, dv_c) = delta + H_bias db on the six position and velocity rows, in both modes
//                TANGENT  (gtsam's TangentPreintegration): theta_c = theta + H_bias[0..3, :] db
//                MANIFOLD (Forster et al.):                theta_c = Log(Exp(theta) Exp(H_bias[0..3, 3..6] db_gyro))
//                R^ = R_i Exp(theta_c),  p^ = p_i + v_i dt + g dt^2 / 2 + R_i dp_c,  v^ = v_i + g dt + R_i dv_c
//                r = [ Log(R_j^T R^) ; R_j^T (p^ - p_j) ; R_j^T (v^ - v_j) ]
//              J (9 x 24, columns [X_i: omega rho | v_i | X_j: omega rho | v_j | b: acc gyro]) is the derivative of r under the retractions
//              above, with A = R_j^T R_i, E = R_j^T R^, K = J_r(r_rot)^-1:
//                r_rot:  d omega_i = K Exp(theta_c)^T;  d omega_j = -K E^T;  d b = K J_r(theta_c) H_bias[0..3, :] (TANGENT),
//                        d b_gyro = K J_r(u) H_bias[0..3, 3..6] with u = H_bias[0..3, 3..6] db_gyro and d b_acc = 0 (MANIFOLD)
//                r_pos:  d omega_i = -A hat(dp_c);  d rho_i = A;  d v_i = R_j^T dt;  d omega_j = hat(r_pos);  d rho_j = -I;  d b = A H_bias[3..6, :]
//                r_vel:  d omega_i = -A hat(dv_c);  d v_i = R_j^T;  d omega_j = hat(r_vel);  d v_j = -R_j^T;  d b = A H_bias[6..9, :]
//              Log, Exp, J_r and J_r^-1 are ct_se3.hpp's (the rotation part of se3_exp, se3_log, se3_jr_blocks and inv3), called.
// Out of scope: CombinedImuFactor, the Coriolis term, body_P_sensor, a preintegrator for raw IMU samples.
#pragma once
#include "ct_se3.hpp"
#include "lm_step.hpp"

namespace glim_amd {
namespace nav {

enum { NODE_POSE = 0, NODE_BIAS = 1, NODE_VELOCITY = 2 };
enum { IMU_TANGENT = 0, IMU_MANIFOLD = 1 };
constexpr int VPRIOR_STRIDE = 36 + 6 + 1;      // doubles of a vector prior's contribution: H (6 x 6), b, cost
constexpr int VBETWEEN_STRIDE = 144 + 12 + 1;  // of a vector between's: H (12 x 12, [i | j]), b, cost
constexpr int IMU_W = 24;                      // the columns of an IMU term: X_i 6 | v_i 3 | X_j 6 | v_j 3 | b 6
constexpr int IMU_STRIDE = IMU_W * IMU_W + IMU_W + 1;
constexpr int IMU_DATA = 1 + 3 + 6 + 9 + 54 + 81;  // doubles of a term: dt | gravity | bias_hat | delta | H_bias (9 x 6) | information (9 x 9)
constexpr int IMU_SLOTS = 5;                   // X_i, v_i, X_j, v_j, b

GLIM_AMD_LM_HD inline int imu_offset(int slot) { return slot == 0 ? 0 : slot == 1 ? 6 : slot == 2 ? 9 : slot == 3 ? 15 : 18; }
GLIM_AMD_LM_HD inline int imu_width(int slot) { return slot == 1 || slot == 3 ? 3 : 6; }
GLIM_AMD_LM_HD inline int node_dim(int kind) { return kind == NODE_VELOCITY ? 3 : 6; }

// the new terms of a graph, and where their contributions at the evaluation live (scratch)
struct Terms {
  const int* kind = nullptr;  // N: the nodes' kinds; or null: every node is a pose and there is no term below
  int VP = 0, VB = 0, I = 0;
  const int* vpk = nullptr;                      // VP: node of a vector prior
  const double *vpv = nullptr, *vpL = nullptr;   //     its value (6) and information (36)
  const int *vbi = nullptr, *vbj = nullptr;      // VB: nodes of a vector between
  const double *vbd = nullptr, *vbL = nullptr;   //     its measurement (6) and information (36)
  const int *imn = nullptr, *imm = nullptr;      // I: the five nodes of an IMU term (X_i, v_i, X_j, v_j, b); its mode
  const double* imd = nullptr;                   //    IMU_DATA doubles
  double *vpc = nullptr, *vbc = nullptr, *ic = nullptr;  // scratch: VPRIOR_STRIDE VP, VBETWEEN_STRIDE VB, IMU_STRIDE I
};
GLIM_AMD_LM_HD inline int kind_of(const Terms& t, int node) { return t.kind ? t.kind[node] : NODE_POSE; }

// J: m x w row-major, L: m x m with row stride ls (upper triangle read), r: m  ->  out: J^T L J (w x w, full), J^T L r (w), r^T L r.
// bundle_lm::term_products at any size (m <= 9, w <= IMU_W)
GLIM_AMD_LM_HD inline void products(const double* J, int m, int w, const double* L, int ls, const double* r, double* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double Lr[9], LJ[9 * IMU_W];
  for (int a = 0; a < m; a++) {
    double s = 0.0;
    for (int n = 0; n < m; n++) s += L[a <= n ? ls * a + n : ls * n + a] * r[n];
    Lr[a] = s;
    for (int c = 0; c < w; c++) {
      double u = 0.0;
      for (int n = 0; n < m; n++) u += L[a <= n ? ls * a + n : ls * n + a] * J[w * n + c];
      LJ[w * a + c] = u;
    }
  }
  for (int a = 0; a < w; a++) {
    for (int b = a; b < w; b++) {
      double s = 0.0;
      for (int k = 0; k < m; k++) s += J[w * k + a] * LJ[w * k + b];
      out[w * a + b] = out[w * b + a] = s;
    }
    double g = 0.0;
    for (int k = 0; k < m; k++) g += J[w * k + a] * Lr[k];
    out[w * w + a] = g;
  }
  double rr = 0.0;
  for (int k = 0; k < m; k++) rr += r[k] * Lr[k];
  out[w * w + w] = rr;
}

// a node's retraction by its kind: out = x (+) delta (12 doubles each, delta 6)
GLIM_AMD_LM_HD inline void retract_node(int kind, const double* x, const double* delta, double* out) {
  if (kind == NODE_POSE) {
    lm::retract(x, delta, out);
    return;
  }
  const int d = node_dim(kind);
  for (int i = 0; i < 12; i++) out[i] = i < d ? x[i] + delta[i] : 0.0;
}

// vector prior p: its contribution in the 6 x 6 layout (a VELOCITY fills the leading 3 x 3 and 3 of b; the rest is +0.0 and never read)
GLIM_AMD_LM_HD inline __attribute__((noinline)) void vector_prior_term(const Terms& t, const double* X, int p) {
  const int k = t.vpk[p], d = node_dim(kind_of(t, k));
  double r[6], J[36], o[VPRIOR_STRIDE];
  for (int a = 0; a < d; a++) {
    r[a] = X[12 * k + a] - t.vpv[6 * p + a];
    for (int b = 0; b < d; b++) J[d * a + b] = a == b ? 1.0 : 0.0;
  }
  products(J, d, d, t.vpL + 36 * p, 6, r, o);
  double* out = t.vpc + VPRIOR_STRIDE * p;
  for (int u = 0; u < VPRIOR_STRIDE; u++) out[u] = 0.0;
  for (int a = 0; a < d; a++) {
    for (int b = 0; b < d; b++) out[6 * a + b] = o[d * a + b];
    out[36 + a] = o[d * d + a];
  }
  out[42] = o[d * d + d];
}

// vector between q: its contribution in the 12 x 12 layout [i | j]
GLIM_AMD_LM_HD inline __attribute__((noinline)) void vector_between_term(const Terms& t, const double* X, int q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int i = t.vbi[q], j = t.vbj[q], d = node_dim(kind_of(t, i)), w = 2 * d;
  double r[6], J[72], o[VBETWEEN_STRIDE];
  for (int a = 0; a < d; a++) {
    r[a] = (X[12 * j + a] - X[12 * i + a]) - t.vbd[6 * q + a];
    for (int b = 0; b < d; b++) {
      J[w * a + b] = a == b ? -1.0 : 0.0;
      J[w * a + d + b] = a == b ? 1.0 : 0.0;
    }
  }
  products(J, d, w, t.vbL + 36 * q, 6, r, o);
  double* out = t.vbc + VBETWEEN_STRIDE * q;
  for (int u = 0; u < VBETWEEN_STRIDE; u++) out[u] = 0.0;
  for (int a = 0; a < w; a++) {
    const int ra = a < d ? a : 6 + a - d;
    for (int b = 0; b < w; b++) out[12 * ra + (b < d ? b : 6 + b - d)] = o[w * a + b];
    out[144 + ra] = o[w * w + a];
  }
  out[156] = o[w * w + w];
}

// the rotation part of ct_se3's maps
GLIM_AMD_LM_HD inline void so3_exp(const double* w, double* R) {
  const double xi[6] = {w[0], w[1], w[2], 0.0, 0.0, 0.0};
  double T[12];
  ct_se3::se3_exp(xi, T);
  ct_se3::rot_of(T, R);
}
GLIM_AMD_LM_HD inline void so3_log(const double* R, double* w) {
  const double T[12] = {R[0], R[1], R[2], 0.0, R[3], R[4], R[5], 0.0, R[6], R[7], R[8], 0.0};
  double xi[6];
  ct_se3::se3_log(T, xi);
  w[0] = xi[0], w[1] = xi[1], w[2] = xi[2];
}
GLIM_AMD_LM_HD inline void so3_jr(const double* w, double* J) {
  const double xi[6] = {w[0], w[1], w[2], 0.0, 0.0, 0.0};
  double Q[9];
  ct_se3::se3_jr_blocks(xi, J, Q);
}
// C = A^T B
GLIM_AMD_LM_HD inline void mtm3(const double* A, const double* B, double* C) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) C[3 * r + c] = A[r] * B[c] + A[3 + r] * B[3 + c] + A[6 + r] * B[6 + c];
}
// block (rows r0.., columns c0..) of J (9 x IMU_W) = sign * M (3 x 3)
GLIM_AMD_LM_HD inline void put3(double* J, int r0, int c0, const double* M, double sign) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) J[IMU_W * (r0 + r) + c0 + c] = sign * M[3 * r + c];
}

// the IMU term's residual r (9) and Jacobian J (9 x IMU_W row-major) at (X_i, v_i, X_j, v_j, b); d: the term's IMU_DATA doubles
GLIM_AMD_LM_HD inline void imu_residual(const double* Xi, const double* vi, const double* Xj, const double* vj, const double* b, const double* d, int mode, double* r,
                                        double* J) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double dt = d[0], *g = d + 1, *bh = d + 4, *del = d + 10, *H = d + 19;
  double db[6], c[9];
  for (int k = 0; k < 6; k++) db[k] = b[k] - bh[k];
  for (int m = 0; m < 9; m++) {
    double s = 0.0;
    for (int k = 0; k < 6; k++) s += H[6 * m + k] * db[k];
    c[m] = del[m] + s;
  }
  double Ec[9], Jb[9];  // Exp(theta_c); d theta_c (as a right perturbation of Exp(theta_c)) by the three columns it depends on: Jb H_rot
  if (mode == IMU_MANIFOLD) {
    double u[3], Rt[9], Ru[9];
    for (int m = 0; m < 3; m++) {
      double s = 0.0;
      for (int k = 0; k < 3; k++) s += H[6 * m + 3 + k] * db[3 + k];
      u[m] = s;
    }
    so3_exp(del, Rt);
    so3_exp(u, Ru);
    ct_se3::mm3(Rt, Ru, Ec);
    so3_log(Ec, c);
    so3_jr(u, Jb);
  } else {
    so3_exp(c, Ec);
    so3_jr(c, Jb);
  }
  double Ri[9], Rj[9], A[9], E[9], rr[3], Jw[9], K[9];
  ct_se3::rot_of(Xi, Ri);
  ct_se3::rot_of(Xj, Rj);
  mtm3(Rj, Ri, A);
  ct_se3::mm3(A, Ec, E);
  so3_log(E, rr);
  so3_jr(rr, Jw);
  ct_se3::inv3(Jw, K);
  double ap[3], av[3];
  for (int m = 0; m < 3; m++) {
    const double Rp = Ri[3 * m] * c[3] + Ri[3 * m + 1] * c[4] + Ri[3 * m + 2] * c[5];
    const double Rv = Ri[3 * m] * c[6] + Ri[3 * m + 1] * c[7] + Ri[3 * m + 2] * c[8];
    ap[m] = (((Xi[4 * m + 3] + vi[m] * dt) + 0.5 * g[m] * dt * dt) + Rp) - Xj[4 * m + 3];
    av[m] = ((vi[m] + g[m] * dt) + Rv) - vj[m];
  }
  for (int m = 0; m < 3; m++) {
    r[m] = rr[m];
    r[3 + m] = Rj[m] * ap[0] + Rj[3 + m] * ap[1] + Rj[6 + m] * ap[2];
    r[6 + m] = Rj[m] * av[0] + Rj[3 + m] * av[1] + Rj[6 + m] * av[2];
  }
  for (int u = 0; u < 9 * IMU_W; u++) J[u] = 0.0;
  double M[9], N[9], Hx[9], RjT[9], I3[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  for (int a = 0; a < 3; a++)
    for (int k = 0; k < 3; k++) RjT[3 * a + k] = Rj[3 * k + a];
  // r_rot
  for (int a = 0; a < 3; a++)
    for (int k = 0; k < 3; k++) M[3 * a + k] = Ec[3 * k + a];
  ct_se3::mm3(K, M, N);
  put3(J, 0, 0, N, 1.0);  // omega_i: K Exp(theta_c)^T
  for (int a = 0; a < 3; a++)
    for (int k = 0; k < 3; k++) M[3 * a + k] = E[3 * k + a];
  ct_se3::mm3(K, M, N);
  put3(J, 0, 9, N, -1.0);  // omega_j: -K E^T
  ct_se3::mm3(K, Jb, M);
  for (int half = mode == IMU_MANIFOLD ? 1 : 0; half < 2; half++) {
    for (int a = 0; a < 3; a++)
      for (int k = 0; k < 3; k++) Hx[3 * a + k] = H[6 * a + 3 * half + k];
    ct_se3::mm3(M, Hx, N);
    put3(J, 0, 18 + 3 * half, N, 1.0);
  }
  // r_pos, r_vel
  for (int part = 0; part < 2; part++) {
    const int r0 = 3 + 3 * part;
    ct_se3::ct_hat(c + r0, Hx);
    ct_se3::mm3(A, Hx, N);
    put3(J, r0, 0, N, -1.0);  // omega_i: -A hat(dp_c) / -A hat(dv_c)
    ct_se3::ct_hat(r + r0, Hx);
    put3(J, r0, 9, Hx, 1.0);  // omega_j: hat(r_pos) / hat(r_vel)
    for (int half = 0; half < 2; half++) {
      for (int a = 0; a < 3; a++)
        for (int k = 0; k < 3; k++) Hx[3 * a + k] = H[6 * (r0 + a) + 3 * half + k];
      ct_se3::mm3(A, Hx, N);
      put3(J, r0, 18 + 3 * half, N, 1.0);
    }
  }
  put3(J, 3, 3, A, 1.0);     // rho_i
  put3(J, 3, 6, RjT, dt);    // v_i
  put3(J, 3, 12, I3, -1.0);  // rho_j
  put3(J, 6, 6, RjT, 1.0);   // v_i
  put3(J, 6, 15, RjT, -1.0);  // v_j
}

GLIM_AMD_LM_HD inline __attribute__((noinline)) void imu_term(const Terms& t, const double* X, int q) {
  const int* n = t.imn + IMU_SLOTS * q;
  const double* d = t.imd + (size_t)IMU_DATA * q;
  double r[9], J[9 * IMU_W];
  imu_residual(X + 12 * n[0], X + 12 * n[1], X + 12 * n[2], X + 12 * n[3], X + 12 * n[4], d, t.imm[q], r, J);
  products(J, 9, IMU_W, d + 73, 9, r, t.ic + (size_t)IMU_STRIDE * q);
}

// ---- the test window of the IMU term (tests/cpp/test_nav_graph_step.cpp): in = X_i 12 | v_i 3 | X_j 12 | v_j 3 | b 6 | mode | IMU_DATA;
// out = r 9 | J 9 x IMU_W
constexpr int IMU_EVAL_IN = 37 + IMU_DATA, IMU_EVAL_OUT = 9 + 9 * IMU_W;
GLIM_AMD_LM_HD inline void imu_eval(const double* in, double* out) { imu_residual(in, in + 12, in + 15, in + 27, in + 30, in + 37, (int)in[36], out, out + 9); }

}  // namespace nav
}  // namespace glim_amd
