// bundle_lm_step.hpp -- the rule of the on-device sub-map bundle optimisation (include/glim_amd.h "Sub-map bundle optimisation"), ONCE, for host
// and device: the expansion of a binary factor, the prior and between terms, the assembly of the dense system, the serial Cholesky and the
// step.  bundle_align.hip's bundle decide kernel runs the ITEM functions below across a workgroup, one owner per item, and runs step() in one
// thread as its cross-check variant; tests/cpp/test_bundle_lm_step.cpp compiles the header with a plain C++ compiler;
// tests/bundle_lm_restatement.py restates it in NumPy.  Plain C++ apart from the host/device macro.
//
// The problem is GLIM's sub-mapping bundle (sub_mapping.cpp:183-216, 276-315, 430-452): N poses X_k, tangent order [X_0: omega v | X_1: omega v
// | ...], right perturbation.  Everything is FP64 with contraction off.
//
//   record     round r evaluates all F factors at T_f = X_t^-1 X_s of the candidate (relative_pose: ct_se3's inverse and compose).  A record is
//              the compact record of lm_step.hpp.
//   blocks     expand_factor: binary_adjoint and expand_compact_record of record_expand.hpp at T_f, the blocks glim_amd_expand_compact gives
//              with GLIM_AMD_FACTOR_BINARY.  H_ss, b_s go to pose s; H_tt, b_t to pose t; H_ts is the block (rows of t, columns of s).
//   terms      prior: r = Log(P^-1 X), J = J_r(r)^-1.  between: r = Log(D^-1 X_i^-1 X_j), J = [-J_r(r)^-1 Ad((X_i^-1 X_j)^-1) | J_r(r)^-1].  Each
//              adds J^T L J to H, J^T L r to b and r^T L r to the cost (term_products; L = the information, of which only the upper triangle
//              is read; L r and L J are formed first, sums ascending from +0.0).
//   huber      a between q may carry a width k_q >= 0 (Graph::bw; 0 or no array: the Gaussian between above, its bits untouched).  After
//              term_products: s = sqrt(c), c = r^T L r.  The between is down-weighted iff k_q > 0 and s > k_q (false for a NaN): then
//              w = k_q / s, each of the 144 + 12 stored values is multiplied once by w and the stored cost becomes k_q ((s + s) - k_q);
//              otherwise w = 1.0 and nothing stored is touched.  This is gtsam's noiseModel::Robust::WhitenSystem and mEstimator::Huber::loss
//              in this header's cost convention (cost = r^T L r, twice gtsam's error).  The weights of the last KEPT evaluation are kept with
//              the kept system (Problem::wk, copied from Problem::wt on accept).
//   damping    a term (pose k, d[6]) is gtsam_points::LinearDampingFactor: from upstream recall its error() is 0 and its linearize() a
//              Hessian factor with G = diag(d), g = 0, f = 0 (the factor's source is not in the reference tree).  It adds d[m]
//              to entry (6k + m, 6k + m) of H and nothing to any other entry, to b or to the cost.  Several on one pose are allowed; a pose
//              touched only by dampings has the block diag(sum d) + lambda I, the right-hand side +0.0 and a zero step.
//   nodes      (the global graph only; Graph::nav, default: none) a block may be a BIAS or a VELOCITY node instead of a pose, and the graph may
//              hold vector priors, vector betweens and IMU terms (gtsam::ImuFactor): nav_terms.hpp, whose item functions are called here.
//              The LDS bundle is not extended: 32 blocks hold only ten frames once a frame needs X, V and B.  Still out of scope: ISAM2,
//              marginals, CombinedImuFactor, IMU terms in the LDS bundle.
//   system     H dense symmetric 6N x 6N, kept as its lower triangle in packed rows (row i at i (i + 1) / 2), then b as row 6N.  Every entry is a
//              sum from +0.0 over the items of its pose block in this order: factors by ascending index, then priors, then betweens, then
//              vector priors, vector betweens and IMU terms, then dampings (assemble_entry, assemble_rhs over the lists build_lists makes).
//              cost = ((((sum_f e_f) + sum priors) + sum betweens) + sum vector priors) + sum vector betweens) + sum IMU terms (total_cost),
//              each ascending from +0.0; without the last three kinds their sums are +0.0 and the bits are those of the first three.  "The cost at a candidate" comes from the LINEARISING evaluation: a trial is one evaluation.
//   solve      (H + lambda I) delta = -b.  L[i][j] = (A[i][j] - sum_{k<j} L[i][k] L[j][k]) / L[j][j], the subtractions one at a time in ascending
//              k (chol_pivot, chol_entry).  -b is carried as row 6N of A, so y = L^-1 (-b) is that row of L.  A pivot that is not > 0 or not
//              finite is a FAILED solve: the candidate is then the kept poses and the trial is rejected.  Back substitution by columns:
//              delta[k] = s[k] / L[k][k], then s[i] -= L[k][i] delta[k] for i < k, k descending from 6N - 1.  A pose no factor or term
//              touches has the block lambda I and a zero step.
//   retract    X_k' = X_k Exp(delta_k) with lm::retract (a BIAS or VELOCITY node: nav::retract_node).  The rotations are re-orthonormalised NEVER.
//   the rest   round 0, accept / reject, the lambda updates, the statuses and the budgets are lm::decide of lm_step.hpp, CALLED with "the error"
//              read as the cost above and "inliers" as the sum of the factors' inlier counts.  A graph WITHOUT factors (F = 0) has no inliers
//              to ask for: the two inlier conditions hold there.  The terms' residuals and Jacobians are ct_se3.hpp's, called too.
//
// The caps: the packed system of MAX_POSES poses, SYSTEM(6 MAX_POSES) = 18 720 doubles = 149 760 B, lives in the 160 KiB of LDS one workgroup of
// a gfx950 CU may declare, beside 14 KiB for the step and the kernel's words.  MAX_FACTORS covers every ordered pair of MAX_POSES poses (992);
// the factors' blocks live in device memory (976 B each), so the number is a bound on scratch, not on LDS.
#pragma once
#include "ct_se3.hpp"
#include "lm_step.hpp"
#include "nav_terms.hpp"
#include "record_expand.hpp"

// an item function: one definition, never inlined, so that the workgroup form and the one-thread form run the same machine code
#define GLIM_AMD_BUNDLE_ITEM GLIM_AMD_LM_HD inline __attribute__((noinline))
// the dot-product loops of the factorisation: unrolled, so that the loads of eight steps are in flight while the subtractions, which stay one
// at a time in ascending k, wait for them (no operation and no order changes: contraction is off and nothing may be reassociated)
#if defined(__clang__)
#define GLIM_AMD_BUNDLE_UNROLL _Pragma("unroll 8")
#else
#define GLIM_AMD_BUNDLE_UNROLL
#endif

namespace glim_amd {
namespace bundle_lm {

constexpr int MAX_POSES = 32;
constexpr int MAX_FACTORS = 1024;
constexpr int MAX_TERMS = 1024;  // priors; and betweens; and dampings
constexpr int MAX_DIM = 6 * MAX_POSES;
constexpr int PRIOR_STRIDE = 36 + 6 + 1;       // doubles of a prior's contribution: H (6 x 6), b, cost
constexpr int BETWEEN_STRIDE = 144 + 12 + 1;   // of a between's: H (12 x 12, [i | j]), b, cost
GLIM_AMD_LM_HD inline int tri(int i) { return i * (i + 1) / 2; }
GLIM_AMD_LM_HD inline int system_doubles(int n) { return tri(n) + n; }  // the packed lower triangle, then row n (b, or -b in the solve)
constexpr int MAX_SYSTEM = MAX_DIM * (MAX_DIM + 1) / 2 + MAX_DIM;

// what an item of a pose block's list adds to the block (rows of pose hi, columns of pose lo, lo <= hi)
// (an IMU item's index is 32 * term + 5 * row slot + column slot: the slots of nav_terms.hpp)
enum { F_TT = 0, F_SS = 1, F_ST = 2, F_TS = 3, PRIOR = 4, B_II = 5, B_JJ = 6, B_JI = 7, B_IJ = 8, DAMP = 9, VPRIOR = 10, VB_II = 11, VB_JJ = 12, VB_JI = 13, VB_IJ = 14, IMU = 15 };

struct Graph {
  int N, F, P, Q;
  const int *ft, *fs;          // F: target and source pose of a factor
  const int* pk;               // P: pose of a prior
  const double *pT, *pL;       //    its pose (12) and information (36)
  const int *bi, *bj;          // Q: poses of a between
  const double *bT, *bL;       //    its measurement (12) and information (36)
  const int *first, *items;    // lists: block (lo, hi) is entry tri(hi) + lo; its items are items[first[e] .. first[e + 1]), item = index << 4 | kind
  int D = 0;                   // dampings
  const int* dk = nullptr;     // D: pose of a damping
  const double* dd = nullptr;  //    its diagonal (6)
  const double* bw = nullptr;  // Q: Huber width of a between (0: Gaussian), or null: every between is Gaussian
  nav::Terms nav;              // node kinds, vector priors, vector betweens, IMU terms (the global graph only); default: none
};
GLIM_AMD_LM_HD inline int list_items(int F, int P, int Q) { return 3 * F + P + 3 * Q; }
GLIM_AMD_LM_HD inline int list_items(int F, int P, int Q, int D) { return list_items(F, P, Q) + D; }
GLIM_AMD_LM_HD inline int list_items(int F, int P, int Q, int D, const nav::Terms& t) { return list_items(F, P, Q, D) + t.VP + 3 * t.VB + 15 * t.I; }

// the lists, in the order of the sums.  first: tri(N) + 1 ints, items: list_items ints, cursor: tri(N) ints of workspace.  Host only.
inline void build_lists(const Graph& g, int* first, int* items, int* cursor) {
  const int nb = tri(g.N);
  for (int pass = 0; pass < 2; pass++) {
    if (pass == 0) {
      for (int e = 0; e <= nb; e++) first[e] = 0;
    } else {
      int at = 0;
      for (int e = 0; e < nb; e++) {
        const int c = first[e + 1];
        first[e] = cursor[e] = at;
        at += c;
      }
      first[nb] = at;
    }
    auto put = [&](int lo, int hi, int index, int kind) {
      const int e = tri(hi) + lo;
      if (pass == 0) first[e + 1]++;
      else items[cursor[e]++] = index << 4 | kind;
    };
    for (int f = 0; f < g.F; f++) {
      const int t = g.ft[f], s = g.fs[f];
      put(t, t, f, F_TT);
      put(s, s, f, F_SS);
      if (t < s) put(t, s, f, F_ST);
      else put(s, t, f, F_TS);
    }
    for (int p = 0; p < g.P; p++) put(g.pk[p], g.pk[p], p, PRIOR);
    for (int q = 0; q < g.Q; q++) {
      const int i = g.bi[q], j = g.bj[q];
      put(i, i, q, B_II);
      put(j, j, q, B_JJ);
      if (i < j) put(i, j, q, B_JI);
      else put(j, i, q, B_IJ);
    }
    for (int p = 0; p < g.nav.VP; p++) put(g.nav.vpk[p], g.nav.vpk[p], p, VPRIOR);
    for (int q = 0; q < g.nav.VB; q++) {
      const int i = g.nav.vbi[q], j = g.nav.vbj[q];
      put(i, i, q, VB_II);
      put(j, j, q, VB_JJ);
      if (i < j) put(i, j, q, VB_JI);
      else put(j, i, q, VB_IJ);
    }
    for (int q = 0; q < g.nav.I; q++) {  // the 15 block pairs of the five nodes
      const int* n = g.nav.imn + nav::IMU_SLOTS * q;
      for (int a = 0; a < nav::IMU_SLOTS; a++)
        for (int b = a; b < nav::IMU_SLOTS; b++) {
          if (n[a] <= n[b]) put(n[a], n[b], 32 * q + 5 * b + a, IMU);
          else put(n[b], n[a], 32 * q + 5 * a + b, IMU);
        }
    }
    for (int d = 0; d < g.D; d++) put(g.dk[d], g.dk[d], d, DAMP);
  }
}

// the layout of the scalar part of a problem's state
struct Scalars {
  double lambda;                       // of the candidate
  double cost, fcost, pcost, bcost;    // at the kept poses
  double inliers;                      // there: the sum of the factors' counts (exact in a double)
  double trial_cost;                   // of the last round's evaluation (kept or not)
  double vpcost, vbcost, icost;        // at the kept poses: the vector priors', the vector betweens', the IMU terms'
  int solve_ok, started, iterations, trials, status, accepted;  // accepted: of the last round
};

// one problem: the graph, what is kept, the candidate, and the scratch of a round
struct Problem {
  Graph g;
  double* X;      // 12 N: the kept poses
  double* cand;   // 12 N: the poses of the next evaluation
  double* delta;  // 6 N: the step that gave them (zero after a failed solve and in round 0)
  double* rec;    // 29 F: the kept records
  double* S;      // system_doubles(6 N): the kept system (H lower-packed, then +b)
  double* Tf;     // 12 F: T_f of the candidate, where the factors of the next round are evaluated
  glim_amd_linearized6* lin;  // F: scratch, the factors' blocks at the evaluation
  double* pc;     // PRIOR_STRIDE P: scratch
  double* bc;     // BETWEEN_STRIDE Q: scratch
  double* W;      // system_doubles(6 N): scratch, the evaluated system and then the solve
  Scalars* s;
  double* wt = nullptr;  // Q: scratch, the betweens' weights at the evaluation; or null: not recorded
  double* wk = nullptr;  // Q: the weights of the kept evaluation; or null
};

// ---- items ------------------------------------------------------------------------------------------------------------------------------------
GLIM_AMD_BUNDLE_ITEM void relative_pose(const double* X, const int* ft, const int* fs, int f, double* Tf) {
  double Ti[12];
  ct_se3::se3_inverse(X + 12 * ft[f], Ti);
  ct_se3::se3_compose(Ti, X + 12 * fs[f], Tf + 12 * f);
}

GLIM_AMD_BUNDLE_ITEM void expand_factor(const double* recs, const double* Tf, int f, glim_amd_linearized6* lin) {
  double adj[ADJOINT_DOUBLES];
  binary_adjoint(Tf + 12 * f, adj);
  expand_compact_record(recs + lm::RECORD * f, adj, lin + f);
}

// J: 6 x w row-major (w = 6 or 12), L: 6 x 6 row-major (upper triangle read), r: 6  ->  out: J^T L J (w x w, full), J^T L r (w), r^T L r
GLIM_AMD_LM_HD inline void term_products(const double* J, int w, const double* L, const double* r, double* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double Lr[6], LJ[72];
  for (int m = 0; m < 6; m++) {
    double s = 0.0;
    for (int n = 0; n < 6; n++) s += L[m <= n ? 6 * m + n : 6 * n + m] * r[n];
    Lr[m] = s;
    for (int c = 0; c < w; c++) {
      double u = 0.0;
      for (int n = 0; n < 6; n++) u += L[m <= n ? 6 * m + n : 6 * n + m] * J[w * n + c];
      LJ[w * m + c] = u;
    }
  }
  for (int a = 0; a < w; a++) {
    for (int b = a; b < w; b++) {
      double s = 0.0;
      for (int m = 0; m < 6; m++) s += J[w * m + a] * LJ[w * m + b];
      out[w * a + b] = out[w * b + a] = s;
    }
    double g = 0.0;
    for (int m = 0; m < 6; m++) g += J[w * m + a] * Lr[m];
    out[w * w + a] = g;
  }
  double rr = 0.0;
  for (int m = 0; m < 6; m++) rr += r[m] * Lr[m];
  out[w * w + w] = rr;
}

GLIM_AMD_BUNDLE_ITEM void prior_term(const Graph& g, const double* X, int p, double* pc) {
  double r[6];
  const ct_se3::Mat6 Ji = ct_se3::prior_residual(g.pT + 12 * p, X + 12 * g.pk[p], r);
  term_products(Ji.m, 6, g.pL + 36 * p, r, pc + PRIOR_STRIDE * p);
}

// wt: the between's weight goes to wt[q] (1.0 unless down-weighted), or null
GLIM_AMD_BUNDLE_ITEM void between_term(const Graph& g, const double* X, int q, double* bc, double* wt) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double r[6], J[72];
  double* out = bc + BETWEEN_STRIDE * q;
  ct_se3::between_residual(g.bT + 12 * q, X + 12 * g.bi[q], X + 12 * g.bj[q], r, J);
  term_products(J, 12, g.bL + 36 * q, r, out);
  double w = 1.0;
  const double k = g.bw ? g.bw[q] : 0.0;
  if (k > 0.0) {
    const double s = sqrt(out[156]);
    if (s > k) {
      w = k / s;
      for (int u = 0; u < 156; u++) out[u] *= w;
      out[156] = k * ((s + s) - k);
    }
  }
  if (wt) wt[q] = w;
}
GLIM_AMD_LM_HD inline void between_term(const Graph& g, const double* X, int q, double* bc) { between_term(g, X, q, bc, nullptr); }

// v[0] + v[stride] + ... (n values), ascending from +0.0
GLIM_AMD_LM_HD inline double sum_ascending(const double* v, int n, int stride) {
  double s = 0.0;
  for (int i = 0; i < n; i++) s += v[(size_t)i * stride];
  return s;
}

// entry (r, c), r >= c, of H
GLIM_AMD_LM_HD inline double assemble_entry(const Graph& g, const glim_amd_linearized6* lin, const double* pc, const double* bc, int r, int c) {
  const int hi = r / 6, lo = c / 6, rr = r - 6 * hi, cc = c - 6 * lo;
  const int e = tri(hi) + lo;
  double s = 0.0;
  for (int u = g.first[e]; u < g.first[e + 1]; u++) {
    const int it = g.items[u], k = it >> 4;
    double v;
    switch (it & 15) {
      case F_TT: v = lin[k].H_tt[6 * rr + cc]; break;
      case F_SS: v = lin[k].H_ss[6 * rr + cc]; break;
      case F_ST: v = lin[k].H_ts[6 * cc + rr]; break;  // rows of s, columns of t: the transpose
      case F_TS: v = lin[k].H_ts[6 * rr + cc]; break;
      case PRIOR: v = pc[PRIOR_STRIDE * k + 6 * rr + cc]; break;
      case B_II: v = bc[BETWEEN_STRIDE * k + 12 * rr + cc]; break;
      case B_JJ: v = bc[BETWEEN_STRIDE * k + 12 * (rr + 6) + cc + 6]; break;
      case B_JI: v = bc[BETWEEN_STRIDE * k + 12 * (rr + 6) + cc]; break;
      case B_IJ: v = bc[BETWEEN_STRIDE * k + 12 * rr + cc + 6]; break;
      case VPRIOR:
      case VB_II:
      case VB_JJ:
      case VB_JI:
      case VB_IJ: {  // a VELOCITY's rows and columns 3..5: nothing
        const int d = nav::node_dim(nav::kind_of(g.nav, hi)), kd = it & 15;
        if (rr >= d || cc >= d) continue;
        if (kd == VPRIOR) v = g.nav.vpc[nav::VPRIOR_STRIDE * k + 6 * rr + cc];
        else v = g.nav.vbc[nav::VBETWEEN_STRIDE * k + 12 * (rr + (kd == VB_JJ || kd == VB_JI ? 6 : 0)) + cc + (kd == VB_JJ || kd == VB_IJ ? 6 : 0)];
        break;
      }
      case IMU: {
        const int q = k >> 5, rs = (k & 31) / 5, cs = (k & 31) % 5;
        if (rr >= nav::imu_width(rs) || cc >= nav::imu_width(cs)) continue;
        v = g.nav.ic[(size_t)nav::IMU_STRIDE * q + nav::IMU_W * (nav::imu_offset(rs) + rr) + nav::imu_offset(cs) + cc];
        break;
      }
      default:  // DAMP: the diagonal, and no other entry of the block
        if (rr != cc) continue;
        v = g.dd[6 * k + rr];
        break;
    }
    s += v;
  }
  return s;
}

// entry r of b
GLIM_AMD_LM_HD inline double assemble_rhs(const Graph& g, const glim_amd_linearized6* lin, const double* pc, const double* bc, int r) {
  const int a = r / 6, rr = r - 6 * a;
  const int e = tri(a) + a;
  double s = 0.0;
  for (int u = g.first[e]; u < g.first[e + 1]; u++) {
    const int it = g.items[u], k = it >> 4;
    double v;
    switch (it & 15) {
      case F_TT: v = lin[k].b_t[rr]; break;
      case F_SS: v = lin[k].b_s[rr]; break;
      case PRIOR: v = pc[PRIOR_STRIDE * k + 36 + rr]; break;
      case B_II: v = bc[BETWEEN_STRIDE * k + 144 + rr]; break;
      case B_JJ: v = bc[BETWEEN_STRIDE * k + 144 + 6 + rr]; break;
      case VPRIOR:
      case VB_II:
      case VB_JJ: {
        const int kd = it & 15;
        if (rr >= nav::node_dim(nav::kind_of(g.nav, a))) continue;
        v = kd == VPRIOR ? g.nav.vpc[nav::VPRIOR_STRIDE * k + 36 + rr] : g.nav.vbc[nav::VBETWEEN_STRIDE * k + 144 + (kd == VB_JJ ? 6 : 0) + rr];
        break;
      }
      case IMU: {
        const int q = k >> 5, rs = (k & 31) / 5;
        if (rr >= nav::imu_width(rs)) continue;
        v = g.nav.ic[(size_t)nav::IMU_STRIDE * q + nav::IMU_W * nav::IMU_W + nav::imu_offset(rs) + rr];
        break;
      }
      default: continue;  // DAMP: nothing
    }
    s += v;
  }
  return s;
}

// entry u of the solve's matrix from a kept system: H + lambda I in the triangle, -b in row n
GLIM_AMD_LM_HD inline double solve_load(const double* S, int n, double lambda, int u, int i, int j) {
  if (i == n) return -S[u];
  return i == j ? S[u] + lambda : S[u];
}

// the pivot of column j: the square root, or a value that is not > 0 (a failed solve)
GLIM_AMD_LM_HD inline double chol_pivot(const double* W, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double* row = W + tri(j);
  double d = row[j];
  GLIM_AMD_BUNDLE_UNROLL
  for (int k = 0; k < j; k++) d -= row[k] * row[k];
  if (!(d > 0.0) || !lm::finite(d)) return -1.0;
  return sqrt(d);
}
// entry (i, j), i > j, of L, column j's pivot in place
GLIM_AMD_LM_HD inline double chol_entry(const double* W, int i, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double *ri = W + tri(i), *rj = W + tri(j);
  double s = ri[j];
  GLIM_AMD_BUNDLE_UNROLL
  for (int k = 0; k < j; k++) s -= ri[k] * rj[k];
  return s / rj[j];
}

// W (H + lambda I, -b) -> L and y in place, delta.  false: a failed solve (delta is then zero)
GLIM_AMD_LM_HD inline bool solve(double* W, int n, double* delta) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int i = 0; i < n; i++) delta[i] = 0.0;
  for (int j = 0; j < n; j++) {
    const double d = chol_pivot(W, j);
    if (!(d > 0.0)) return false;
    W[tri(j) + j] = d;
    for (int i = j + 1; i <= n; i++) W[tri(i) + j] = chol_entry(W, i, j);
  }
  double* s = W + tri(n);
  for (int k = n - 1; k >= 0; k--) {
    const double* rk = W + tri(k);
    delta[k] = s[k] / rk[k];
    for (int i = 0; i < k; i++) s[i] -= rk[i] * delta[k];
  }
  return true;
}

// the cost from its parts: ((((factors + priors) + betweens) + vector priors) + vector betweens) + IMU.  A sum from +0.0 is never -0.0, so a
// graph without the last three (their sums are +0.0) has the bits of (factors + priors) + betweens
GLIM_AMD_LM_HD inline double total_cost(double fcost, double pcost, double bcost, double vpcost, double vbcost, double icost) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return ((((fcost + pcost) + bcost) + vpcost) + vbcost) + icost;
}

// the rule's scalar part: lm::decide on the cost, and the bundle's own bookkeeping.  The evaluation at the candidate gave (cost, fcost, pcost,
// bcost, inliers).  true: the candidate is kept
GLIM_AMD_LM_HD inline bool decide(const lm::Params& p, int F, Scalars& s, double cost, double fcost, double pcost, double bcost, double inliers, double vpcost = 0.0,
                                  double vbcost = 0.0, double icost = 0.0) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const bool seen = F == 0 || inliers >= 1.0;
  s.trial_cost = cost;
  const bool keep = lm::decide(p, s.lambda, s.solve_ok, s.started, s.iterations, s.trials, s.status, s.accepted, s.cost, cost, seen);
  if (keep) {
    s.cost = cost;
    s.fcost = fcost;
    s.pcost = pcost;
    s.bcost = bcost;
    s.inliers = inliers;
    s.vpcost = vpcost;
    s.vbcost = vbcost;
    s.icost = icost;
  }
  return keep;
}

// the state before round 0: the next evaluation is at the initial poses (their T_f: relative_pose, by the caller)
GLIM_AMD_LM_HD inline void init(const lm::Params& p, const double* X_init, Problem& pr) {
  for (int i = 0; i < 12 * pr.g.N; i++) pr.X[i] = pr.cand[i] = X_init[i];
  for (int i = 0; i < 6 * pr.g.N; i++) pr.delta[i] = 0.0;
  for (int i = 0; i < lm::RECORD * pr.g.F; i++) pr.rec[i] = 0.0;
  for (int i = 0; i < system_doubles(6 * pr.g.N); i++) pr.S[i] = 0.0;
  if (pr.wk)
    for (int q = 0; q < pr.g.Q; q++) pr.wk[q] = 1.0;
  Scalars& s = *pr.s;
  s.lambda = p.lambda_initial;
  s.cost = s.fcost = s.pcost = s.bcost = s.inliers = s.trial_cost = s.vpcost = s.vbcost = s.icost = 0.0;
  s.solve_ok = 1;
  s.started = s.iterations = s.trials = s.accepted = 0;
  s.status = lm::RUNNING;
}

// One round: `recs` are the F records evaluated at pr.Tf (= the relative poses of pr.cand).  Updates what is kept, the status, the candidate of
// the next round and its T_f.
GLIM_AMD_LM_HD inline void step(const lm::Params& p, Problem& pr, const double* recs) {
  const Graph& g = pr.g;
  Scalars& s = *pr.s;
  const int n = 6 * g.N, nsys = system_doubles(n);
  if (s.status != lm::RUNNING) return;
  s.accepted = 0;
  if (!lm::all_finite(recs, lm::RECORD * g.F) || !lm::all_finite(pr.cand, 12 * g.N)) {
    s.status = lm::NUMERIC;
    return;
  }
  for (int f = 0; f < g.F; f++) expand_factor(recs, pr.Tf, f, pr.lin);
  for (int q = 0; q < g.P; q++) prior_term(g, pr.cand, q, pr.pc);
  for (int q = 0; q < g.Q; q++) between_term(g, pr.cand, q, pr.bc, pr.wt);
  for (int q = 0; q < g.nav.VP; q++) nav::vector_prior_term(g.nav, pr.cand, q);
  for (int q = 0; q < g.nav.VB; q++) nav::vector_between_term(g.nav, pr.cand, q);
  for (int q = 0; q < g.nav.I; q++) nav::imu_term(g.nav, pr.cand, q);
  const double fcost = sum_ascending(recs + 1, g.F, lm::RECORD), inliers = sum_ascending(recs, g.F, lm::RECORD);
  const double pcost = sum_ascending(pr.pc + 42, g.P, PRIOR_STRIDE), bcost = sum_ascending(pr.bc + 156, g.Q, BETWEEN_STRIDE);
  const double vpcost = g.nav.VP ? sum_ascending(g.nav.vpc + 42, g.nav.VP, nav::VPRIOR_STRIDE) : 0.0;
  const double vbcost = g.nav.VB ? sum_ascending(g.nav.vbc + 156, g.nav.VB, nav::VBETWEEN_STRIDE) : 0.0;
  const double icost = g.nav.I ? sum_ascending(g.nav.ic + nav::IMU_STRIDE - 1, g.nav.I, nav::IMU_STRIDE) : 0.0;
  const double cost = total_cost(fcost, pcost, bcost, vpcost, vbcost, icost);
  for (int r = 0; r < n; r++)
    for (int c = 0; c <= r; c++) pr.W[tri(r) + c] = assemble_entry(g, pr.lin, pr.pc, pr.bc, r, c);
  for (int r = 0; r < n; r++) pr.W[tri(n) + r] = assemble_rhs(g, pr.lin, pr.pc, pr.bc, r);
  if (!lm::all_finite(pr.W, nsys) || !lm::finite(cost)) {
    s.status = lm::NUMERIC;
    return;
  }
  if (decide(p, g.F, s, cost, fcost, pcost, bcost, inliers, vpcost, vbcost, icost)) {
    for (int i = 0; i < 12 * g.N; i++) pr.X[i] = pr.cand[i];
    for (int i = 0; i < lm::RECORD * g.F; i++) pr.rec[i] = recs[i];
    for (int i = 0; i < nsys; i++) pr.S[i] = pr.W[i];
    if (pr.wt && pr.wk)
      for (int q = 0; q < g.Q; q++) pr.wk[q] = pr.wt[q];
  }
  if (s.status != lm::RUNNING) return;
  for (int i = 0; i <= n; i++)
    for (int j = 0; j < (i < n ? i + 1 : n); j++) pr.W[tri(i) + j] = solve_load(pr.S, n, s.lambda, tri(i) + j, i, j);
  s.solve_ok = solve(pr.W, n, pr.delta) ? 1 : 0;
  for (int k = 0; k < g.N; k++) {
    if (s.solve_ok) {
      nav::retract_node(nav::kind_of(g.nav, k), pr.X + 12 * k, pr.delta + 6 * k, pr.cand + 12 * k);
    } else {
      for (int i = 0; i < 12; i++) pr.cand[12 * k + i] = pr.X[12 * k + i];
    }
  }
  if (!lm::all_finite(pr.cand, 12 * g.N)) {
    s.status = lm::NUMERIC;
    return;
  }
  for (int f = 0; f < g.F; f++) relative_pose(pr.cand, g.ft, g.fs, f, pr.Tf);
}

}  // namespace bundle_lm
}  // namespace glim_amd
