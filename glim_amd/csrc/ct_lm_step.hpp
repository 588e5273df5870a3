// ct_lm_step.hpp -- the step rule of the on-device CT frame alignment (include/glim_amd.h "CT-GICP frame alignment"): ONE function, host and
// device.  ct_align.hip's decide kernel calls it once per round; tests/cpp/test_ct_lm_step.cpp compiles it with a plain C++ compiler and
// runs the same statements on the CPU; tests/ct_lm_restatement.py restates it in NumPy.  Plain C++ apart from the host/device macro.
//
// The problem is GLIM's continuous-time odometry frame (odometry_estimation_ct.cpp:158-195): 12 DoF, tangent order [X: omega v | Y: omega v],
// right perturbation, X = the pose at sweep begin, Y = at sweep end.  Everything is FP64 with contraction off.
//
//   record       the continuous-time factor's record at a pair: [num_inliers, error, 78 upper entries of the 12 x 12 H (row-major), 12 of b].
//   terms        location prior: r_p = Log(P^-1 X), J_p = J_r(r_p)^-1; adds k_p J_p^T J_p to H[X,X], k_p J_p^T r_p to b[X], k_p r_p^T r_p to the cost.
//                between: r_b = Log(D^-1 X^-1 Y), J = [-J_r(r_b)^-1 Ad((X^-1 Y)^-1) | J_r(r_b)^-1]; adds k_b J^T J, k_b J^T r_b, k_b r_b^T r_b.
//                A precision of 0 switches a term off (its pose is then not read).
//   system       the record with the terms added, in the record's layout; entry 1 is the total cost (error + prior cost) + between cost.
//                "The error at a pair" is that total cost from the LINEARISING evaluation at the pair: a trial is one search.
//   solve        (H + lambda I) delta = -b by 12 x 12 Cholesky.  A pivot that is not > 0 is a FAILED solve; the candidate is then the kept pair
//                and the trial is rejected.
//   retract      X' = X Exp(delta[0:6]), Y' = Y Exp(delta[6:12]) with lm::retract.  The rotations are re-orthonormalised NEVER.
//   the rest     round 0, accept / reject, the lambda updates, the statuses and the budgets are lm::decide of lm_step.hpp, CALLED with "the error"
//                read as that total cost; the solve is lm::solve_dense<12>, the terms' residuals and Jacobians ct_se3.hpp's.  See lm_step.hpp's head.
#pragma once
#include "ct_se3.hpp"
#include "lm_step.hpp"

namespace glim_amd {
namespace ct_lm {

constexpr int RECORD = 92;          // doubles of a record of the continuous-time factor
constexpr int SOLVE_WORK = 144 + 12;      // doubles of the workspace of solve(): the Cholesky factor, then the forward substitution
constexpr int WORK = RECORD + SOLVE_WORK;  // of step(): the candidate's system, then solve()'s (the between Jacobian lives there before the solve)

// the layout of glim_amd_ct_align_terms
struct Terms {
  double P[12], kp;  // location prior on X
  double D[12], kb;  // measurement of X^-1 Y
};

// what is kept, and the candidate the next round evaluates
struct State {
  double X[12], Y[12];        // the kept pair
  double rec[RECORD];         // the factor's record at it
  double sys[RECORD];         // the system at it: the record with the terms added, sys[1] = the total cost
  double cost_p, cost_b;      // the terms' costs at it
  double lambda;              // of the candidate below
  double candX[12], candY[12];
  double delta[12];           // the step that gave it (zero after a failed solve and in round 0)
  int solve_ok, started, iterations, trials, status, accepted;  // accepted: of the last round
};

GLIM_AMD_LM_HD inline int upper12(int r, int c) { return r * 12 - r * (r - 1) / 2 + (c - r); }  // r <= c

// sys = rec with the two terms at (X, Y) added; J: 72 doubles of workspace.  Returns the terms' costs.
GLIM_AMD_LM_HD inline void assemble(const Terms& t, const double* X, const double* Y, const double* rec, double* sys, double* J, double& cost_p, double& cost_b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  using namespace ct_se3;
  for (int i = 0; i < RECORD; i++) sys[i] = rec[i];
  cost_p = 0.0;
  cost_b = 0.0;
  if (t.kp > 0.0) {
    double r[6];
    const Mat6 Ji = prior_residual(t.P, X, r);
    GLIM_AMD_SE3_UNROLL
    for (int i = 0; i < 36; i++) J[i] = Ji.m[i];
    for (int a = 0; a < 6; a++) {
      for (int b = a; b < 6; b++) {
        double s = 0.0;
        for (int m = 0; m < 6; m++) s += J[6 * m + a] * J[6 * m + b];
        sys[2 + upper12(a, b)] += t.kp * s;
      }
      double g = 0.0;
      GLIM_AMD_SE3_UNROLL
      for (int m = 0; m < 6; m++) g += J[6 * m + a] * r[m];
      sys[80 + a] += t.kp * g;
    }
    double rr = 0.0;
    GLIM_AMD_SE3_UNROLL
    for (int m = 0; m < 6; m++) rr += r[m] * r[m];
    cost_p = t.kp * rr;
  }
  if (t.kb > 0.0) {
    double r[6];
    between_residual(t.D, X, Y, r, J);
    for (int a = 0; a < 12; a++) {
      for (int b = a; b < 12; b++) {
        double s = 0.0;
        for (int m = 0; m < 6; m++) s += J[12 * m + a] * J[12 * m + b];
        sys[2 + upper12(a, b)] += t.kb * s;
      }
      double g = 0.0;
      GLIM_AMD_SE3_UNROLL
      for (int m = 0; m < 6; m++) g += J[12 * m + a] * r[m];
      sys[80 + a] += t.kb * g;
    }
    double rr = 0.0;
    GLIM_AMD_SE3_UNROLL
    for (int m = 0; m < 6; m++) rr += r[m] * r[m];
    cost_b = t.kb * rr;
  }
  sys[1] = (rec[1] + cost_p) + cost_b;
}

// (H + lambda I) delta = -b from a system.  L: SOLVE_WORK doubles of workspace.  false: a pivot of the Cholesky factor is not > 0 (delta is then zero)
GLIM_AMD_LM_HD inline bool solve(const double* sys, double lambda, double* delta, double* L) {
  return lm::solve_dense<12>(sys + 2, sys + 80, lambda, delta, L);
}

// the state before round 0: the next evaluation is at the initial pair
GLIM_AMD_LM_HD inline void init(const lm::Params& p, const double* X_init, const double* Y_init, State& s) {
  for (int i = 0; i < 12; i++) {
    s.X[i] = s.candX[i] = X_init[i];
    s.Y[i] = s.candY[i] = Y_init[i];
    s.delta[i] = 0.0;
  }
  for (int i = 0; i < RECORD; i++) s.rec[i] = s.sys[i] = 0.0;
  s.cost_p = s.cost_b = 0.0;
  s.lambda = p.lambda_initial;
  s.solve_ok = 1;
  s.started = s.iterations = s.trials = s.accepted = 0;
  s.status = lm::RUNNING;
}

// One round: `rec` is the factor's record evaluated at (s.candX, s.candY).  Updates what is kept, the status, and the candidate of the next
// round.  work: WORK doubles.
GLIM_AMD_LM_HD inline void step(const lm::Params& p, const Terms& t, State& s, const double* rec, double* work) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (s.status != lm::RUNNING) return;
  s.accepted = 0;
  if (!lm::all_finite(rec, RECORD) || !lm::all_finite(s.candX, 12) || !lm::all_finite(s.candY, 12)) {
    s.status = lm::NUMERIC;
    return;
  }
  double* sys = work;
  double cp, cb;
  assemble(t, s.candX, s.candY, rec, sys, work + RECORD, cp, cb);
  if (!lm::all_finite(sys, RECORD)) {
    s.status = lm::NUMERIC;
    return;
  }
  if (lm::decide(p, s.lambda, s.solve_ok, s.started, s.iterations, s.trials, s.status, s.accepted, s.sys[1], sys[1], rec[0] >= 1.0)) {
    for (int i = 0; i < 12; i++) {  // (round 0: the initial pair onto itself)
      s.X[i] = s.candX[i];
      s.Y[i] = s.candY[i];
    }
    for (int i = 0; i < RECORD; i++) {
      s.rec[i] = rec[i];
      s.sys[i] = sys[i];
    }
    s.cost_p = cp;
    s.cost_b = cb;
  }
  if (s.status != lm::RUNNING) return;
  s.solve_ok = solve(s.sys, s.lambda, s.delta, work + RECORD) ? 1 : 0;
  if (s.solve_ok) {
    lm::retract(s.X, s.delta, s.candX);
    lm::retract(s.Y, s.delta + 6, s.candY);
  } else {
    for (int i = 0; i < 12; i++) {
      s.candX[i] = s.X[i];
      s.candY[i] = s.Y[i];
    }
  }
  if (!lm::all_finite(s.candX, 12) || !lm::all_finite(s.candY, 12)) s.status = lm::NUMERIC;
}

}  // namespace ct_lm
}  // namespace glim_amd
