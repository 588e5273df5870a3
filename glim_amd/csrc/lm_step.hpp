// lm_step.hpp -- the step rule of the on-device GICP fine registration (include/glim_amd.h "GICP fine registration"): ONE function, host and
// device.  The decide kernels of gicp_align.hip and vgicp_align.hip call it once per round and problem; tests/cpp/test_lm_step.cpp compiles it with a plain C++ compiler
// and runs the same statements on the CPU.  The header includes nothing of the project.  The rule's scalar part (decide) and the dense solve
// (solve_dense<N>) are also what the CT loop (ct_lm_step.hpp) and the sub-map bundle (bundle_lm_step.hpp) call: they exist here, once.
//
// Everything is FP64 with contraction off.  The rule is upstream RECALL of GTSAM's LevenbergMarquardtOptimizer in fixed-lambda-factor mode
// (diagonalDamping off), which gtsam_points' LevenbergMarquardtOptimizerExt follows; GTSAM is not in the reference tree.
//
//   record       the compact record of the factor at a pose: [num_inliers, error, 21 upper entries of H_ss (row-major), 6 of b_s].  "The error at
//                a pose" is the `error` field of the LINEARISING evaluation at that pose: a trial is one search, not two.
//   solve        (H_ss + lambda I) delta = -b_s by 6 x 6 Cholesky (tests/ct_restatement.py::gn_step's sign).  A pivot that is not > 0 is a FAILED
//                solve; the candidate is then the kept pose and the trial is rejected.
//   retract      T' = T Exp(delta), omega first: R = I + a W + b W^2, t = (I + b W + c W^2) v, a = sin th / th, b = (1 - cos th) / th^2,
//                c = (th - sin th) / th^3, their Taylor series (three terms) below th = 0.02.  The rotation is re-orthonormalised NEVER: the
//                pose travels as 12 doubles, and the pose returned is bit for bit the pose its record was evaluated at.
//   round 0      the record at the initial pose: always kept, not an iteration and not a trial.  Zero inliers: NO_CORRESPONDENCES, the pose
//                returned is the initial pose.
//   a trial      the record at the candidate.  trials += 1.  ACCEPT iff the solve succeeded, the candidate has >= 1 inlier and e_new < e_cur.
//     accept     T <- T', the record is kept, lambda <- max(lambda / lambda_factor, lambda_lower_bound), iterations += 1;
//                CONVERGED if e_cur - e_new <= absolute_error_tol / error_scale or (e_cur - e_new) / e_cur <= relative_error_tol.
//     reject     lambda <- lambda * lambda_factor; LAMBDA_BOUND if lambda > lambda_upper_bound.  The kept record and pose are unchanged; the next
//                candidate is solved from the kept record with the new lambda.
//   budgets      after a round that did not end otherwise: MAX_ITERATIONS at iterations >= max_iterations, then MAX_TRIALS at trials >= max_trials.
//   non-finite   a non-finite record, or a non-finite pose (initial or candidate): NUMERIC, the last kept pose is returned.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define GLIM_AMD_LM_HD __host__ __device__
#else
#define GLIM_AMD_LM_HD
#endif

namespace glim_amd {
namespace lm {

enum { RUNNING = 0, CONVERGED = 1, MAX_ITERATIONS = 2, MAX_TRIALS = 3, LAMBDA_BOUND = 4, NO_CORRESPONDENCES = 5, NUMERIC = 6 };
constexpr int RECORD = 29;             // doubles of a compact record
constexpr double EXP_SERIES = 0.02;    // rad below which the coefficients of Exp are their series (truncation < 1e-16 there)

// the layout of glim_amd_lm_params; max_trials is the resolved budget here (never 0 = "twice max_iterations")
struct Params {
  double lambda_initial, lambda_factor, lambda_upper_bound, lambda_lower_bound, relative_error_tol, absolute_error_tol;
  int max_iterations, max_trials;
  double error_scale;
};

// one problem: what is kept, and the candidate the next round evaluates
struct State {
  double T[12];        // the kept pose (row-major 3 x 4)
  double rec[RECORD];  // its record
  double lambda;       // of the candidate below
  double cand[12];     // the pose of the next evaluation
  double delta[6];     // the step that gave it (zero after a failed solve and in round 0)
  int solve_ok, started, iterations, trials, status, accepted;  // accepted: of the last round
};

GLIM_AMD_LM_HD inline bool finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // false for NaN
GLIM_AMD_LM_HD inline bool all_finite(const double* v, int n) {
  bool ok = true;
  for (int i = 0; i < n; i++) ok = ok && finite(v[i]);
  return ok;
}

// (H + lambda I) delta = -b, H symmetric N x N given as its upper triangle in row-major order.  L: N * N + N doubles of workspace (the Cholesky
// factor, then the forward substitution).  false: a pivot of the factor is not > 0 (delta is then zero)
template <int N>
GLIM_AMD_LM_HD inline bool solve_dense(const double* upper, const double* b, double lambda, double* delta, double* L) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  int u = 0;
  for (int r = 0; r < N; r++)
    for (int c = r; c < N; c++, u++) L[N * c + r] = upper[u] + (r == c ? lambda : 0.0);  // lower triangle
  for (int i = 0; i < N; i++) delta[i] = 0.0;
  for (int j = 0; j < N; j++) {
    double d = L[N * j + j];
    for (int k = 0; k < j; k++) d -= L[N * j + k] * L[N * j + k];
    if (!(d > 0.0) || !finite(d)) return false;
    d = sqrt(d);
    L[N * j + j] = d;
    for (int i = j + 1; i < N; i++) {
      double s = L[N * i + j];
      for (int k = 0; k < j; k++) s -= L[N * i + k] * L[N * j + k];
      L[N * i + j] = s / d;
    }
  }
  double* y = L + N * N;
  for (int i = 0; i < N; i++) {
    double s = -b[i];
    for (int k = 0; k < i; k++) s -= L[N * i + k] * y[k];
    y[i] = s / L[N * i + i];
  }
  for (int i = N - 1; i >= 0; i--) {
    double s = y[i];
    for (int k = i + 1; k < N; k++) s -= L[N * k + i] * delta[k];
    delta[i] = s / L[N * i + i];
  }
  return true;
}

// the solve from a compact record
GLIM_AMD_LM_HD inline bool solve(const double* rec, double lambda, double* delta) {
  double L[36 + 6];
  return solve_dense<6>(rec + 2, rec + 23, lambda, delta, L);
}

// out = T Exp(xi), xi = (omega, v)
GLIM_AMD_LM_HD inline void retract(const double* T, const double* xi, double* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double wx = xi[0], wy = xi[1], wz = xi[2];
  const double t2 = (wx * wx + wy * wy) + wz * wz;
  const double th = sqrt(t2);
  double a, b, c;
  if (th < EXP_SERIES) {
    a = 1.0 - t2 / 6.0 + t2 * t2 / 120.0;
    b = 0.5 - t2 / 24.0 + t2 * t2 / 720.0;
    c = 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0;
  } else {
    const double s = sin(th), co = cos(th);
    a = s / th;
    b = (1.0 - co) / t2;
    c = (th - s) / (t2 * th);
  }
  const double W[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
  double E[12];
  for (int r = 0; r < 3; r++) {
    double tr = 0.0;
    for (int k = 0; k < 3; k++) {
      const double w2 = (W[3 * r] * W[k] + W[3 * r + 1] * W[3 + k]) + W[3 * r + 2] * W[6 + k];
      const double I = r == k ? 1.0 : 0.0;
      E[4 * r + k] = (I + a * W[3 * r + k]) + b * w2;
      tr += ((I + b * W[3 * r + k]) + c * w2) * xi[3 + k];
    }
    E[4 * r + 3] = tr;
  }
  for (int r = 0; r < 3; r++) {
    for (int k = 0; k < 3; k++) out[4 * r + k] = (T[4 * r] * E[k] + T[4 * r + 1] * E[4 + k]) + T[4 * r + 2] * E[8 + k];
    out[4 * r + 3] = ((T[4 * r] * E[3] + T[4 * r + 1] * E[7]) + T[4 * r + 2] * E[11]) + T[4 * r + 3];
  }
}

// the state before round 0: the next evaluation is at the initial pose
GLIM_AMD_LM_HD inline void init(const Params& p, const double* T_init, State& s) {
  for (int i = 0; i < 12; i++) s.T[i] = s.cand[i] = T_init[i];
  for (int i = 0; i < RECORD; i++) s.rec[i] = 0.0;
  for (int i = 0; i < 6; i++) s.delta[i] = 0.0;
  s.lambda = p.lambda_initial;
  s.solve_ok = 1;
  s.started = s.iterations = s.trials = s.accepted = 0;
  s.status = RUNNING;
}

// The scalar part of the rule, for every loop of the family (step below, ct_lm::step, bundle_lm::decide): round 0 and the trial counting, the
// accept condition and both lambda updates, the statuses and the budgets, on the progress words of a state.  e_cur: the error at what is kept,
// e_new and has_inliers: of the evaluation at the candidate.  true: the candidate is kept (the caller then copies what it keeps).
GLIM_AMD_LM_HD inline bool decide(const Params& p, double& lambda, int solve_ok, int& started, int& iterations, int& trials, int& status, int& accepted, double e_cur,
                                  double e_new, bool has_inliers) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  bool keep = false;
  if (!started) {
    started = 1;
    keep = true;
  } else {
    trials += 1;
    if (solve_ok && has_inliers && e_new < e_cur) {
      keep = true;
      const double l = lambda / p.lambda_factor;
      lambda = l > p.lambda_lower_bound ? l : p.lambda_lower_bound;
      iterations += 1;
      const double d = e_cur - e_new;
      if (d <= p.absolute_error_tol / p.error_scale || d / e_cur <= p.relative_error_tol) status = CONVERGED;
    } else {
      lambda = lambda * p.lambda_factor;
      if (!(lambda <= p.lambda_upper_bound)) status = LAMBDA_BOUND;
    }
  }
  if (keep) {
    accepted = 1;
    if (!has_inliers) {  // round 0 only: a trial without inliers is never kept
      status = NO_CORRESPONDENCES;
      return keep;
    }
  }
  if (status == RUNNING && iterations >= p.max_iterations) status = MAX_ITERATIONS;
  if (status == RUNNING && trials >= p.max_trials) status = MAX_TRIALS;
  return keep;
}

// One round: `rec` is the record evaluated at s.cand.  Updates what is kept, the status, and the candidate of the next round.
GLIM_AMD_LM_HD inline void step(const Params& p, State& s, const double* rec) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (s.status != RUNNING) return;
  s.accepted = 0;
  if (!all_finite(rec, RECORD) || !all_finite(s.cand, 12)) {
    s.status = NUMERIC;
    return;
  }
  if (decide(p, s.lambda, s.solve_ok, s.started, s.iterations, s.trials, s.status, s.accepted, s.rec[1], rec[1], rec[0] >= 1.0)) {
    for (int i = 0; i < 12; i++) s.T[i] = s.cand[i];  // (round 0: the initial pose onto itself)
    for (int i = 0; i < RECORD; i++) s.rec[i] = rec[i];
  }
  if (s.status != RUNNING) return;
  s.solve_ok = solve(s.rec, s.lambda, s.delta) ? 1 : 0;
  if (s.solve_ok) {
    retract(s.T, s.delta, s.cand);
  } else {
    for (int i = 0; i < 12; i++) s.cand[i] = s.T[i];
  }
  if (!all_finite(s.cand, 12)) s.status = NUMERIC;
}

}  // namespace lm
}  // namespace glim_amd
