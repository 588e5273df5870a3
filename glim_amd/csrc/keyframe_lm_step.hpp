// keyframe_lm_step.hpp -- what the scan-to-keyframes VGICP registration (include/glim_amd.h "Scan-to-keyframes VGICP registration") adds to the
// step rule of lm_step.hpp, ONCE, for host and device: one pose X per problem, M unary VGICP factors with FIXED target poses P_f, an optional
// prior on X.  vgicp_align.hip's keyframe decide kernel runs the functions below across one wavefront, an owner per value;
// tests/cpp/test_keyframe_lm_step.cpp compiles the header alone with a plain C++ compiler and runs step() on the CPU;
// tests/keyframe_restatement.py restates it in NumPy.  Plain C++ apart from the host/device macro.  Everything is FP64 with contraction off.
//
//   poses      factor f is evaluated at T_f = P_f^-1 X (target_inverse once per call, factor_pose per round: ct_se3's inverse and compose).  With
//              right perturbation X Exp(d) gives T_f Exp(d): every factor's H_ss and b_s are already expressed in d of X, and simply add.
//   sum        entry t of the problem's record is ((+0.0 + r_0[t]) + r_1[t]) + ... over its factors by ascending index (sum_entry): 29 independent
//              ordered sums.  A sum of compact records is a compact record, so the rule is lm::step, unchanged, on the sum.
//   prior      r = Log(P^-1 X), J = J_r(r)^-1 (ct_se3::prior_residual); J^T L J, J^T L r and r^T L r by bundle_lm::term_products
//              (prior_contribution: the 21 upper entries of J^T L J, then the 6 of J^T L r, then r^T L r).  add_prior adds it LAST, to H, b and the
//              error; never to the inlier count, so a prior alone makes no candidate acceptable.
//   non-finite a T_f that is not finite (a P_f or an X that is not) ends the problem with NUMERIC, as a non-finite record does.
#pragma once
#include "bundle_lm_step.hpp"

namespace glim_amd {
namespace keyframe_lm {

constexpr int MAX_TARGETS = 64;
constexpr int PRIOR = 21 + 6 + 1;   // doubles of a prior's contribution
constexpr int PRIOR_TERM = 12 + 36; // doubles of a prior as the loop carries it: P (row-major 3 x 4), then the information (row-major 6 x 6)

GLIM_AMD_LM_HD inline void target_inverse(const double* P, double* Pinv) { ct_se3::se3_inverse(P, Pinv); }

// T_f = P_f^-1 X.  One definition, never inlined: the kernel of round 0 and the decide kernel run the same machine code
GLIM_AMD_BUNDLE_ITEM void factor_pose(const double* Pinv, const double* X, double* Tf) { ct_se3::se3_compose(Pinv, X, Tf); }

// entry t of the sum of M records (29 doubles apart), ascending from +0.0
GLIM_AMD_LM_HD inline double sum_entry(const double* recs, int M, int t) { return bundle_lm::sum_ascending(recs + t, M, lm::RECORD); }

// term: P | information.  out: PRIOR doubles
GLIM_AMD_BUNDLE_ITEM void prior_contribution(const double* term, const double* X, double* out) {
  double r[6], full[bundle_lm::PRIOR_STRIDE];
  const ct_se3::Mat6 Ji = ct_se3::prior_residual(term, X, r);
  bundle_lm::term_products(Ji.m, 6, term + 12, r, full);
  int u = 0;
  for (int a = 0; a < 6; a++)
    for (int b = a; b < 6; b++) out[u++] = full[6 * a + b];
  for (int a = 0; a < 7; a++) out[21 + a] = full[36 + a];
}

// entry t of the summed record with the prior's contribution added
GLIM_AMD_LM_HD inline double add_prior(double s, const double* c, int t) {
  if (t == 0) return s;
  if (t == 1) return s + c[27];
  return s + c[t - 2];  // the 21 of H, then the 6 of b: the order of the record
}

// One round of one problem in one thread, what the wavefront of the decide kernel does: `recs` are the M records evaluated at `Tf` (= the
// factor poses of s.cand).  term: the prior, or null.  sum: RECORD doubles, pc: PRIOR doubles (zero without a prior) -- the round's summed
// record and the prior's contribution, for whoever traces them.  Updates the state and, while the problem runs, the T_f of the next round.
// keyframe_decide_kernel (vgicp_align.hip) spreads THIS sequence over its lanes -- contribution, sums, the non-finite T_f, lm::step, fan-out, in
// this order: the two share the functions above, not the control flow, so a change to the sequence here is a change there.
GLIM_AMD_LM_HD inline void step(const lm::Params& p, lm::State& s, int M, const double* Pinv, const double* term, const double* recs, double* Tf, double* sum,
                                double* pc) {
  if (s.status != lm::RUNNING) return;
  for (int t = 0; t < PRIOR; t++) pc[t] = 0.0;
  if (term) prior_contribution(term, s.cand, pc);
  for (int t = 0; t < lm::RECORD; t++) {
    const double v = sum_entry(recs, M, t);
    sum[t] = term ? add_prior(v, pc, t) : v;
  }
  if (!lm::all_finite(Tf, 12 * M)) {
    s.accepted = 0;
    s.status = lm::NUMERIC;
    return;
  }
  lm::step(p, s, sum);
  if (s.status != lm::RUNNING) return;
  for (int f = 0; f < M; f++) factor_pose(Pinv + 12 * f, s.cand, Tf + 12 * f);
}

}  // namespace keyframe_lm
}  // namespace glim_amd
