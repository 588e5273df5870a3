// ct_align.hpp -- header-only C++17 mirror, over the C ABI (glim_amd.h "CT-GICP frame alignment"), of the frame optimisation of GLIM's LiDAR-only
// continuous-time odometry (odometry_estimation_ct.cpp:158-195): Levenberg-Marquardt over the sweep's begin pose X and end pose Y on
// { IntegratedCT_GICPFactor, PriorFactor<Pose3>(X), BetweenFactor<Pose3>(X, Y) }, one call and one host synchronisation.
//
//   glim_amd::IntegratedCT_GICPFactor factor(X_key, Y_key, target_ivox, frame, target_ivox);                  // :158-160
//   glim_amd::CtAlignTerms terms;
//   terms.location(predicted_T_world_lidar_begin, 1e-3);   // "location consistency"
//   terms.between(glim_amd::Isometry3d::Identity(), 1e3);  // "constant velocity"
//   auto r = glim_amd::align_ct(factor, values, terms);     // r.X, r.Y, r.linearized (the factor's Hessian at the estimate), r.status
#pragma once

#include <cstdint>

#include "gicp_align.hpp"
#include "gtsam_points_compat.hpp"

namespace glim_amd {

// GLIM's LM settings for this loop: lambdaInitial 1e-10, absoluteErrorTol 1e-2, lm_max_iterations 8; the rest are LMParams' defaults
inline LMParams ct_align_params() {
  LMParams p;
  p.lambda_initial = 1e-10;
  p.absolute_error_tol = 1e-2;
  p.max_iterations = 8;
  return p;
}

struct CtAlignTerms {
  glim_amd_ct_align_terms raw{};  // both precisions 0: no terms
  CtAlignTerms& location(const Isometry3d& T, double precision) {
    for (int k = 0; k < 12; k++) raw.T_location[k] = T.m[k];
    raw.location_precision = precision;
    return *this;
  }
  CtAlignTerms& between(const Isometry3d& T, double precision) {
    for (int k = 0; k < 12; k++) raw.T_between[k] = T.m[k];
    raw.between_precision = precision;
    return *this;
  }
};

struct CtAlignResult {
  Isometry3d X, Y;                    // the last kept pair
  glim_amd_ct_linearized linearized;  // the factor's record at it
  double cost = 0.0, location_cost = 0.0, between_cost = 0.0;
  std::int64_t num_inliers = 0;
  int iterations = 0, trials = 0;
  int status = 0;  // GLIM_AMD_ALIGN_*
  glim_amd_ct_align_result raw;
};

inline CtAlignResult align_ct(glim_amd_ct_gicp_factor* factor, const Isometry3d& X_init, const Isometry3d& Y_init, const CtAlignTerms& terms = CtAlignTerms(),
                              const LMParams& params = ct_align_params()) {
  const glim_amd_lm_params p = params.c();
  CtAlignResult r;
  check(glim_amd_ct_align(factor, X_init.m.data(), Y_init.m.data(), &terms.raw, &p, &r.raw), "align_ct");
  for (int k = 0; k < 12; k++) {
    r.X.m[k] = r.raw.X[k];
    r.Y.m[k] = r.raw.Y[k];
  }
  r.linearized = r.raw.linearized;
  r.cost = r.raw.cost;
  r.location_cost = r.raw.location_cost;
  r.between_cost = r.raw.between_cost;
  r.num_inliers = r.raw.linearized.num_inliers;
  r.iterations = r.raw.iterations;
  r.trials = r.raw.trials;
  r.status = r.raw.status;
  return r;
}

inline CtAlignResult align_ct(const IntegratedCT_GICPFactor& factor, const Values& values, const CtAlignTerms& terms = CtAlignTerms(),
                              const LMParams& params = ct_align_params()) {
  const std::vector<Key> keys = factor.keys();
  return align_ct(factor.handle(), values.at(keys[0]), values.at(keys[1]), terms, params);
}

}  // namespace glim_amd
