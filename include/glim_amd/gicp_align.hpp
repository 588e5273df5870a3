// gicp_align.hpp -- header-only C++17 mirror, over the C ABI (glim_amd.h "GICP fine registration"), of the loop GLIM runs wherever it refines a
// coarse T_target_source with "a few Levenberg-Marquardt iterations over one unary IntegratedGICPFactor" (global_mapping_pose_graph.cpp:386-426,
// global_mapping.cpp:393-426, manual_loop_close_modal.cpp:470-520, loose_initial_state_estimation.cpp): problems in, poses out, one call and one
// host synchronisation for the whole batch.
//
//   glim_amd::NearestNeighborSearchGPU tree(target, 1.0);                                   // candidate.target->tree
//   auto r = glim_amd::align_gicp(tree, *source, T_init, 1.0);                              // one problem
//   auto rs = glim_amd::align_gicp({{&tree, source.get(), T0, 1.0}, {&tree, other.get(), T1, 1.0}});   // many candidates, one launch sequence
//   if (r.inlier_fraction > 0.3) graph.add(BetweenFactor(..., r.T_target_source, r.information));      // 6 x 6 H_ss at the estimate
#pragma once

#include <array>
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

#include "gtsam_points_compat.hpp"

namespace glim_amd {

struct LMParams {  // gtsam::LevenbergMarquardtParams, the fields the loop reads
  double lambda_initial = 1e-5;
  double lambda_factor = 10.0;
  double lambda_upper_bound = 1e5;
  double lambda_lower_bound = 0.0;
  double relative_error_tol = 1e-5;
  double absolute_error_tol = 1e-5;
  int max_iterations = 10;
  int max_trials = 0;  // 0: twice max_iterations
  double error_scale = 1.0;
  glim_amd_lm_params c() const {
    glim_amd_lm_params p;
    p.lambda_initial = lambda_initial;
    p.lambda_factor = lambda_factor;
    p.lambda_upper_bound = lambda_upper_bound;
    p.lambda_lower_bound = lambda_lower_bound;
    p.relative_error_tol = relative_error_tol;
    p.absolute_error_tol = absolute_error_tol;
    p.max_iterations = max_iterations;
    p.max_trials = max_trials;
    p.error_scale = error_scale;
    return p;
  }
};

struct AlignResult {
  Isometry3d T_target_source;  // the last kept pose
  double error = 0.0;          // IntegratedGICPFactor::error there
  double inlier_fraction = 0.0;
  std::int64_t num_inliers = 0;
  int iterations = 0, trials = 0;
  int status = 0;                      // GLIM_AMD_ALIGN_*
  std::array<double, 36> information;  // H_ss of the factor at the estimate, row-major (global_mapping.cpp:423-424)
  glim_amd_align_result raw;
};

template <class Target>  // NearestNeighborSearchGPU or IncrementalVoxelMap
struct AlignProblem {
  const Target* target;
  const PointCloudGPU* source;
  Isometry3d T_init;
  double max_correspondence_distance;
};

namespace detail {
inline int align_batch(const glim_amd_nn_index* const* t, const glim_amd_cloud* const* s, const double* T, const double* d, std::int32_t n,
                       const glim_amd_lm_params* p, glim_amd_align_result* o) {
  return glim_amd_gicp_align_batch(t, s, T, d, n, p, o);
}
inline int align_batch(const glim_amd_ivox* const* t, const glim_amd_cloud* const* s, const double* T, const double* d, std::int32_t n,
                       const glim_amd_lm_params* p, glim_amd_align_result* o) {
  return glim_amd_gicp_align_batch_incremental(t, s, T, d, n, p, o);
}
}  // namespace detail

template <class Target>
inline std::vector<AlignResult> align_gicp(const std::vector<AlignProblem<Target>>& problems, const LMParams& params = LMParams()) {
  using Handle = std::remove_pointer_t<decltype(std::declval<const Target&>().handle())>;
  const std::size_t n = problems.size();
  std::vector<const Handle*> targets(n);
  std::vector<const glim_amd_cloud*> sources(n);
  std::vector<double> T(12 * n), dist(n);
  for (std::size_t i = 0; i < n; i++) {
    targets[i] = problems[i].target->handle();
    sources[i] = problems[i].source->handle();
    for (int k = 0; k < 12; k++) T[12 * i + k] = problems[i].T_init.m[k];
    dist[i] = problems[i].max_correspondence_distance;
  }
  std::vector<glim_amd_align_result> raw(n);
  const glim_amd_lm_params p = params.c();
  check(detail::align_batch(targets.data(), sources.data(), T.data(), dist.data(), (std::int32_t)n, &p, raw.data()), "align_gicp");
  std::vector<AlignResult> out(n);
  for (std::size_t i = 0; i < n; i++) {
    AlignResult& r = out[i];
    r.raw = raw[i];
    for (int k = 0; k < 12; k++) r.T_target_source.m[k] = raw[i].T_target_source[k];
    r.error = raw[i].error;
    r.num_inliers = raw[i].num_inliers;
    const std::size_t size = problems[i].source->size();
    r.inlier_fraction = size ? (double)raw[i].num_inliers / (double)size : 0.0;
    r.iterations = raw[i].iterations;
    r.trials = raw[i].trials;
    r.status = raw[i].status;
    glim_amd_linearized6 lin;
    check(glim_amd_expand_compact(raw[i].compact, raw[i].T_target_source, 0, &lin), "align_gicp");
    for (int k = 0; k < 36; k++) r.information[k] = lin.H_ss[k];
  }
  return out;
}

template <class Target>
inline AlignResult align_gicp(const Target& target, const PointCloudGPU& source, const Isometry3d& T_init, double max_correspondence_distance,
                              const LMParams& params = LMParams()) {
  return align_gicp(std::vector<AlignProblem<Target>>{{&target, &source, T_init, max_correspondence_distance}}, params)[0];
}

}  // namespace glim_amd
