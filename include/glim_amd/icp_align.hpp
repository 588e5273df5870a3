// icp_align.hpp -- header-only C++17 mirror, over the C ABI (glim_amd.h "ICP factors", "ICP fine registration"), of gtsam_points::IntegratedICPFactor
// and of the loop GLIM's manual loop closing runs over it when a cloud carries no covariances (manual_loop_close_modal.cpp:485-490: Levenberg-
// Marquardt capped at 200 iterations): problems in, poses out, the whole batch in one call.
//
//   glim_amd::NearestNeighborSearchGPU tree(target, 1.0);                                   // the GICP factor's index: no covariances needed
//   auto r = glim_amd::align_icp(tree, *source, T_init, 1.0);                               // one problem, point-to-point
//   auto rs = glim_amd::align_icp({{&tree, source.get(), T0, 1.0}, {&tree, other.get(), T1, 1.0}}, glim_amd::ICPParams(), /*point_to_plane=*/true);
#pragma once

#include <algorithm>
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

#include "gicp_align.hpp"

namespace glim_amd {

// gtsam_points::IntegratedICPFactor (point-to-point) / IntegratedPointToPlaneICPFactor over the search index of the target cloud.  The forms of
// IntegratedGICPFactor: binary (target_key, source_key, ...) and unary (fixed_target_pose, source_key, ...), an optional shared target tree.
class IntegratedICPFactor {
public:
  using shared_ptr = std::shared_ptr<IntegratedICPFactor>;
  IntegratedICPFactor(Key target_key, Key source_key, PointCloudGPU::ConstPtr target, PointCloudGPU::ConstPtr source,
                      NearestNeighborSearchGPU::ConstPtr target_tree = nullptr, bool use_point_to_plane = false)
      : is_binary_(true), plane_(use_point_to_plane), target_key_(target_key), source_key_(source_key), source_(std::move(source)),
        tree_(target_tree ? std::move(target_tree) : std::make_shared<NearestNeighborSearchGPU>(std::move(target))) {}
  IntegratedICPFactor(const Isometry3d& fixed_target_pose, Key source_key, PointCloudGPU::ConstPtr target, PointCloudGPU::ConstPtr source,
                      NearestNeighborSearchGPU::ConstPtr target_tree = nullptr, bool use_point_to_plane = false)
      : is_binary_(false), plane_(use_point_to_plane), target_key_(0), source_key_(source_key), fixed_target_pose_(fixed_target_pose),
        source_(std::move(source)), tree_(target_tree ? std::move(target_tree) : std::make_shared<NearestNeighborSearchGPU>(std::move(target))) {}

  void set_max_correspondence_distance(double d) { max_correspondence_distance_ = d; }
  void set_num_threads(int) {}  // accepted for source compatibility; the device has no thread knob
  std::vector<Key> keys() const { return is_binary_ ? std::vector<Key>{target_key_, source_key_} : std::vector<Key>{source_key_}; }
  std::size_t dim() const { return 6; }
  bool is_binary() const { return is_binary_; }
  bool use_point_to_plane() const { return plane_; }
  std::uint32_t flags() const { return (is_binary_ ? GLIM_AMD_FACTOR_BINARY : 0u) | (plane_ ? GLIM_AMD_ICP_POINT_TO_PLANE : 0u); }
  Isometry3d calc_delta(const Values& values) const {
    const Isometry3d& Ts = values.at(source_key_);
    return (is_binary_ ? values.at(target_key_) : fixed_target_pose_).inverse() * Ts;
  }
  const LinearizedSystem6& linearize(const Values& values) {
    const Isometry3d d = calc_delta(values);
    check(glim_amd_icp_linearize(tree_->handle(), source_->handle(), d.m.data(), max_correspondence_distance_, flags(), &linearized_),
          "IntegratedICPFactor::linearize");
    num_inliers_ = linearized_.num_inliers;
    return linearized_;
  }
  double error(const Values& values) {
    const Isometry3d d = calc_delta(values);
    double e = 0.0;
    check(glim_amd_icp_error(tree_->handle(), source_->handle(), d.m.data(), max_correspondence_distance_, flags(), &e, &num_inliers_),
          "IntegratedICPFactor::error");
    return e;
  }
  double inlier_fraction() const { return (double)num_inliers_ / (double)std::max<std::size_t>(1, source_->size()); }
  const LinearizedSystem6& linearized() const { return linearized_; }
  const NearestNeighborSearchGPU::ConstPtr& target_tree() const { return tree_; }

private:
  bool is_binary_, plane_;
  Key target_key_, source_key_;
  Isometry3d fixed_target_pose_;
  PointCloudGPU::ConstPtr source_;
  NearestNeighborSearchGPU::ConstPtr tree_;  // keeps the target alive
  double max_correspondence_distance_ = 1.0;
  std::int64_t num_inliers_ = 0;
  LinearizedSystem6 linearized_{};
};

struct ICPParams : LMParams {  // glim_amd_icp_align_default_params
  ICPParams() { max_iterations = 200; }
};

using ICPAlignProblem = AlignProblem<NearestNeighborSearchGPU>;

inline std::vector<AlignResult> align_icp(const std::vector<ICPAlignProblem>& problems, const LMParams& params = ICPParams(), bool point_to_plane = false) {
  const std::size_t n = problems.size();
  std::vector<const glim_amd_nn_index*> targets(n);
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
  check(glim_amd_icp_align_batch(targets.data(), sources.data(), T.data(), dist.data(), point_to_plane ? GLIM_AMD_ICP_POINT_TO_PLANE : 0u, (std::int32_t)n, &p,
                                 raw.data()),
        "align_icp");
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
    check(glim_amd_expand_compact(raw[i].compact, raw[i].T_target_source, 0, &lin), "align_icp");
    for (int k = 0; k < 36; k++) r.information[k] = lin.H_ss[k];
  }
  return out;
}

inline AlignResult align_icp(const NearestNeighborSearchGPU& target, const PointCloudGPU& source, const Isometry3d& T_init, double max_correspondence_distance,
                             const LMParams& params = ICPParams(), bool point_to_plane = false) {
  return align_icp(std::vector<ICPAlignProblem>{{&target, &source, T_init, max_correspondence_distance}}, params, point_to_plane)[0];
}

}  // namespace glim_amd
