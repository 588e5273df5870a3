// keyframe_align.hpp -- header-only C++17 mirror, over the C ABI (glim_amd.h "Scan-to-keyframes VGICP registration"), of the LiDAR part of GLIM's
// frame-to-keyframes matching cost (odometry_estimation_gpu.cpp:150-165, 183-203): one unary IntegratedVGICPFactorGPU(fixed_target_pose,
// X(current), voxelmap, frame) per keyframe and per voxel-map level, all on the same pose -- Levenberg-Marquardt over that pose on the sum, in
// one call and one host synchronisation for a whole batch of frames.  LMParams and AlignResult are gicp_align.hpp's.
//
//   glim_amd::KeyframeAlignProblem pr{frame.get(), {}, T_world_frame_predicted};
//   for (auto& kf : keyframes)
//     for (auto& level : kf.voxelmaps) pr.targets.push_back({level.get(), kf.T_world_lidar});
//   auto r = glim_amd::align_to_keyframes({pr}, params, true)[0];   // r.T_target_source: T_world_frame; r.information: 6 x 6 H_ss of the sum there
#pragma once

#include <array>
#include <cstdint>
#include <vector>

#include "gicp_align.hpp"

namespace glim_amd {

struct KeyframeTarget {
  const GaussianVoxelMapGPU* voxelmap;
  Isometry3d T_world_target;  // fixed
};

struct KeyframePrior {  // PriorFactor<Pose3> on the pose
  Isometry3d T;
  std::array<double, 36> information;  // row-major 6 x 6, (omega, v) order; the upper triangle is read
};

struct KeyframeAlignProblem {
  const PointCloudGPU* source;
  std::vector<KeyframeTarget> targets;  // at most GLIM_AMD_KEYFRAME_ALIGN_MAX_TARGETS
  Isometry3d X_init;                    // T_world_source
  const KeyframePrior* prior = nullptr;
};

// surface_validation: IntegratedVGICPFactorGPU::set_enable_surface_validation, for every factor of the batch.  factor_records: when given, every
// factor's compact record (29 doubles) at the returned pose of its problem, in the order of the problems and their targets
inline std::vector<AlignResult> align_to_keyframes(const std::vector<KeyframeAlignProblem>& problems, const LMParams& params = LMParams(),
                                                   bool surface_validation = false, std::vector<double>* factor_records = nullptr) {
  const std::size_t n = problems.size();
  std::vector<const glim_amd_cloud*> sources(n);
  std::vector<std::int32_t> first(n + 1, 0);
  std::vector<const glim_amd_voxelmap*> targets;
  std::vector<double> P, X(12 * n);
  std::vector<glim_amd_bundle_prior> priors;
  for (std::size_t i = 0; i < n; i++) {
    sources[i] = problems[i].source->handle();
    for (const KeyframeTarget& t : problems[i].targets) {
      targets.push_back(t.voxelmap->handle());
      P.insert(P.end(), t.T_world_target.m.begin(), t.T_world_target.m.end());
    }
    first[i + 1] = (std::int32_t)targets.size();
    for (int k = 0; k < 12; k++) X[12 * i + k] = problems[i].X_init.m[k];
    if (problems[i].prior) {
      glim_amd_bundle_prior c{};
      c.pose = (std::int32_t)i;
      for (int k = 0; k < 12; k++) c.T[k] = problems[i].prior->T.m[k];
      for (int k = 0; k < 36; k++) c.information[k] = problems[i].prior->information[k];
      priors.push_back(c);
    }
  }
  std::vector<glim_amd_align_result> raw(n);
  if (factor_records) factor_records->assign(targets.size() * GLIM_AMD_COMPACT_DOUBLES, 0.0);
  const glim_amd_lm_params p = params.c();
  const std::uint32_t flags = surface_validation ? GLIM_AMD_FACTOR_SURFACE_VALIDATION : 0u;
  check(glim_amd_keyframe_align_batch(sources.data(), first.data(), targets.data(), P.data(), X.data(), priors.empty() ? nullptr : priors.data(),
                                      (std::int32_t)priors.size(), flags, (std::int32_t)n, &p, raw.data(), factor_records ? factor_records->data() : nullptr),
        "align_to_keyframes");
  std::vector<AlignResult> out(n);
  for (std::size_t i = 0; i < n; i++) {
    AlignResult& r = out[i];
    r.raw = raw[i];
    for (int k = 0; k < 12; k++) r.T_target_source.m[k] = raw[i].T_target_source[k];
    r.error = raw[i].error;
    r.num_inliers = raw[i].num_inliers;
    const std::size_t size = problems[i].source->size() * problems[i].targets.size();  // the inliers are summed over the factors
    r.inlier_fraction = size ? (double)raw[i].num_inliers / (double)size : 0.0;
    r.iterations = raw[i].iterations;
    r.trials = raw[i].trials;
    r.status = raw[i].status;
    glim_amd_linearized6 lin;
    check(glim_amd_expand_compact(raw[i].compact, raw[i].T_target_source, 0, &lin), "align_to_keyframes");
    for (int k = 0; k < 36; k++) r.information[k] = lin.H_ss[k];
  }
  return out;
}

}  // namespace glim_amd
