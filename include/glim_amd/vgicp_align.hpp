// vgicp_align.hpp -- header-only C++17 mirror, over the C ABI (glim_amd.h "VGICP fine registration"), of the loop GLIM runs when it validates loop
// candidates with registration_type "VGICP" (global_mapping_pose_graph.cpp:405-417): "a few Levenberg-Marquardt iterations over one unary
// IntegratedVGICPFactor(Pose3(), 0, target->voxels, source)", then `error` and `inlier_fraction` -- problems in, poses out, one call and one host
// synchronisation for the whole batch.  LMParams and AlignResult are gicp_align.hpp's.
//
//   auto r = glim_amd::align_vgicp(*target_voxels, *source, T_init);                                       // one problem
//   auto rs = glim_amd::align_vgicp({{voxels_a.get(), source.get(), T0}, {voxels_b.get(), source.get(), T1}});   // many candidates, one launch sequence
//   if (r.inlier_fraction > 0.3) graph.add(BetweenFactor(..., r.T_target_source, r.information));          // 6 x 6 H_ss at the estimate
#pragma once

#include <cstdint>
#include <vector>

#include "gicp_align.hpp"

namespace glim_amd {

struct VGICPAlignProblem {
  const GaussianVoxelMapGPU* target;
  const PointCloudGPU* source;
  Isometry3d T_init;
};

// surface_validation: IntegratedVGICPFactorGPU::set_enable_surface_validation, for every problem of the batch
inline std::vector<AlignResult> align_vgicp(const std::vector<VGICPAlignProblem>& problems, const LMParams& params = LMParams(), bool surface_validation = false) {
  const std::size_t n = problems.size();
  std::vector<const glim_amd_voxelmap*> targets(n);
  std::vector<const glim_amd_cloud*> sources(n);
  std::vector<double> T(12 * n);
  for (std::size_t i = 0; i < n; i++) {
    targets[i] = problems[i].target->handle();
    sources[i] = problems[i].source->handle();
    for (int k = 0; k < 12; k++) T[12 * i + k] = problems[i].T_init.m[k];
  }
  std::vector<glim_amd_align_result> raw(n);
  const glim_amd_lm_params p = params.c();
  const std::uint32_t flags = surface_validation ? GLIM_AMD_FACTOR_SURFACE_VALIDATION : 0u;
  check(glim_amd_vgicp_align_batch(targets.data(), sources.data(), T.data(), flags, (std::int32_t)n, &p, raw.data()), "align_vgicp");
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
    check(glim_amd_expand_compact(raw[i].compact, raw[i].T_target_source, 0, &lin), "align_vgicp");
    for (int k = 0; k < 36; k++) r.information[k] = lin.H_ss[k];
  }
  return out;
}

inline AlignResult align_vgicp(const GaussianVoxelMapGPU& target, const PointCloudGPU& source, const Isometry3d& T_init, const LMParams& params = LMParams(),
                               bool surface_validation = false) {
  return align_vgicp(std::vector<VGICPAlignProblem>{{&target, &source, T_init}}, params, surface_validation)[0];
}

}  // namespace glim_amd
