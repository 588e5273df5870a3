// gnc.hpp -- header-only C++17 mirror, over the C ABI (glim_amd.h "GNC"), of the GNC global registration of GLIM's loop-close tool
// (viewer/interactive/manual_loop_close_modal.cpp:445-458): two device clouds in, T_target_source out.
//
//   auto target_fpfh = glim_amd::estimate_fpfh(*target, 5.0), source_fpfh = glim_amd::estimate_fpfh(*source, 5.0);
//   glim_amd::GNCParams params;                                                          // reciprocal_check = true, as the modal sets it
//   auto result = glim_amd::estimate_pose_gnc(*target, *source, *target_fpfh, *source_fpfh, params);   // matching on the device
//   auto result2 = glim_amd::estimate_pose_gnc(*target, *source, nearest, params);                     // or a correspondence list of the caller's
#pragma once

#include <cstdint>
#include <vector>

#include "ransac.hpp"

namespace glim_amd {

struct GNCParams {
  int max_init_samples = 5000;
  bool reciprocal_check = true;  // the *_fpfh form: keep a correspondence only when it is mutual (GLIM_AMD_FPFH_RECIPROCAL)
  bool tuple_check = false;
  double tuple_thresh = 0.9;
  int max_num_tuples = 1000;
  double div_factor = 1.4;
  int max_iterations = 64;
  double max_corr_dist = 0.0;  // <= 0: 0.025 of the larger bounding-box diagonal
  double inlier_voxel_resolution = 1.0;
  int dof = 6;  // 4: rotation about z + translation
  std::uint64_t seed = 0;
  glim_amd_gnc_params c() const {
    glim_amd_gnc_params p;
    p.max_init_samples = max_init_samples;
    p.tuple_check = tuple_check ? 1 : 0;
    p.tuple_thresh = tuple_thresh;
    p.max_num_tuples = max_num_tuples;
    p.div_factor = div_factor;
    p.max_iterations = max_iterations;
    p.max_corr_dist = max_corr_dist;
    p.inlier_voxel_resolution = inlier_voxel_resolution;
    p.dof = dof;
    p.seed = seed;
    return p;
  }
};

// nearest: one entry per source point, the matched target point or -1 (match_fpfh's `nearest`); info may be null
inline RegistrationResult estimate_pose_gnc(const PointCloudGPU& target, const PointCloudGPU& source, const std::vector<std::int32_t>& nearest,
                                            const GNCParams& params = GNCParams(), glim_amd_gnc_info* info = nullptr) {
  if (nearest.size() != source.size()) throw std::runtime_error("estimate_pose_gnc: nearest must hold one entry per source point");
  const glim_amd_gnc_params p = params.c();
  glim_amd_registration_result r;
  check(glim_amd_gnc_align(target.handle(), source.handle(), nearest.data(), &p, &r, info), "estimate_pose_gnc");
  return from_c(r);
}

// the correspondences are found on the device and never visit the host
inline RegistrationResult estimate_pose_gnc(const PointCloudGPU& target, const PointCloudGPU& source, const FPFHFeatures& target_features,
                                            const FPFHFeatures& source_features, const GNCParams& params = GNCParams(),
                                            glim_amd_gnc_info* info = nullptr) {
  const glim_amd_gnc_params p = params.c();
  glim_amd_registration_result r;
  check(glim_amd_gnc_align_fpfh(target.handle(), source.handle(), target_features.handle(), source_features.handle(),
                                params.reciprocal_check ? GLIM_AMD_FPFH_RECIPROCAL : 0u, &p, &r, info),
        "estimate_pose_gnc");
  return from_c(r);
}

}  // namespace glim_amd
