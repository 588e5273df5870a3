// ransac.hpp -- header-only C++17 mirror, over the C ABI (glim_amd.h "RANSAC"), of the RANSAC global registration of GLIM's loop-close tool
// (viewer/interactive/manual_loop_close_modal.cpp:431-443): two device clouds in, T_target_source out.
//
//   auto target_fpfh = glim_amd::estimate_fpfh(*target, 5.0), source_fpfh = glim_amd::estimate_fpfh(*source, 5.0);
//   glim_amd::RANSACParams params;                                                       // the modal's defaults
//   auto result = glim_amd::estimate_pose_ransac(*target, *source, *target_fpfh, *source_fpfh, params);   // matching on the device
//   auto result2 = glim_amd::estimate_pose_ransac(*target, *source, nearest, params);                     // or a correspondence list of the caller's
#pragma once

#include <cstdint>
#include <vector>

#include "fpfh.hpp"

namespace glim_amd {

struct RANSACParams {
  int max_iterations = 5000;
  double early_stop_inlier_rate = 0.9;
  double poly_error_thresh = 0.5;
  double inlier_voxel_resolution = 1.0;
  int dof = 6;  // 4: rotation about z + translation
  std::uint64_t seed = 0;
  bool reciprocal_check = false;  // the *_fpfh form: keep a correspondence only when it is mutual (GLIM_AMD_FPFH_RECIPROCAL)
  glim_amd_ransac_params c() const {
    glim_amd_ransac_params p;
    p.max_iterations = max_iterations;
    p.early_stop_inlier_rate = early_stop_inlier_rate;
    p.poly_error_thresh = poly_error_thresh;
    p.inlier_voxel_resolution = inlier_voxel_resolution;
    p.dof = dof;
    p.seed = seed;
    return p;
  }
};

struct RegistrationResult {
  Isometry3d T_target_source;
  double inlier_rate = 0.0;
  std::int64_t num_inliers = 0;
  int best_iteration = -1;  // -1: no hypothesis passed the checks (T_target_source is the identity)
  int iterations_run = 0;
};

inline RegistrationResult from_c(const glim_amd_registration_result& r) {
  RegistrationResult out;
  for (int i = 0; i < 12; i++) out.T_target_source.m[(std::size_t)i] = r.T_target_source[i];
  out.inlier_rate = r.inlier_rate;
  out.num_inliers = r.num_inliers;
  out.best_iteration = r.best_iteration;
  out.iterations_run = r.iterations_run;
  return out;
}

// nearest: one entry per source point, the matched target point or -1 (match_fpfh's `nearest`)
inline RegistrationResult estimate_pose_ransac(const PointCloudGPU& target, const PointCloudGPU& source, const std::vector<std::int32_t>& nearest,
                                               const RANSACParams& params = RANSACParams()) {
  if (nearest.size() != source.size()) throw std::runtime_error("estimate_pose_ransac: nearest must hold one entry per source point");
  const glim_amd_ransac_params p = params.c();
  glim_amd_registration_result r;
  check(glim_amd_ransac_align(target.handle(), source.handle(), nearest.data(), &p, &r), "estimate_pose_ransac");
  return from_c(r);
}

// the correspondences are found on the device and never visit the host
inline RegistrationResult estimate_pose_ransac(const PointCloudGPU& target, const PointCloudGPU& source, const FPFHFeatures& target_features,
                                               const FPFHFeatures& source_features, const RANSACParams& params = RANSACParams()) {
  const glim_amd_ransac_params p = params.c();
  glim_amd_registration_result r;
  check(glim_amd_ransac_align_fpfh(target.handle(), source.handle(), target_features.handle(), source_features.handle(),
                                   params.reciprocal_check ? GLIM_AMD_FPFH_RECIPROCAL : 0u, &p, &r),
        "estimate_pose_ransac");
  return from_c(r);
}

// descriptors that are already on the host (n x 33 floats) as a device object
inline FPFHFeatures::Ptr upload_fpfh(const float* descriptors33, std::int64_t n, Context ctx) {
  glim_amd_fpfh* h = nullptr;
  check(glim_amd_fpfh_create(ctx->context(), n, descriptors33, &h), "upload_fpfh");
  return std::make_shared<FPFHFeatures>(h, std::move(ctx));
}

}  // namespace glim_amd
