// gtsam_points/registration/graduated_non_convexity.hpp, MI355X edition: the call GLIM's loop-close tool makes, unchanged --
//   result = gtsam_points::estimate_pose_gnc(*target, *source, target_fpfh, source_fpfh, *target_tree, *target_fpfh_tree, *source_fpfh_tree,
//                                            gnc_params);                            viewer/interactive/manual_loop_close_modal.cpp:458
// with GNCParams{max_init_samples, reciprocal_check, tuple_check, max_num_tuples, dof, seed, num_threads}.  The points are uploaded, the
// descriptors narrowed to FP32 and uploaded (glim_amd_fpfh_create), and glim_amd_gnc_align_fpfh matches, selects, solves and scores on the
// device.  The three tree arguments are accepted and ignored (the matcher is a scan, the inlier test an occupancy table), num_threads likewise.
// Semantics: include/glim_amd.h "GNC" (a restatement of Fast Global Registration with counter-based draws).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include <Eigen/Core>
#include <Eigen/Geometry>

#include <glim_amd/gnc.hpp>
#include <gtsam_points/registration/registration_result.hpp>
#include <gtsam_points/types/point_cloud.hpp>

namespace gtsam_points {

struct GNCParams {
  int max_init_samples = 5000;
  bool reciprocal_check = true;
  bool tuple_check = false;
  double tuple_thresh = 0.9;
  int max_num_tuples = 1000;
  double div_factor = 1.4;
  int max_iterations = 64;
  double max_corr_dist = 0.0;
  double inlier_voxel_resolution = 1.0;
  int dof = 6;
  std::uint64_t seed = 5489u;
  int num_threads = 4;  // the device does the work: ignored
};

// Features: a 33-vector of doubles with data() (gtsam_points::FPFHSignature), one per point
template <class Features, class TargetTree, class TargetFeatureTree, class SourceFeatureTree>
RegistrationResult estimate_pose_gnc(const PointCloud& target, const PointCloud& source, const Features* target_features,
                                     const Features* source_features, const TargetTree& /*target_tree*/,
                                     const TargetFeatureTree& /*target_features_tree*/, const SourceFeatureTree& /*source_features_tree*/,
                                     const GNCParams& params = GNCParams()) {
  static_assert(sizeof(Eigen::Vector4d) == 4 * sizeof(double), "Vector4d arrays are n x 4 doubles");
  const auto upload = [](const PointCloud& c, const Features* f, glim_amd::PointCloudGPU::Ptr* cloud, glim_amd::FPFHFeatures::Ptr* fpfh) {
    const std::size_t n = c.size();
    *cloud = glim_amd::PointCloudGPU::clone(n ? c.points[0].data() : nullptr, nullptr, nullptr, (std::int64_t)n);
    std::vector<float> d(n * (std::size_t)glim_amd::FPFH_DIM);
    for (std::size_t i = 0; i < n; i++)
      for (int b = 0; b < glim_amd::FPFH_DIM; b++) d[i * glim_amd::FPFH_DIM + b] = (float)f[i].data()[b];
    *fpfh = glim_amd::upload_fpfh(d.data(), (std::int64_t)n, (*cloud)->context());
  };
  glim_amd::PointCloudGPU::Ptr t, s;
  glim_amd::FPFHFeatures::Ptr tf, sf;
  upload(target, target_features, &t, &tf);
  upload(source, source_features, &s, &sf);
  glim_amd::GNCParams p;
  p.max_init_samples = params.max_init_samples;
  p.reciprocal_check = params.reciprocal_check;
  p.tuple_check = params.tuple_check;
  p.tuple_thresh = params.tuple_thresh;
  p.max_num_tuples = params.max_num_tuples;
  p.div_factor = params.div_factor;
  p.max_iterations = params.max_iterations;
  p.max_corr_dist = params.max_corr_dist;
  p.inlier_voxel_resolution = params.inlier_voxel_resolution;
  p.dof = params.dof;
  p.seed = params.seed;
  const glim_amd::RegistrationResult r = glim_amd::estimate_pose_gnc(*t, *s, *tf, *sf, p);
  RegistrationResult out;
  out.inlier_rate = r.inlier_rate;
  for (int row = 0; row < 3; row++)
    for (int col = 0; col < 4; col++) out.T_target_source.matrix()(row, col) = r.T_target_source.m[(std::size_t)(4 * row + col)];
  return out;
}

}  // namespace gtsam_points
