// gtsam_points/features/fpfh_estimation.hpp, MI355X edition: the call GLIM's global registration makes, unchanged --
//   auto fpfh = gtsam_points::estimate_fpfh(points, normals, num_points, *tree, params);      viewer/interactive/manual_loop_close_modal.cpp:396
// with FPFHEstimationParams{search_radius, num_threads}.  The points and normals are uploaded, glim_amd_fpfh_estimate runs on the device (its
// own cell grid finds the neighbours: the search object is accepted and ignored, num_threads likewise) and the FP32 descriptors are widened
// into the FPFHSignature vectors the caller's KdTreeX<FPFH_DIM> / RANSAC / GNC consume.  A caller that stays on the device uses
// glim_amd::estimate_fpfh / glim_amd::match_fpfh (include/glim_amd/fpfh.hpp) and never downloads the descriptors.
// Semantics: include/glim_amd.h "FPFH" (PCL's FPFHEstimation; no PFH, no 4-DoF variant).
#pragma once

#include <cstddef>
#include <vector>

#include <Eigen/Core>

#include <glim_amd/fpfh.hpp>

namespace gtsam_points {

constexpr int FPFH_DIM = glim_amd::FPFH_DIM;
using FPFHSignature = Eigen::Matrix<double, FPFH_DIM, 1>;

struct FPFHEstimationParams {
  double search_radius = 5.0;
  int num_threads = 1;  // the device does the work: ignored
};

template <class Search>
std::vector<FPFHSignature> estimate_fpfh(const Eigen::Vector4d* points, const Eigen::Vector4d* normals, int num_points, const Search& /*search*/,
                                         const FPFHEstimationParams& params = FPFHEstimationParams()) {
  std::vector<FPFHSignature> out((std::size_t)(num_points > 0 ? num_points : 0));
  if (out.empty()) return out;
  static_assert(sizeof(Eigen::Vector4d) == 4 * sizeof(double), "Vector4d arrays are n x 4 doubles");
  auto cloud = glim_amd::PointCloudGPU::clone(points[0].data(), nullptr, normals[0].data(), num_points);
  const std::vector<float> d = glim_amd::estimate_fpfh(*cloud, params.search_radius)->download();
  for (std::size_t i = 0; i < out.size(); i++) {
    double* o = out[i].data();
    for (int b = 0; b < FPFH_DIM; b++) o[b] = (double)d[i * FPFH_DIM + b];
  }
  return out;
}

}  // namespace gtsam_points
