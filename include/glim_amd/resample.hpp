// resample.hpp -- header-only C++17 mirror, over the C ABI (glim_amd.h "Resampling a resident cloud"), of the gtsam_points functions that
// derive a cloud from another one, for clouds that are already on the device:
//
//   auto sub = glim_amd::random_sampling(cloud, 0.1, mt);      // gtsam_points::random_sampling(frame, rate, mt): sub_mapping.cpp:385
//   auto sel = glim_amd::sample(cloud, indices);               // gtsam_points::sample(frame, indices): points_selector.cpp:561
//   auto moved = glim_amd::transform(cloud, T_world_lidar);    // gtsam_points::transform(frame, T): sub_mapping_passthrough.cpp:75
//
// Each call returns a new cloud; the input is untouched.  There is no drop-in redirection: at GLIM's call sites the argument's static type is
// gtsam_points::PointCloud::Ptr, so an overload on the device type would never be chosen.  INTEGRATION.md shows the two-line edit instead
// (clone once, then sample the clone).
#pragma once

#include <cstdint>
#include <random>
#include <vector>

#include "gtsam_points_compat.hpp"

namespace glim_amd {

// int(size * rate) points in their original order; rate >= 0.99 copies the whole cloud.  The draw is a function of (seed, size).
inline PointCloudGPU::Ptr random_sampling(const PointCloudGPU::ConstPtr& cloud, double rate, std::uint64_t seed) {
  if (!cloud) throw std::invalid_argument("null cloud");
  glim_amd_cloud* h = nullptr;
  check(glim_amd_cloud_random_sample(cloud->handle(), rate, seed, &h), "random_sampling");
  return PointCloudGPU::adopt(h, cloud->context());
}

// the signature of the call sites, which hand their generator over: one 64-bit seed is drawn from it as two calls of mt(), the first one
// the upper half, so that a call site keeps its generator and its runs stay reproducible
inline std::uint64_t draw_seed(std::mt19937& mt) {
  const std::uint64_t hi = (std::uint64_t)(std::uint32_t)mt();
  const std::uint64_t lo = (std::uint64_t)(std::uint32_t)mt();
  return (hi << 32) | lo;
}
inline PointCloudGPU::Ptr random_sampling(const PointCloudGPU::ConstPtr& cloud, double rate, std::mt19937& mt) {
  if (!cloud) throw std::invalid_argument("null cloud");
  return random_sampling(cloud, rate, draw_seed(mt));
}

// point j of the result = point indices[j] of the cloud: any order, duplicates allowed
inline PointCloudGPU::Ptr sample(const PointCloudGPU::ConstPtr& cloud, const std::vector<std::int32_t>& indices) {
  if (!cloud) throw std::invalid_argument("null cloud");
  glim_amd_cloud* h = nullptr;
  check(glim_amd_cloud_sample(cloud->handle(), (std::int64_t)indices.size(), indices.empty() ? nullptr : indices.data(), &h), "sample");
  return PointCloudGPU::adopt(h, cloud->context());
}

// points, covariances and normals moved by T
inline PointCloudGPU::Ptr transform(const PointCloudGPU::ConstPtr& cloud, const Isometry3d& T) {
  if (!cloud) throw std::invalid_argument("null cloud");
  glim_amd_cloud* h = nullptr;
  check(glim_amd_cloud_transform(cloud->handle(), T.m.data(), &h), "transform");
  return PointCloudGPU::adopt(h, cloud->context());
}

}  // namespace glim_amd
