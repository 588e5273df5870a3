// fpfh.hpp -- header-only C++17 mirror, over the C ABI (glim_amd.h "FPFH"), of the two data-parallel stages of GLIM's global registration
// (viewer/interactive/manual_loop_close_modal.cpp:376-463): FPFH descriptors of a device cloud and nearest-descriptor correspondences.
//
//   auto frame = glim_amd::PointCloudGPU::clone(points4, nullptr, normals4, n);
//   auto fpfh  = glim_amd::estimate_fpfh(*frame, 5.0);                         // gtsam_points::estimate_fpfh, :396
//   auto corr  = glim_amd::match_fpfh(*target_fpfh, *source_fpfh, true);       // the KdTreeX<FPFH_DIM> queries, reciprocal_check = true
//
// RANSAC / GNC consume corr.nearest; they stay on the host side of the caller.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "gtsam_points_compat.hpp"

namespace glim_amd {

constexpr int FPFH_DIM = 33;

// n x 33 FP32 descriptors on the device; owns the handle, keeps the cloud's context alive
class FPFHFeatures {
public:
  using Ptr = std::shared_ptr<FPFHFeatures>;
  using ConstPtr = std::shared_ptr<const FPFHFeatures>;
  FPFHFeatures(glim_amd_fpfh* h, Context ctx) : ctx_(std::move(ctx)), h_(h) {}
  ~FPFHFeatures() { glim_amd_fpfh_destroy(h_); }
  FPFHFeatures(const FPFHFeatures&) = delete;
  FPFHFeatures& operator=(const FPFHFeatures&) = delete;
  std::size_t size() const {
    std::int64_t n = 0;
    glim_amd_fpfh_size(h_, &n);
    return (std::size_t)n;
  }
  // n x 33, row i = point i of the cloud
  std::vector<float> download() const {
    std::vector<float> out(size() * (std::size_t)FPFH_DIM);
    if (!out.empty()) check(glim_amd_fpfh_download(h_, out.data()), "FPFHFeatures::download");
    return out;
  }
  glim_amd_fpfh* handle() const { return h_; }

private:
  Context ctx_;
  glim_amd_fpfh* h_ = nullptr;
};

// the cloud needs normals (clone with normals, or estimate_covariances)
inline FPFHFeatures::Ptr estimate_fpfh(const PointCloudGPU& cloud, double search_radius) {
  glim_amd_fpfh* h = nullptr;
  check(glim_amd_fpfh_estimate(cloud.handle(), search_radius, &h), "estimate_fpfh");
  return std::make_shared<FPFHFeatures>(h, cloud.context());
}

struct FPFHCorrespondences {
  std::vector<std::int32_t> nearest;  // per source descriptor: target index, or -1 (empty target / failed reciprocal check)
  std::vector<float> sqdist;          // squared L2 distance to the nearest target descriptor
};

inline FPFHCorrespondences match_fpfh(const FPFHFeatures& target, const FPFHFeatures& source, bool reciprocal_check = false) {
  FPFHCorrespondences c;
  c.nearest.assign(source.size(), -1);
  c.sqdist.assign(source.size(), 0.0f);
  check(glim_amd_fpfh_match(target.handle(), source.handle(), reciprocal_check ? GLIM_AMD_FPFH_RECIPROCAL : 0u, c.nearest.data(), c.sqdist.data()),
        "match_fpfh");
  return c;
}

}  // namespace glim_amd
