// plane_ba.hpp -- header-only C++17 mirror, over the C ABI (glim_amd.h "Plane / edge bundle-adjustment factors and ball selection"), of the
// data-parallel steps of GLIM's plane bundle-adjustment tool (viewer/interactive/bundle_adjustment_modal.cpp) and of the factor it builds.
//
//   auto pairs  = glim_amd::extract_ball(submaps, poses, center, radius);               // extract_points, :143-161
//   auto lambda = glim_amd::ball_eigenvalues(submaps, poses, center, radius);           // calc_eigenvalues, :163-184
//   double r    = glim_amd::auto_radius(submaps, poses, center, radius).radius;         // auto_radius, :186-227
//   auto factor = glim_amd::PlaneEVMFactorHIP::from_ball(submaps, poses, center, r);    // create_factor, :229-245
//   auto lin    = factor->linearize(frame_poses);                                       // cost, g (6 K), H (6 K x 6 K): plain arrays
//
// The gtsam-typed drop-in is adapters/gtsam_points_hip/gtsam_points/factors/bundle_adjustment_factor_evm.hpp.
#pragma once

#include <array>
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

#include "gtsam_points_compat.hpp"

namespace glim_amd {

namespace ba_detail {
struct BallArgs {
  std::vector<const glim_amd_cloud*> handles;
  std::vector<double> T12;
};
inline BallArgs ball_args(const std::vector<PointCloudGPU::ConstPtr>& submaps, const std::vector<Isometry3d>& poses) {
  if (submaps.size() != poses.size()) throw std::invalid_argument("one pose per sub-map");
  BallArgs a;
  for (std::size_t s = 0; s < submaps.size(); s++) {
    a.handles.push_back(submaps[s]->handle());
    a.T12.insert(a.T12.end(), poses[s].m.begin(), poses[s].m.end());
  }
  return a;
}
}  // namespace ba_detail

// (sub-map index, point index) of every point within `radius` of `center`, in the reference's loop order
inline std::vector<std::pair<int, int>> extract_ball(const std::vector<PointCloudGPU::ConstPtr>& submaps, const std::vector<Isometry3d>& poses,
                                                     const std::array<double, 3>& center, double radius) {
  const auto a = ba_detail::ball_args(submaps, poses);
  std::int64_t count = 0;
  check(glim_amd_ba_ball_select(a.handles.data(), (std::int32_t)a.handles.size(), a.T12.data(), center.data(), radius, 0, nullptr, &count), "extract_ball");
  std::vector<std::int32_t> flat(2 * (std::size_t)count + 2);
  check(glim_amd_ba_ball_select(a.handles.data(), (std::int32_t)a.handles.size(), a.T12.data(), center.data(), radius, count, flat.data(), &count), "extract_ball");
  std::vector<std::pair<int, int>> out((std::size_t)count);
  for (std::size_t i = 0; i < out.size(); i++) out[i] = {flat[2 * i], flat[2 * i + 1]};
  return out;
}

inline glim_amd_ba_stats ball_statistics(const std::vector<PointCloudGPU::ConstPtr>& submaps, const std::vector<Isometry3d>& poses,
                                         const std::array<double, 3>& center, double radius) {
  const auto a = ba_detail::ball_args(submaps, poses);
  glim_amd_ba_stats st;
  check(glim_amd_ba_ball_stats(a.handles.data(), (std::int32_t)a.handles.size(), a.T12.data(), center.data(), radius, &st), "ball_statistics");
  return st;
}

// the three eigenvalues of the ball's covariance, ascending
inline std::array<double, 3> ball_eigenvalues(const std::vector<PointCloudGPU::ConstPtr>& submaps, const std::vector<Isometry3d>& poses,
                                              const std::array<double, 3>& center, double radius) {
  const glim_amd_ba_stats st = ball_statistics(submaps, poses, center, radius);
  return {st.eigenvalues[0], st.eigenvalues[1], st.eigenvalues[2]};
}

inline glim_amd_ba_radius_result auto_radius(const std::vector<PointCloudGPU::ConstPtr>& submaps, const std::vector<Isometry3d>& poses,
                                             const std::array<double, 3>& center, double radius, const glim_amd_ba_params* params = nullptr) {
  const auto a = ba_detail::ball_args(submaps, poses);
  glim_amd_ba_radius_result out;
  check(glim_amd_ba_auto_radius(a.handles.data(), (std::int32_t)a.handles.size(), a.T12.data(), center.data(), radius, params, &out), "auto_radius");
  return out;
}

struct EVMLinearization {
  double cost = 0.0;
  std::uint32_t status = 0;  // GLIM_AMD_BA_DEGENERATE or 0
  std::vector<double> g;     // 6 K, [rotation, translation] per frame
  std::vector<double> H;     // 6 K x 6 K row-major
};

// gtsam_points::PlaneEVMFactor (KIND = GLIM_AMD_BA_PLANE) / EdgeEVMFactor (GLIM_AMD_BA_EDGE) over per-frame moments on the device
template <int KIND>
class EVMFactorHIP {
public:
  using Ptr = std::shared_ptr<EVMFactorHIP>;
  EVMFactorHIP(glim_amd_ba_factor* h, Context ctx) : ctx_(std::move(ctx)), h_(h) {
    check(glim_amd_ba_factor_info(h_, &K_, &N_, nullptr, nullptr, nullptr), "EVMFactorHIP");
  }
  ~EVMFactorHIP() { glim_amd_ba_factor_destroy(h_); }
  EVMFactorHIP(const EVMFactorHIP&) = delete;
  EVMFactorHIP& operator=(const EVMFactorHIP&) = delete;

  static Ptr from_ball(const std::vector<PointCloudGPU::ConstPtr>& submaps, const std::vector<Isometry3d>& poses, const std::array<double, 3>& center,
                       double radius) {
    const auto a = ba_detail::ball_args(submaps, poses);
    glim_amd_ba_factor* h = nullptr;
    check(glim_amd_ba_factor_create_from_ball(a.handles.data(), (std::int32_t)a.handles.size(), a.T12.data(), center.data(), radius, KIND, &h),
          "EVMFactorHIP::from_ball");
    return std::make_shared<EVMFactorHIP>(h, submaps.front()->context());
  }
  // points3: n x 3 frame-local; frame_index: n entries in [0, num_frames)
  static Ptr from_points(const std::vector<double>& points3, const std::vector<std::int32_t>& frame_index, int num_frames, Context ctx = nullptr) {
    if (!ctx) ctx = StreamTempBufferRoundRobin::default_instance();
    if (points3.size() != 3 * frame_index.size()) throw std::invalid_argument("one frame index per point");
    glim_amd_ba_factor* h = nullptr;
    check(glim_amd_ba_factor_create(ctx->context(), KIND, (std::int64_t)frame_index.size(), points3.data(), frame_index.data(), num_frames, &h),
          "EVMFactorHIP::from_points");
    return std::make_shared<EVMFactorHIP>(h, ctx);
  }

  int num_frames() const { return K_; }
  std::int64_t num_points() const { return N_; }
  // the frame (or sub-map) indices that hold a point, ascending: pose k of error() / linearize() belongs to frames()[k]
  std::vector<std::int32_t> frames() const {
    std::vector<std::int32_t> kept((std::size_t)K_);
    check(glim_amd_ba_factor_info(h_, nullptr, nullptr, nullptr, kept.data(), nullptr), "EVMFactorHIP::frames");
    return kept;
  }
  std::vector<double> moments() const {
    std::vector<double> m((std::size_t)K_ * GLIM_AMD_BA_MOMENT_DOUBLES);
    check(glim_amd_ba_factor_info(h_, nullptr, nullptr, nullptr, nullptr, m.data()), "EVMFactorHIP::moments");
    return m;
  }
  double error(const std::vector<Isometry3d>& poses, std::uint32_t* status = nullptr) const {
    const std::vector<double> T = flat(poses);
    double cost = 0.0;
    check(glim_amd_ba_factor_error(h_, T.data(), &cost, status), "EVMFactorHIP::error");
    return cost;
  }
  EVMLinearization linearize(const std::vector<Isometry3d>& poses) const {
    const std::vector<double> T = flat(poses);
    EVMLinearization l;
    l.g.assign(6 * (std::size_t)K_, 0.0);
    l.H.assign(36 * (std::size_t)K_ * K_, 0.0);
    check(glim_amd_ba_factor_linearize(h_, T.data(), &l.cost, l.g.data(), l.H.data(), &l.status), "EVMFactorHIP::linearize");
    return l;
  }
  glim_amd_ba_factor* handle() const { return h_; }

private:
  std::vector<double> flat(const std::vector<Isometry3d>& poses) const {
    if ((int)poses.size() != K_) throw std::invalid_argument("one pose per kept frame");
    std::vector<double> T;
    for (const auto& p : poses) T.insert(T.end(), p.m.begin(), p.m.end());
    return T;
  }
  Context ctx_;
  glim_amd_ba_factor* h_ = nullptr;
  std::int32_t K_ = 0;
  std::int64_t N_ = 0;
};
using PlaneEVMFactorHIP = EVMFactorHIP<GLIM_AMD_BA_PLANE>;
using EdgeEVMFactorHIP = EVMFactorHIP<GLIM_AMD_BA_EDGE>;

}  // namespace glim_amd
