// gtsam_points/factors/bundle_adjustment_factor_evm.hpp, MI355X edition: gtsam_points::PlaneEVMFactor and EdgeEVMFactor with the interface the
// plane bundle-adjustment tool uses (bundle_adjustment_modal.cpp:229-245) --
//   factor->add(point, key);  factor->num_points();  factor->error(values);  factor->linearize(values);
// Points are collected on the host.  The device factor (glim_amd::EVMFactorHIP, per-frame moments: one pass over the points) is built at the
// first error() / linearize() and rebuilt after an add(); every evaluation after that costs O(frames^2) and reads no point.
//
// Unlike the registration headers beside this one, the upstream header is NOT pulled in with #include_next: upstream declares PlaneEVMFactor
// and EdgeEVMFactor as plain classes, so the names cannot be taken over by renaming an alias.  This header replaces it.
//
// Two choices rest on recall of gtsam_points, which is not in the reference tree: error() returns the eigenvalue sum unscaled,
// and linearize() returns HessianFactor(keys, G = H, g = -gradient, f = 2 cost), so that 0.5 (f - 2 x^T g + x^T G x) is the second-order
// model of the cost.  H is in general indefinite (the eigenvalue's second derivative is): optimisers damp it.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include <gtsam/linear/HessianFactor.h>
#include <gtsam/nonlinear/NonlinearFactor.h>

#include <glim_amd/plane_ba.hpp>
#include <glim_amd_gtsam.hpp>

namespace gtsam_points {

class BundleAdjustmentFactorBase : public gtsam::NonlinearFactor {
public:
  using shared_ptr = std::shared_ptr<BundleAdjustmentFactorBase>;
  virtual void add(const Eigen::Vector3d& pt, const gtsam::Key& key) = 0;
  virtual int num_points() const = 0;
};

template <int KIND>
class EVMFactorDropIn : public BundleAdjustmentFactorBase {
public:
  EVMFactorDropIn() {}

  // frames are the keys in the order of their first point
  void add(const Eigen::Vector3d& pt, const gtsam::Key& key) override {
    std::int32_t f = 0;
    while (f < (std::int32_t)keys_.size() && keys_[(std::size_t)f] != key) f++;
    if (f == (std::int32_t)keys_.size()) keys_.push_back(key);
    frame_.push_back(f);
    for (int r = 0; r < 3; r++) points_.push_back(pt[r]);
    device_.reset();
  }
  int num_points() const override { return (int)frame_.size(); }
  size_t dim() const override { return 6 * keys_.size(); }

  double error(const gtsam::Values& values) const override { return device().error(poses(values)); }

  std::shared_ptr<gtsam::GaussianFactor> linearize(const gtsam::Values& values) const override {
    const glim_amd::EVMLinearization l = device().linearize(poses(values));
    const int K = (int)keys_.size();
    std::vector<gtsam::Matrix> Gs;  // the upper block triangle, row by row
    std::vector<gtsam::Vector> gs;
    for (int i = 0; i < K; i++) {
      for (int j = i; j < K; j++) {
        gtsam::Matrix G(6, 6);
        for (int r = 0; r < 6; r++)
          for (int c = 0; c < 6; c++) G(r, c) = l.H[(std::size_t)(6 * i + r) * 6 * K + 6 * j + c];
        Gs.push_back(G);
      }
      gtsam::Vector g(6);
      for (int r = 0; r < 6; r++) g(r) = -l.g[(std::size_t)(6 * i + r)];
      gs.push_back(g);
    }
    return std::shared_ptr<gtsam::GaussianFactor>(new gtsam::HessianFactor(keys_, Gs, gs, 2.0 * l.cost));
  }

  gtsam::NonlinearFactor::shared_ptr clone() const override {
    auto c = std::make_shared<EVMFactorDropIn>();
    c->keys_ = keys_;
    c->points_ = points_;
    c->frame_ = frame_;
    return c;
  }

private:
  const glim_amd::EVMFactorHIP<KIND>& device() const {
    if (!device_) device_ = glim_amd::EVMFactorHIP<KIND>::from_points(points_, frame_, (int)keys_.size());
    return *device_;
  }
  std::vector<glim_amd::Isometry3d> poses(const gtsam::Values& values) const {
    std::vector<glim_amd::Isometry3d> T;
    for (const gtsam::Key k : keys_) T.push_back(glim_amd::to_iso(values.at<gtsam::Pose3>(k)));
    return T;
  }
  std::vector<double> points_;        // n x 3, frame-local
  std::vector<std::int32_t> frame_;   // index into keys_
  mutable typename glim_amd::EVMFactorHIP<KIND>::Ptr device_;
};

class PlaneEVMFactor : public EVMFactorDropIn<GLIM_AMD_BA_PLANE> {
public:
  using shared_ptr = std::shared_ptr<PlaneEVMFactor>;
};
class EdgeEVMFactor : public EVMFactorDropIn<GLIM_AMD_BA_EDGE> {
public:
  using shared_ptr = std::shared_ptr<EdgeEVMFactor>;
};

}  // namespace gtsam_points
