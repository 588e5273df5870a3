// gtsam_points/factors/bundle_adjustment_factor_lsq.hpp, MI355X edition.  GLIM's plane bundle-adjustment tool includes this header
// (bundle_adjustment_modal.cpp) but never constructs the factor; the least-squares bundle-adjustment factor is NOT built here (DESIGN.md 9,
// INTEGRATION.md).  The class is declared so that the include and any mention of the type compile; using it says so.
#pragma once

#include <stdexcept>

#include <gtsam_points/factors/bundle_adjustment_factor_evm.hpp>

namespace gtsam_points {

class LsqBundleAdjustmentFactor : public BundleAdjustmentFactorBase {
public:
  using shared_ptr = std::shared_ptr<LsqBundleAdjustmentFactor>;
  LsqBundleAdjustmentFactor() { not_built(); }
  void add(const Eigen::Vector3d&, const gtsam::Key&) override { not_built(); }
  int num_points() const override { return 0; }
  size_t dim() const override { return 0; }
  double error(const gtsam::Values&) const override { return not_built(), 0.0; }
  std::shared_ptr<gtsam::GaussianFactor> linearize(const gtsam::Values&) const override { return not_built(), nullptr; }
  gtsam::NonlinearFactor::shared_ptr clone() const override { return not_built(), nullptr; }

private:
  [[noreturn]] static void not_built() {
    throw std::logic_error("gtsam_points::LsqBundleAdjustmentFactor is not built in the HIP drop-in: use PlaneEVMFactor / EdgeEVMFactor");
  }
};

}  // namespace gtsam_points
