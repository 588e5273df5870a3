// gtsam_points/registration/registration_result.hpp, MI355X edition: what the global registrations return (manual_loop_close_modal.cpp:429,
// :462-465 reads T_target_source and inlier_rate).
#pragma once

#include <Eigen/Core>
#include <Eigen/Geometry>

namespace gtsam_points {

struct RegistrationResult {
  double inlier_rate = 0.0;
  Eigen::Isometry3d T_target_source = Eigen::Isometry3d::Identity();
};

}  // namespace gtsam_points
