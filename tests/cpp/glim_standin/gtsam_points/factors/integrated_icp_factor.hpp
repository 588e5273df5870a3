#pragma once
// upstream's shape (from recall): class templates over the target / source frame types + the aliases call sites name
#include <gtsam_points/factors/integrated_matching_cost_factor.hpp>
namespace gtsam_points {
class NearestNeighborSearch;
template <typename TargetFrame = PointCloud, typename SourceFrame = PointCloud>
class IntegratedICPFactor_ : public IntegratedMatchingCostFactor {
public:
  IntegratedICPFactor_(gtsam::Key, gtsam::Key, const std::shared_ptr<const TargetFrame>&, const std::shared_ptr<const SourceFrame>&,
                       const std::shared_ptr<const NearestNeighborSearch>&, bool use_point_to_plane = false);
  IntegratedICPFactor_(gtsam::Key, gtsam::Key, const std::shared_ptr<const TargetFrame>&, const std::shared_ptr<const SourceFrame>&,
                       bool use_point_to_plane = false);
  IntegratedICPFactor_(const gtsam::Pose3&, gtsam::Key, const std::shared_ptr<const TargetFrame>&, const std::shared_ptr<const SourceFrame>&,
                       const std::shared_ptr<const NearestNeighborSearch>&, bool use_point_to_plane = false);
  IntegratedICPFactor_(const gtsam::Pose3&, gtsam::Key, const std::shared_ptr<const TargetFrame>&, const std::shared_ptr<const SourceFrame>&,
                       bool use_point_to_plane = false);
  void set_max_correspondence_distance(double);
};
template <typename TargetFrame = PointCloud, typename SourceFrame = PointCloud>
class IntegratedPointToPlaneICPFactor_ : public IntegratedICPFactor_<TargetFrame, SourceFrame> {};
using IntegratedICPFactor = IntegratedICPFactor_<>;
using IntegratedPointToPlaneICPFactor = IntegratedPointToPlaneICPFactor_<>;
}  // namespace gtsam_points
