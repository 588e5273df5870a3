// gtsam_points/factors/integrated_icp_factor.hpp, MI355X edition: gtsam_points::IntegratedICPFactor and IntegratedPointToPlaneICPFactor with the
// constructor forms of the drop-in GICP header beside this one --
//   IntegratedICPFactor(target_key, source_key, target_frame, source_frame[, target_tree])
//   IntegratedICPFactor(fixed_target_pose, source_key, target_frame, source_frame[, target_tree])       manual_loop_close_modal.cpp:485-487
// taking the base-class pointers the call sites hold (gtsam_points::PointCloud::ConstPtr).  A frame made by PointCloudGPU::clone is used where it
// lies in HBM, any other frame is uploaded once by the constructor; neither needs covariances (point-to-plane needs the target's normals).
// error / linearize / clone / set_max_correspondence_distance / set_num_threads (a no-op) / inlier_fraction: glim_amd::IntegratedICPFactorHIP, i.e.
// glim_amd_icp_linearize / glim_amd_icp_error on the device.  A target tree passed by the call site is accepted and ignored: the device index is
// built from the target frame, once per factor.
//
// As in the GICP header, the real header stays reachable: upstream defines class TEMPLATES IntegratedICPFactor_<TargetFrame, SourceFrame> and
// IntegratedPointToPlaneICPFactor_<...> with the plain names as aliases; it is pulled in with #include_next under a rename of the two ALIASES only,
// and the plain names are the device classes below.
#pragma once

#define IntegratedICPFactor IntegratedICPFactorUpstreamAlias
#define IntegratedPointToPlaneICPFactor IntegratedPointToPlaneICPFactorUpstreamAlias
#include_next <gtsam_points/factors/integrated_icp_factor.hpp>
#undef IntegratedPointToPlaneICPFactor
#undef IntegratedICPFactor

#include <memory>

#include <gtsam_points/types/point_cloud_gpu.hpp>

#include <glim_amd_gtsam.hpp>

namespace gtsam_points {

class NearestNeighborSearch;  // gtsam_points/ann/nearest_neighbor_search.hpp (CPU); only ever passed through

class IntegratedICPFactor : public glim_amd::IntegratedICPFactorHIP {
public:
  using shared_ptr = std::shared_ptr<IntegratedICPFactor>;

  IntegratedICPFactor(gtsam::Key target_key, gtsam::Key source_key, const PointCloud::ConstPtr& target, const PointCloud::ConstPtr& source,
                      bool use_point_to_plane = false)
  : glim_amd::IntegratedICPFactorHIP(target_key, source_key, device_cloud(target), device_cloud(source), nullptr, use_point_to_plane) {}

  IntegratedICPFactor(gtsam::Key target_key, gtsam::Key source_key, const PointCloud::ConstPtr& target, const PointCloud::ConstPtr& source,
                      const std::shared_ptr<const NearestNeighborSearch>& /*target_tree: the device index replaces it*/, bool use_point_to_plane = false)
  : glim_amd::IntegratedICPFactorHIP(target_key, source_key, device_cloud(target), device_cloud(source), nullptr, use_point_to_plane) {}

  IntegratedICPFactor(const gtsam::Pose3& fixed_target_pose, gtsam::Key source_key, const PointCloud::ConstPtr& target, const PointCloud::ConstPtr& source,
                      bool use_point_to_plane = false)
  : glim_amd::IntegratedICPFactorHIP(fixed_target_pose, source_key, device_cloud(target), device_cloud(source), nullptr, use_point_to_plane) {}

  IntegratedICPFactor(const gtsam::Pose3& fixed_target_pose, gtsam::Key source_key, const PointCloud::ConstPtr& target, const PointCloud::ConstPtr& source,
                      const std::shared_ptr<const NearestNeighborSearch>& /*target_tree*/, bool use_point_to_plane = false)
  : glim_amd::IntegratedICPFactorHIP(fixed_target_pose, source_key, device_cloud(target), device_cloud(source), nullptr, use_point_to_plane) {}
};

class IntegratedPointToPlaneICPFactor : public IntegratedICPFactor {
public:
  using shared_ptr = std::shared_ptr<IntegratedPointToPlaneICPFactor>;

  IntegratedPointToPlaneICPFactor(gtsam::Key target_key, gtsam::Key source_key, const PointCloud::ConstPtr& target, const PointCloud::ConstPtr& source)
  : IntegratedICPFactor(target_key, source_key, target, source, true) {}

  IntegratedPointToPlaneICPFactor(gtsam::Key target_key, gtsam::Key source_key, const PointCloud::ConstPtr& target, const PointCloud::ConstPtr& source,
                                  const std::shared_ptr<const NearestNeighborSearch>& target_tree)
  : IntegratedICPFactor(target_key, source_key, target, source, target_tree, true) {}

  IntegratedPointToPlaneICPFactor(const gtsam::Pose3& fixed_target_pose, gtsam::Key source_key, const PointCloud::ConstPtr& target, const PointCloud::ConstPtr& source)
  : IntegratedICPFactor(fixed_target_pose, source_key, target, source, true) {}

  IntegratedPointToPlaneICPFactor(const gtsam::Pose3& fixed_target_pose, gtsam::Key source_key, const PointCloud::ConstPtr& target, const PointCloud::ConstPtr& source,
                                  const std::shared_ptr<const NearestNeighborSearch>& target_tree)
  : IntegratedICPFactor(fixed_target_pose, source_key, target, source, target_tree, true) {}
};

}  // namespace gtsam_points
