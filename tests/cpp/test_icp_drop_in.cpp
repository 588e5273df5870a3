// test_icp_drop_in.cpp -- gtsam_points::IntegratedICPFactor and IntegratedPointToPlaneICPFactor of adapters/gtsam_points_hip driven the way
// GLIM's manual loop closing drives the factor (manual_loop_close_modal.cpp:485-490): a fixed target pose, frames WITHOUT covariances held as
// gtsam_points::PointCloud::ConstPtr, linearize / error / inlier_fraction / set_max_correspondence_distance / set_num_threads / clone.
// Stand-in third-party headers: tests/cpp/glim_standin.  Built by tests/test_icp.py (it compiles and links here, and runs its no-device
// branch), run on the device by tests/test_icp_gpu.py.
#include <cmath>
#include <cstdio>
#include <vector>

#include <gtsam/linear/HessianFactor.h>
#include <gtsam/nonlinear/NonlinearFactorGraph.h>
#include <gtsam_points/factors/integrated_icp_factor.hpp>
#include <gtsam_points/types/point_cloud_cpu.hpp>

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                              \
    }                                                                        \
  } while (0)

// three walls of a room corner shifted by (dx, dy), FP32-representable points; normals of the wall a point lies on when asked for
static gtsam_points::PointCloudCPU::Ptr make_frame(int n, double dx, double dy, bool normals) {
  auto f = std::make_shared<gtsam_points::PointCloudCPU>();
  f->points_storage.resize((size_t)n);
  if (normals) f->normals_storage.resize((size_t)n);
  for (int i = 0; i < n; i++) {
    const double u = (double)((i * 37) % 101) / 101.0, v = (double)((i * 53) % 103) / 103.0;
    double x, y, z, nx = 0, ny = 0, nz = 0;
    if (i % 3 == 0) { x = 8.0 * u; y = 6.0 * v; z = -1.5; nz = 1; }
    else if (i % 3 == 1) { x = 8.0; y = 6.0 * u; z = -1.5 + 3.0 * v; nx = -1; }
    else { x = 8.0 * u; y = 6.0; z = -1.5 + 3.0 * v; ny = -1; }
    f->points_storage[(size_t)i] = Eigen::Vector4d((double)(float)(x + dx), (double)(float)(y + dy), (double)(float)z, 1.0);
    if (normals) f->normals_storage[(size_t)i] = Eigen::Vector4d(nx, ny, nz, 0.0);
  }
  f->num_points = (size_t)n;
  f->points = f->points_storage.data();
  if (normals) f->normals = f->normals_storage.data();
  return f;
}

int main() {
  if (glim_amd_device_count() < 1) {
    std::printf("test_icp_drop_in OK (no device: nothing run)\n");
    return 0;
  }
  const int N = 3000;
  const gtsam_points::PointCloud::ConstPtr target = make_frame(N, 0.0, 0.0, true), source = make_frame(N, 0.03, -0.02, false);
  auto factor = gtsam::make_shared<gtsam_points::IntegratedICPFactor>(gtsam::Pose3(), 0, target, source);   // manual_loop_close_modal.cpp:486
  factor->set_max_correspondence_distance(0.5);
  factor->set_num_threads(4);
  gtsam::NonlinearFactorGraph graph;
  graph.add(factor);
  REQUIRE(dynamic_cast<gtsam_points::IntegratedICPFactor*>(graph[0].get()) != nullptr);
  REQUIRE(factor->dim() == 6 && factor->keys().size() == 1 && factor->clone() != nullptr);
  gtsam::Values values;
  values.insert(0, gtsam::Pose3());
  auto lin = std::dynamic_pointer_cast<gtsam::HessianFactor>(factor->linearize(values));
  REQUIRE(lin != nullptr && lin->keys_.size() == 1);
  const double e = factor->error(values);
  REQUIRE(e > 0.0 && factor->inlier_fraction() > 0.5 && factor->inlier_fraction() <= 1.0);
  // point-to-point: H_vv = sum R^T R = (inliers) I
  REQUIRE(std::fabs(lin->G22_(3, 3) - factor->inlier_fraction() * N) < 1e-3 * N);
  // the binary form and the point-to-plane sibling over the same frames (the target carries normals)
  auto binary = gtsam::make_shared<gtsam_points::IntegratedICPFactor>(0, 1, target, source, std::shared_ptr<const gtsam_points::NearestNeighborSearch>());
  REQUIRE(binary->keys().size() == 2);
  auto plane = gtsam::make_shared<gtsam_points::IntegratedPointToPlaneICPFactor>(gtsam::Pose3(), 0, target, source);
  plane->set_max_correspondence_distance(0.5);
  const double ep = plane->error(values);
  REQUIRE(ep > 0.0 && ep < e && plane->inlier_fraction() == factor->inlier_fraction());  // the in-plane part of every residual is dropped
  REQUIRE(dynamic_cast<gtsam_points::IntegratedICPFactor*>(plane.get()) != nullptr);
  // ... and refused over a target without normals
  bool threw = false;
  try {
    gtsam_points::IntegratedPointToPlaneICPFactor(gtsam::Pose3(), 0, source, source).error(values);
  } catch (const std::exception&) {
    threw = true;
  }
  REQUIRE(threw);
  std::printf("test_icp_drop_in OK (%d points, error %.6g point-to-point, %.6g point-to-plane)\n", N, e, ep);
  return 0;
}
