// Stands in for viewer/interactive/manual_loop_close_modal.cpp:431-443 (which needs Iridescence): the drop-in gtsam_points::estimate_pose_ransac
// with the modal's argument list, and the mirror glim_amd::estimate_pose_ransac, on a known-answer case the Python test dumped.
//   test_ransac <case.bin>    the layout of registration_case.hpp
// Without an argument: the compile-and-link check only (no device is touched).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <gtsam_points/features/fpfh_estimation.hpp>
#include <gtsam_points/registration/ransac.hpp>

#include "registration_case.hpp"

struct NoTree {};

int main(int argc, char** argv) {
  gtsam_points::RANSACParams params;
  static_assert(sizeof(glim_amd_ransac_params) == 48 && sizeof(glim_amd_registration_result) == 120, "the layouts glim_amd/_lib.py binds");
  REQUIRE(params.max_iterations == 5000 && params.early_stop_inlier_rate == 0.9 && params.inlier_voxel_resolution == 1.0);
  if (argc < 2) {
    std::printf("test_ransac OK (no case given: nothing run)\n");
    return 0;
  }
  Case in;
  REQUIRE(in.load(argv[1]) == 0);
  const std::int32_t nt = in.nt, ns = in.ns, dof = in.dof;
  const std::uint64_t seed = in.seed;
  std::vector<Eigen::Vector4d>&tp = in.tp, &sp = in.sp;
  std::vector<gtsam_points::FPFHSignature>&tf = in.tf, &sf = in.sf;
  const double *T = in.T, rate = in.rate;

  gtsam_points::PointCloud target, source;
  target.points = tp.data();
  target.num_points = (std::size_t)nt;
  source.points = sp.data();
  source.num_points = (std::size_t)ns;
  params.dof = dof;
  params.seed = seed;
  params.num_threads = 4;
  const gtsam_points::RegistrationResult result = gtsam_points::estimate_pose_ransac(target, source, tf.data(), sf.data(), NoTree(), NoTree(), params);
  // the same bits as the Python call on the same inputs: the kernels are deterministic
  REQUIRE(result.inlier_rate == rate);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) REQUIRE(result.T_target_source.matrix()(r, c) == T[4 * r + c]);
  REQUIRE(result.T_target_source.matrix()(3, 3) == 1.0 && result.T_target_source.matrix()(3, 0) == 0.0);

  // the mirror with a correspondence list of the caller's: the identity list on (source, source) finds the identity
  auto cloud = glim_amd::PointCloudGPU::clone(sp[0].data(), nullptr, nullptr, ns);
  std::vector<std::int32_t> nearest((std::size_t)ns);
  for (int i = 0; i < ns; i++) nearest[(std::size_t)i] = i;
  glim_amd::RANSACParams mp;
  mp.seed = seed;
  const glim_amd::RegistrationResult self = glim_amd::estimate_pose_ransac(*cloud, *cloud, nearest, mp);
  REQUIRE(self.best_iteration >= 0 && self.iterations_run == self.best_iteration + 1 && self.inlier_rate >= 0.9);
  bool threw = false;
  try {
    mp.dof = 5;
    glim_amd::estimate_pose_ransac(*cloud, *cloud, nearest, mp);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  REQUIRE(threw);
  std::printf("test_ransac OK (%d x %d points, dof %d)\n", (int)nt, (int)ns, (int)dof);
  return 0;
}
