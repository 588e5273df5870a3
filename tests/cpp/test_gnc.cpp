// Stands in for viewer/interactive/manual_loop_close_modal.cpp:445-458 (which needs Iridescence): the drop-in gtsam_points::estimate_pose_gnc with
// the modal's argument list and the fields it sets, and the mirror glim_amd::estimate_pose_gnc, on a known-answer case the Python test dumped.
//   test_gnc <case.bin>    the layout of registration_case.hpp
// Without an argument: the compile-and-link check only (no device is touched).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include <gtsam_points/features/fpfh_estimation.hpp>
#include <gtsam_points/registration/graduated_non_convexity.hpp>
#include <gtsam_points/registration/ransac.hpp>

#include "registration_case.hpp"

struct NoTree {};

int main(int argc, char** argv) {
  static_assert(sizeof(glim_amd_gnc_params) == 72 && sizeof(glim_amd_gnc_info) == 48, "the layouts glim_amd/_lib.py binds");
  {
    gtsam_points::GNCParams d;
    REQUIRE(d.max_init_samples == 5000 && d.reciprocal_check && !d.tuple_check && d.max_num_tuples == 1000 && d.dof == 6);
  }
  if (argc < 2) {
    std::printf("test_gnc OK (no case given: nothing run)\n");
    return 0;
  }
  Case in;
  REQUIRE(in.load(argv[1]) == 0);
  const std::int32_t nt = in.nt, ns = in.ns, dof = in.dof;
  const std::uint64_t seed_in = in.seed;
  std::vector<Eigen::Vector4d>&tp = in.tp, &sp = in.sp;
  std::vector<gtsam_points::FPFHSignature>&tf = in.tf, &sf = in.sf;
  const double *T = in.T, rate = in.rate;

  auto target = std::make_shared<gtsam_points::PointCloud>(), source = std::make_shared<gtsam_points::PointCloud>();
  target->points = tp.data();
  target->num_points = (std::size_t)nt;
  source->points = sp.data();
  source->num_points = (std::size_t)ns;
  const gtsam_points::FPFHSignature *target_fpfh = tf.data(), *source_fpfh = sf.data();
  auto target_tree = std::make_shared<NoTree>(), target_fpfh_tree = std::make_shared<NoTree>(), source_fpfh_tree = std::make_shared<NoTree>();
  // the fields the modal sets (max_init_samples, reciprocal_check, tuple_check, max_num_tuples, dof, seed, num_threads) and its argument list:
  // two clouds, two descriptor arrays, three trees by reference, the parameters
  gtsam_points::GNCParams params;
  params.max_init_samples = 10000;
  params.reciprocal_check = true;
  params.tuple_check = false;
  params.max_num_tuples = 5000;
  params.dof = dof;
  params.seed = seed_in;
  params.num_threads = 4;
  const std::uint64_t seed = seed_in;
  const gtsam_points::RegistrationResult result =
    gtsam_points::estimate_pose_gnc(*target, *source, target_fpfh, source_fpfh, *target_tree, *target_fpfh_tree, *source_fpfh_tree, params);
  // the same bits as the Python call on the same inputs: the kernels are deterministic
  REQUIRE(result.inlier_rate == rate);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) REQUIRE(result.T_target_source.matrix()(r, c) == T[4 * r + c]);
  REQUIRE(result.T_target_source.matrix()(3, 3) == 1.0 && result.T_target_source.matrix()(3, 0) == 0.0);

  // the mirror with a correspondence list of the caller's: the identity list on (source, source) finds the identity
  auto cloud = glim_amd::PointCloudGPU::clone(sp[0].data(), nullptr, nullptr, ns);
  std::vector<std::int32_t> nearest((std::size_t)ns);
  for (int i = 0; i < ns; i++) nearest[(std::size_t)i] = i;
  glim_amd::GNCParams mp;
  mp.seed = seed;
  glim_amd_gnc_info info;
  const glim_amd::RegistrationResult self = glim_amd::estimate_pose_gnc(*cloud, *cloud, nearest, mp, &info);
  REQUIRE(self.iterations_run == 64 && self.best_iteration == 63 && self.inlier_rate >= 0.9 && info.list_length == info.num_correspondences);
  bool threw = false;
  try {
    mp.dof = 5;
    glim_amd::estimate_pose_gnc(*cloud, *cloud, nearest, mp);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  REQUIRE(threw);
  std::printf("test_gnc OK (%d x %d points, dof %d)\n", (int)nt, (int)ns, (int)dof);
  return 0;
}
