// test_plane_ba_drop_in.cpp -- gtsam_points::PlaneEVMFactor / EdgeEVMFactor of adapters/gtsam_points_hip driven the way GLIM's plane
// bundle-adjustment tool drives the factor (bundle_adjustment_modal.cpp:229-245): add(point, key) point by point, then error / linearize over
// gtsam::Values.  Stand-in third-party headers: tests/cpp/plane_ba_standin (the N-key HessianFactor) in front of tests/cpp/glim_standin.
// Built by tests/test_plane_ba.py (it compiles and links there, and runs the no-device branch), run on the device by
// tests/test_plane_ba_gpu.py, which compares the blocks written here with glim_amd_ba_factor_linearize byte for byte.
//
//   usage : test_plane_ba_drop_in <in> <out>
//   input : kind K n, n lines "frame x y z", K lines of 12 pose entries (3x4 row-major); frame f is added under key 100 + 7 f
//   output: f, then per key the g block (6), then the upper block triangle row by row (36 each, row-major)
#include <cstdio>
#include <vector>

#include <gtsam_points/factors/bundle_adjustment_factor_evm.hpp>
#include <gtsam_points/factors/bundle_adjustment_factor_lsq.hpp>

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                              \
    }                                                                        \
  } while (0)

template <class Factor>
static int run(int K, long n, const std::vector<int>& frame, const std::vector<double>& pts, const std::vector<double>& poses, const char* out_path) {
  auto factor = std::make_shared<Factor>();
  for (long i = 0; i < n; i++)
    factor->add(Eigen::Vector3d(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]), (gtsam::Key)(100 + 7 * frame[(size_t)i]));
  REQUIRE(factor->num_points() == (int)n && (int)factor->keys().size() == K && factor->dim() == 6 * (size_t)K);
  gtsam::Values values;
  for (int f = 0; f < K; f++) {
    Eigen::Matrix4d M = Eigen::Matrix4d::Identity();
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) M(r, c) = poses[12 * (size_t)f + 4 * r + c];
    values.insert((gtsam::Key)(100 + 7 * f), gtsam::Pose3(M));
  }
  auto lin = std::dynamic_pointer_cast<gtsam::HessianFactor>(factor->linearize(values));
  REQUIRE(lin != nullptr && (int)lin->keys_.size() == K && (int)lin->gs_.size() == K && (int)lin->Gs_.size() == K * (K + 1) / 2);
  REQUIRE(lin->f_ == 2.0 * factor->error(values));
  gtsam::NonlinearFactor::shared_ptr base = factor;  // the type the modal hands to the graph
  REQUIRE(base->clone() != nullptr && base->clone()->dim() == factor->dim());
  FILE* out = std::fopen(out_path, "w");
  REQUIRE(out != nullptr);
  std::fprintf(out, "%.17g\n", lin->f_);
  for (const auto& g : lin->gs_)
    for (int r = 0; r < 6; r++) std::fprintf(out, "%.17g\n", g(r));
  for (const auto& G : lin->Gs_)
    for (int r = 0; r < 6; r++)
      for (int c = 0; c < 6; c++) std::fprintf(out, "%.17g\n", G(r, c));
  std::fclose(out);
  return 0;
}

int main(int argc, char** argv) {
  bool threw = false;
  try {
    gtsam_points::LsqBundleAdjustmentFactor lsq;
  } catch (const std::logic_error&) {
    threw = true;
  }
  REQUIRE(threw);  // declared, not built
  if (glim_amd_device_count() < 1) {
    std::printf("test_plane_ba_drop_in OK (no device: nothing run)\n");
    return 0;
  }
  REQUIRE(argc == 3);
  FILE* in = std::fopen(argv[1], "r");
  REQUIRE(in != nullptr);
  int kind = 0, K = 0;
  long n = 0;
  REQUIRE(std::fscanf(in, "%d %d %ld", &kind, &K, &n) == 3 && K >= 1 && n >= 1);
  std::vector<double> pts(3 * (size_t)n), poses(12 * (size_t)K);
  std::vector<int> frame((size_t)n);
  for (long i = 0; i < n; i++) REQUIRE(std::fscanf(in, "%d %lf %lf %lf", &frame[(size_t)i], &pts[3 * (size_t)i], &pts[3 * (size_t)i + 1], &pts[3 * (size_t)i + 2]) == 4);
  for (size_t i = 0; i < poses.size(); i++) REQUIRE(std::fscanf(in, "%lf", &poses[i]) == 1);
  std::fclose(in);
  const int rc = kind == 0 ? run<gtsam_points::PlaneEVMFactor>(K, n, frame, pts, poses, argv[2]) : run<gtsam_points::EdgeEVMFactor>(K, n, frame, pts, poses, argv[2]);
  if (rc == 0) std::printf("test_plane_ba_drop_in OK (%ld points, %d keys)\n", n, K);
  return rc;
}
