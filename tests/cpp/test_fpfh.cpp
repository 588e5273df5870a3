// Stands in for viewer/interactive/manual_loop_close_modal.cpp:376-463 (which needs Iridescence): the drop-in gtsam_points::estimate_fpfh and the
// device-side mirror glim_amd::estimate_fpfh / match_fpfh on one cloud, compared with the values the Python test dumped for the same cloud.
//   test_fpfh <cloud.bin>     int32 n, double radius, n x 4 doubles points, n x 4 doubles normals, n x 33 floats expected descriptors,
//                             n int32 expected nearest (the set against itself), n int32 expected reciprocal nearest
// Without an argument: the compile-and-link check only (no device is touched).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <gtsam_points/features/fpfh_estimation.hpp>

struct NoSearch {};

#define REQUIRE(c)                                                  \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAILED %s (%s:%d)\n", #c, __FILE__, __LINE__);   \
      return 1;                                                     \
    }                                                               \
  } while (0)

template <class T>
static bool read_n(std::FILE* f, T* p, std::size_t n) {
  return std::fread(p, sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  static_assert(gtsam_points::FPFH_DIM == 33, "FPFH has 33 bins");
  if (argc < 2) {
    std::printf("test_fpfh OK (no cloud given: nothing run)\n");
    return 0;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f != nullptr);
  std::int32_t n = 0;
  double radius = 0.0;
  REQUIRE(read_n(f, &n, 1) && read_n(f, &radius, 1) && n > 0);
  std::vector<Eigen::Vector4d> points((std::size_t)n), normals((std::size_t)n);
  std::vector<float> expected((std::size_t)n * 33);
  std::vector<std::int32_t> nearest((std::size_t)n), reciprocal((std::size_t)n);
  REQUIRE(read_n(f, points[0].data(), (std::size_t)n * 4) && read_n(f, normals[0].data(), (std::size_t)n * 4));
  REQUIRE(read_n(f, expected.data(), expected.size()) && read_n(f, nearest.data(), nearest.size()) && read_n(f, reciprocal.data(), reciprocal.size()));
  std::fclose(f);

  // the drop-in: same bits as the Python call on the same cloud (the kernels are deterministic), widened to double
  gtsam_points::FPFHEstimationParams params;
  params.search_radius = radius;
  params.num_threads = 4;
  const std::vector<gtsam_points::FPFHSignature> sig = gtsam_points::estimate_fpfh(points.data(), normals.data(), n, NoSearch(), params);
  REQUIRE((int)sig.size() == n);
  for (int i = 0; i < n; i++)
    for (int b = 0; b < 33; b++) REQUIRE(sig[(std::size_t)i].data()[b] == (double)expected[(std::size_t)i * 33 + b]);

  // the mirror: descriptors stay on the device, correspondences come back
  auto cloud = glim_amd::PointCloudGPU::clone(points[0].data(), nullptr, normals[0].data(), n);
  auto fpfh = glim_amd::estimate_fpfh(*cloud, radius);
  REQUIRE((int)fpfh->size() == n);
  const std::vector<float> d = fpfh->download();
  REQUIRE(std::memcmp(d.data(), expected.data(), expected.size() * sizeof(float)) == 0);
  const glim_amd::FPFHCorrespondences fwd = glim_amd::match_fpfh(*fpfh, *fpfh, false);
  const glim_amd::FPFHCorrespondences rec = glim_amd::match_fpfh(*fpfh, *fpfh, true);
  for (int i = 0; i < n; i++) {
    REQUIRE(fwd.nearest[(std::size_t)i] == nearest[(std::size_t)i]);
    REQUIRE(rec.nearest[(std::size_t)i] == reciprocal[(std::size_t)i]);
  }
  bool threw = false;
  try {
    glim_amd::estimate_fpfh(*cloud, 0.0);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  REQUIRE(threw);
  std::printf("test_fpfh OK (%d points, r = %g)\n", n, radius);
  return 0;
}
