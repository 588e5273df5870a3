// The C++ mirror of the ICP factors and the ICP fine registration (include/glim_amd/icp_align.hpp): it compiles and links on its own, its
// parameters are the library's, and -- where a device is visible -- the factor and the loop run on a small synthetic pair without covariances:
// the batch form and the single form return the same bytes, the loop's record is the factor's at the estimate.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <glim_amd/icp_align.hpp>

#define REQUIRE(c)                                                \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s (%s:%d)\n", #c, __FILE__, __LINE__); \
      return 1;                                                   \
    }                                                             \
  } while (0)

// three walls of a room corner, n x Vector4d, FP32-representable; shifted by (dx, dy)
static std::vector<double> corner(int n, double dx, double dy) {
  std::vector<double> p((std::size_t)n * 4);
  for (int i = 0; i < n; i++) {
    const double u = (double)((i * 37) % 101) / 101.0, v = (double)((i * 53) % 103) / 103.0;
    double x, y, z;
    if (i % 3 == 0) { x = 8.0 * u; y = 6.0 * v; z = -1.5; }
    else if (i % 3 == 1) { x = 8.0; y = 6.0 * u; z = -1.5 + 3.0 * v; }
    else { x = 8.0 * u; y = 6.0; z = -1.5 + 3.0 * v; }
    p[4 * (std::size_t)i + 0] = (double)(float)(x + dx);
    p[4 * (std::size_t)i + 1] = (double)(float)(y + dy);
    p[4 * (std::size_t)i + 2] = (double)(float)z;
    p[4 * (std::size_t)i + 3] = 1.0;
  }
  return p;
}

int main() {
  {
    glim_amd_lm_params d;
    REQUIRE(glim_amd_icp_align_default_params(&d) == GLIM_AMD_OK);
    const glim_amd_lm_params m = glim_amd::ICPParams().c();
    REQUIRE(std::memcmp(&d, &m, sizeof(d)) == 0 && d.max_iterations == 200);
    REQUIRE(glim_amd_icp_align_default_params(nullptr) == GLIM_AMD_ERR_INVALID);
    REQUIRE(glim_amd_icp_align_batch(nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr) == GLIM_AMD_OK);
    REQUIRE(glim_amd_icp_align_batch(nullptr, nullptr, nullptr, nullptr, GLIM_AMD_FACTOR_BINARY, 0, nullptr, nullptr) == GLIM_AMD_ERR_INVALID);
  }
  if (glim_amd_device_count() <= 0) {
    std::printf("test_icp_align OK (no device: nothing run)\n");
    return 0;
  }
  const int n = 3000;
  const std::vector<double> tp = corner(n, 0.0, 0.0), sp = corner(n, 0.03, -0.02);
  auto target = glim_amd::PointCloudGPU::clone(tp.data(), nullptr, nullptr, n);
  auto source = glim_amd::PointCloudGPU::clone(sp.data(), nullptr, nullptr, n);
  auto tree = std::make_shared<glim_amd::NearestNeighborSearchGPU>(target, 0.5);
  glim_amd::Isometry3d I;
  glim_amd::IntegratedICPFactor f(I, 1, target, source, tree);
  f.set_max_correspondence_distance(0.5);
  glim_amd::Values values;
  values[1] = I;
  const glim_amd::LinearizedSystem6 L = f.linearize(values);
  REQUIRE(L.num_inliers > n / 2 && L.error > 0.0 && f.inlier_fraction() > 0.5);
  REQUIRE(std::fabs(f.error(values) - L.error) <= 1e-12 * L.error);
  // point-to-plane over a target without normals: a state error, surfaced as an exception
  bool threw = false;
  try {
    glim_amd::IntegratedICPFactor(I, 1, target, source, tree, true).linearize(values);
  } catch (const std::exception&) {
    threw = true;
  }
  REQUIRE(threw);
  glim_amd::ICPParams prm;
  prm.max_iterations = 5;
  const auto batch = glim_amd::align_icp({{tree.get(), source.get(), I, 0.5}, {tree.get(), source.get(), I, 0.25}}, prm);
  REQUIRE(batch.size() == 2);
  const auto single = glim_amd::align_icp(*tree, *source, I, 0.5, prm);
  REQUIRE(std::memcmp(&single.raw, &batch[0].raw, sizeof(single.raw)) == 0);
  REQUIRE(single.status >= GLIM_AMD_ALIGN_CONVERGED && single.status <= GLIM_AMD_ALIGN_LAMBDA_BOUND && single.iterations >= 1 && single.error < L.error);
  values[1] = single.T_target_source;
  const glim_amd::LinearizedSystem6 E = f.linearize(values);
  REQUIRE(E.error == single.error && E.num_inliers == single.num_inliers && std::memcmp(E.H_ss, single.information.data(), sizeof(E.H_ss)) == 0);
  std::printf("test_icp_align OK (%d points, error %.6g -> %.6g in %d iterations)\n", n, L.error, single.error, single.iterations);
  return 0;
}
