// test_ct_adapter.cpp -- compiles the continuous-time factor of adapters/gtsam/glim_amd_gtsam.hpp (IntegratedCT_GICPFactorHIP) against the
// stand-in headers of tests/cpp/mock/ and checks that the gtsam::HessianFactor it returns holds exactly the C record of the same evaluation
// (odometry_estimation_ct.cpp:158-195).  Built by tests/test_ct_adapter.py like test_adapter.cpp.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include <glim_amd_gtsam.hpp>

using namespace glim_amd;

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                              \
    }                                                                        \
  } while (0)

// three walls of a room corner seen from (ox, oy, yaw); FP32-representable coordinates
static std::vector<Eigen::Vector4d> make_scan(int n, double ox, double oy, double yaw, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::normal_distribution<double> G(0.0, 0.005);
  std::vector<Eigen::Vector4d> pts((size_t)n);
  const double c = std::cos(yaw), s = std::sin(yaw);
  for (int i = 0; i < n; i++) {
    double x, y, z;
    if (i % 3 == 0) { x = 8.0 * U(rng); y = 6.0 * U(rng); z = -1.5 + G(rng); }
    else if (i % 3 == 1) { x = 8.0 + G(rng); y = 6.0 * U(rng); z = -1.5 + 3.0 * U(rng); }
    else { x = 8.0 * U(rng); y = 6.0 + G(rng); z = -1.5 + 3.0 * U(rng); }
    const double wx = x - ox, wy = y - oy;
    pts[(size_t)i][0] = (double)(float)(c * wx + s * wy);
    pts[(size_t)i][1] = (double)(float)(-s * wx + c * wy);
    pts[(size_t)i][2] = (double)(float)z;
    pts[(size_t)i][3] = 1.0;
  }
  return pts;
}

static gtsam::Pose3 pose2d(double x, double y, double yaw) {
  Eigen::Matrix4d T = Eigen::Matrix4d::Identity();
  T(0, 0) = std::cos(yaw); T(0, 1) = -std::sin(yaw); T(1, 0) = std::sin(yaw); T(1, 1) = std::cos(yaw);
  T(0, 3) = x; T(1, 3) = y;
  return gtsam::Pose3(T);
}

static bool same(const gtsam::Matrix& G, const double* ref) {
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++)
      if (G(r, c) != ref[6 * r + c]) return false;
  return true;
}
static bool same_neg(const gtsam::Vector& g, const double* b) {
  for (int r = 0; r < 6; r++)
    if (g(r) != -b[r]) return false;
  return true;
}

int main() {
  if (glim_amd_device_count() < 1) {
    std::fprintf(stderr, "no HIP device: this test must run on the GPU box\n");
    return 2;
  }
  const int n = 20000, k = 10;
  std::vector<Eigen::Vector4d> pt = make_scan(n, 0.0, 0.0, 0.0, 1), ps = make_scan(n, 1.0, 1.0, 0.05, 2);
  std::vector<double> times((size_t)n);
  for (int i = 0; i < n; i++) times[(size_t)i] = 0.1 * i / n;  // a 0.1 s sweep, ~100 buckets
  gtsam_points::PointCloud vt, vs;
  vt.num_points = vs.num_points = (size_t)n;
  vt.points = pt.data();
  vs.points = ps.data();
  auto ft = glim_amd::clone(vt), fs = glim_amd::clone(vs);
  for (auto& f : {ft, fs}) {
    f->find_neighbors(k);
    f->estimate_covariances(k);
  }
  const gtsam::Key X = 0, Y = 1;
  auto tree = std::make_shared<NearestNeighborSearchGPU>(ft, 1.0);
  IntegratedCT_GICPFactorHIP factor(X, Y, ft, fs, tree, times.data());
  factor.set_max_correspondence_distance(1.0);
  factor.set_num_threads(4);
  REQUIRE(factor.keys().size() == 2 && factor.keys()[0] == X && factor.keys()[1] == Y && factor.dim() == 6);

  gtsam::Values values;
  values.insert(X, pose2d(1.0, 1.0, 0.05));
  values.insert(Y, pose2d(1.02, 1.01, 0.06));
  auto g = factor.linearize(values);
  auto* hf = dynamic_cast<gtsam::HessianFactor*>(g.get());
  REQUIRE(hf != nullptr && hf->keys.size() == 2 && hf->keys[0] == X && hf->keys[1] == Y);

  // the same evaluation through the C ABI directly
  glim_amd_ct_gicp_factor* c = nullptr;
  REQUIRE(glim_amd_ct_gicp_create(tree->handle(), fs->handle(), times.data(), &c) == GLIM_AMD_OK);
  const Isometry3d Xi = to_iso(values.at<gtsam::Pose3>(X)), Yi = to_iso(values.at<gtsam::Pose3>(Y));
  glim_amd_ct_linearized rec{};
  REQUIRE(glim_amd_ct_gicp_linearize(c, Xi.m.data(), Yi.m.data(), &rec) == GLIM_AMD_OK);
  REQUIRE(rec.num_inliers > n / 2);
  REQUIRE(same(hf->G11, rec.H_00) && same(hf->G12, rec.H_01) && same(hf->G22, rec.H_11));
  REQUIRE(same_neg(hf->g1, rec.b_0) && same_neg(hf->g2, rec.b_1));
  REQUIRE(hf->f == rec.error);
  double e = 0.0;
  REQUIRE(glim_amd_ct_gicp_error(c, Xi.m.data(), Yi.m.data(), &e, nullptr) == GLIM_AMD_OK);
  REQUIRE(factor.error(values) == e);
  const std::vector<Eigen::Vector4d> d = factor.deskewed_source_points(values, true);
  REQUIRE(d.size() == (size_t)n);
  REQUIRE(std::fabs(d[0].data()[0] - ps[0].data()[0]) < 1e-9 && d[0].data()[3] == 1.0);  // the first bucket's pose is the local frame
  auto cl = std::dynamic_pointer_cast<IntegratedCT_GICPFactorHIP>(factor.clone());
  REQUIRE(cl && cl->error(values) == e);
  glim_amd_ct_gicp_destroy(c);
  std::printf("test_ct_adapter OK: %lld inliers, error %.6f\n", (long long)rec.num_inliers, rec.error);
  return 0;
}
