// test_ivox_adapter.cpp -- compiles the device iVox mirror (glim_amd::IncrementalVoxelMap) and the factors over it (IntegratedGICPFactorHIP,
// IntegratedCT_GICPFactorHIP of adapters/gtsam/glim_amd_gtsam.hpp) against the stand-in headers of tests/cpp/mock/ and checks that the
// gtsam::HessianFactor blocks hold exactly the C records of the same evaluations over the same map (odometry_estimation_ct.cpp:56-63,
// :158-162, :229-235).  Built by tests/test_ivox_adapter.py like test_ct_adapter.cpp.
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
  // the map as odometry_estimation_ct.cpp:56-63 sets it up (a finer leaf: at 1 m every cell of these dense walls is full after one insert and
  // the second insert below would change nothing), then insert(frame) with the frame's pose
  auto ivox = std::make_shared<IncrementalVoxelMap>(0.25);
  IncrementalVoxelMap::InsertionSetting setting;
  setting.min_dist_in_cell = 0.05;
  ivox->set_voxel_insertion_setting(setting);
  ivox->set_lru_horizon(30);
  ivox->set_neighbor_voxel_mode(1);
  ivox->insert(*ft, to_iso(pose2d(0.0, 0.0, 0.0)));
  REQUIRE(ivox->num_voxels() > 50 && ivox->size() > 1000 && ivox->size() <= (size_t)n && ivox->leaf_size() == 0.25);
  REQUIRE(ivox->voxel_points().size() == 4 * ivox->size());
  IncrementalVoxelMap::InsertionSetting late;
  bool refused = false;
  try {
    ivox->set_voxel_insertion_setting(late);
  } catch (const std::exception&) {
    refused = true;
  }
  REQUIRE(refused);  // the cell size is fixed once the map holds points

  const gtsam::Key X = 0, Y = 1;
  gtsam::Values values;
  values.insert(X, pose2d(1.0, 1.0, 0.05));
  values.insert(Y, pose2d(1.02, 1.01, 0.06));
  const Isometry3d Xi = to_iso(values.at<gtsam::Pose3>(X)), Yi = to_iso(values.at<gtsam::Pose3>(Y));

  // rigid GICP over the map (unary): blocks equal the C record
  IntegratedGICPFactorHIP rigid(gtsam::Pose3(Eigen::Matrix4d::Identity()), Y, ivox, fs);
  auto gr = rigid.linearize(values);
  auto* hr = dynamic_cast<gtsam::HessianFactor*>(gr.get());
  REQUIRE(hr != nullptr && hr->keys.size() == 1 && hr->keys[0] == Y);
  glim_amd_linearized6 r6{};
  REQUIRE(glim_amd_ivox_gicp_linearize(ivox->handle(), fs->handle(), Yi.m.data(), 1.0, 0u, &r6) == GLIM_AMD_OK);
  REQUIRE(r6.num_inliers > n / 4);
  REQUIRE(same(hr->G11, r6.H_ss) && same_neg(hr->g1, r6.b_s));

  // the continuous-time factor over the map: the constructor of odometry_estimation_ct.cpp:158-160
  IntegratedCT_GICPFactorHIP factor(X, Y, ivox, fs, ivox, times.data());
  factor.set_max_correspondence_distance(2.0);  // config_odometry_ct.json; any distance is accepted over a map
  factor.set_num_threads(4);
  REQUIRE(factor.keys().size() == 2 && factor.keys()[0] == X && factor.keys()[1] == Y && factor.dim() == 6);
  auto g = factor.linearize(values);
  auto* hf = dynamic_cast<gtsam::HessianFactor*>(g.get());
  REQUIRE(hf != nullptr && hf->keys.size() == 2 && hf->keys[0] == X && hf->keys[1] == Y);
  glim_amd_ct_gicp_factor* c = nullptr;
  REQUIRE(glim_amd_ivox_ct_factor_create(ivox->handle(), fs->handle(), times.data(), &c) == GLIM_AMD_OK);
  REQUIRE(glim_amd_ct_gicp_set_max_correspondence_distance(c, 2.0) == GLIM_AMD_OK);
  glim_amd_ct_linearized rec{};
  REQUIRE(glim_amd_ct_gicp_linearize(c, Xi.m.data(), Yi.m.data(), &rec) == GLIM_AMD_OK);
  REQUIRE(rec.num_inliers > n / 4);
  REQUIRE(same(hf->G11, rec.H_00) && same(hf->G12, rec.H_01) && same(hf->G22, rec.H_11));
  REQUIRE(same_neg(hf->g1, rec.b_0) && same_neg(hf->g2, rec.b_1));
  REQUIRE(hf->f == rec.error);
  double e = 0.0;
  REQUIRE(glim_amd_ct_gicp_error(c, Xi.m.data(), Yi.m.data(), &e, nullptr) == GLIM_AMD_OK);
  REQUIRE(factor.error(values) == e);
  // the map refuses to go while a factor on it lives
  REQUIRE(glim_amd_ivox_destroy(ivox->handle()) == GLIM_AMD_ERR_STATE);
  // an insert between linearize and error: both factors see the new map (their kept correspondences are dropped)
  ivox->insert(*fs, Xi);
  double e2 = 0.0;
  REQUIRE(glim_amd_ct_gicp_error(c, Xi.m.data(), Yi.m.data(), &e2, nullptr) == GLIM_AMD_OK);
  REQUIRE(factor.error(values) == e2 && e2 != e);
  glim_amd_ct_gicp_destroy(c);
  std::printf("test_ivox_adapter OK: %lld inliers, error %.6f -> %.6f after the insert, %zu voxels\n", (long long)rec.num_inliers, e, e2, ivox->num_voxels());
  return 0;
}
