// The C++ mirror of the scan-to-keyframes VGICP registration (include/glim_amd/keyframe_align.hpp) on a case the Python test dumped: one problem,
// one source over K keyframe clouds with a voxel map per resolution each, returns the bytes vgicp_align_keyframes returned in that process.
//   test_keyframe_align <case.bin>   int32 K, int32 L, int32 n_source, K x int32 keyframe sizes, then doubles: per keyframe n x 4 points and
//                                    n x 16 covariances (column-major 4 x 4) and 12 of its pose, the same points and covariances for the
//                                    source, L resolutions, 12 of X_init, then the expected row: 12 pose, error, inlier_fraction, iterations,
//                                    trials, status, 36 information, and K x L x 29 factor records (keyframe-major)
// Without an argument: the compile-and-link check only (no device is touched).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include <glim_amd/keyframe_align.hpp>

#define REQUIRE(c)                                                \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s (%s:%d)\n", #c, __FILE__, __LINE__); \
      return 1;                                                   \
    }                                                             \
  } while (0)

static bool read_d(std::FILE* f, std::vector<double>& v, std::size_t n) {
  v.resize(n);
  return std::fread(v.data(), sizeof(double), n, f) == n;
}

int main(int argc, char** argv) {
  static_assert(GLIM_AMD_KEYFRAME_ALIGN_MAX_TARGETS == 64, "the cap glim_amd/api.py names");
  {
    glim_amd_lm_params d;
    REQUIRE(glim_amd_keyframe_align_default_params(&d) == GLIM_AMD_OK);
    const glim_amd_lm_params m = glim_amd::LMParams().c();
    REQUIRE(std::memcmp(&d, &m, sizeof(d)) == 0);
    REQUIRE(glim_amd::align_to_keyframes(std::vector<glim_amd::KeyframeAlignProblem>{}).empty());  // an empty batch: answered before any device call
  }
  if (argc < 2) {
    std::printf("test_keyframe_align OK (no case given: nothing run)\n");
    return 0;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f != nullptr);
  std::int32_t head[3];
  REQUIRE(std::fread(head, sizeof(std::int32_t), 3, f) == 3 && head[0] > 0 && head[1] > 0 && head[2] > 0);
  const std::size_t K = (std::size_t)head[0], L = (std::size_t)head[1], ns = (std::size_t)head[2];
  std::vector<std::int32_t> sizes(K);
  REQUIRE(std::fread(sizes.data(), sizeof(std::int32_t), K, f) == K);
  std::vector<glim_amd::PointCloudGPU::Ptr> clouds;
  std::vector<glim_amd::Isometry3d> poses(K);
  std::vector<double> p, c, pose, res, X0, want, want_records;
  for (std::size_t k = 0; k < K; k++) {
    const std::size_t n = (std::size_t)sizes[k];
    REQUIRE(read_d(f, p, n * 4) && read_d(f, c, n * 16) && read_d(f, pose, 12));
    clouds.push_back(glim_amd::PointCloudGPU::clone(p.data(), c.data(), nullptr, (std::int64_t)n));
    for (int u = 0; u < 12; u++) poses[k].m[u] = pose[u];
  }
  REQUIRE(read_d(f, p, ns * 4) && read_d(f, c, ns * 16) && read_d(f, res, L) && read_d(f, X0, 12) && read_d(f, want, 53) && read_d(f, want_records, K * L * 29));
  std::fclose(f);
  auto source = glim_amd::PointCloudGPU::clone(p.data(), c.data(), nullptr, (std::int64_t)ns);
  std::vector<std::unique_ptr<glim_amd::GaussianVoxelMapGPU>> maps;
  glim_amd::KeyframeAlignProblem problem{source.get(), {}, glim_amd::Isometry3d()};
  for (int u = 0; u < 12; u++) problem.X_init.m[u] = X0[u];
  for (std::size_t k = 0; k < K; k++)
    for (std::size_t l = 0; l < L; l++) {
      maps.push_back(std::make_unique<glim_amd::GaussianVoxelMapGPU>((float)res[l]));
      maps.back()->insert(*clouds[k]);
      problem.targets.push_back({maps.back().get(), poses[k]});
    }
  std::vector<double> records;
  const auto out = glim_amd::align_to_keyframes({problem}, glim_amd::LMParams(), false, &records);
  REQUIRE(out.size() == 1 && records.size() == K * L * 29);
  const glim_amd::AlignResult& r = out[0];
  const double* w = want.data();
  REQUIRE(std::memcmp(r.T_target_source.m.data(), w, 12 * sizeof(double)) == 0 && r.error == w[12] && r.inlier_fraction == w[13]);
  REQUIRE(r.iterations == (int)w[14] && r.trials == (int)w[15] && r.status == (int)w[16]);
  REQUIRE(std::memcmp(r.information.data(), w + 17, 36 * sizeof(double)) == 0);
  REQUIRE(std::memcmp(records.data(), want_records.data(), records.size() * sizeof(double)) == 0);
  REQUIRE(r.status >= GLIM_AMD_ALIGN_CONVERGED && r.status <= GLIM_AMD_ALIGN_LAMBDA_BOUND && r.num_inliers > 0);
  std::printf("test_keyframe_align OK (%zu keyframes x %zu levels, %zu source points)\n", K, L, ns);
  return 0;
}
