// The C++ mirror of the VGICP fine registration (include/glim_amd/vgicp_align.hpp) on a case the Python test dumped: the batch form and the single
// form return the bytes vgicp_align_batch returned in that process.
//   test_vgicp_align <case.bin>   int32 n_target, int32 n_source, int32 B, then doubles: n_target x 4 points, n_target x 16 covariances
//                                 (column-major 4 x 4), the same for the source, the voxel resolution, B x 12 initial poses,
//                                 B x (12 pose, error, inlier_fraction, iterations, trials, status, 36 information) expected from the batch,
//                                 then the same B rows expected from each problem run alone
// Without an argument: the compile-and-link check only (no device is touched).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <glim_amd/vgicp_align.hpp>

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

static bool same(const glim_amd::AlignResult& r, const double* w) {
  return std::memcmp(r.T_target_source.m.data(), w, 12 * sizeof(double)) == 0 && r.error == w[12] && r.inlier_fraction == w[13] && r.iterations == (int)w[14] &&
         r.trials == (int)w[15] && r.status == (int)w[16] && std::memcmp(r.information.data(), w + 17, 36 * sizeof(double)) == 0;
}

int main(int argc, char** argv) {
  static_assert(sizeof(glim_amd_lm_params) == 64 && sizeof(glim_amd_align_result) == 368, "the layouts glim_amd/_lib.py binds");
  {
    glim_amd_lm_params d;
    REQUIRE(glim_amd_vgicp_align_default_params(&d) == GLIM_AMD_OK);
    const glim_amd_lm_params m = glim_amd::LMParams().c();
    REQUIRE(std::memcmp(&d, &m, sizeof(d)) == 0);
    REQUIRE(glim_amd::align_vgicp(std::vector<glim_amd::VGICPAlignProblem>{}).empty());  // an empty batch: answered before any device call
  }
  if (argc < 2) {
    std::printf("test_vgicp_align OK (no case given: nothing run)\n");
    return 0;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f != nullptr);
  std::int32_t head[3];
  REQUIRE(std::fread(head, sizeof(std::int32_t), 3, f) == 3 && head[0] > 0 && head[1] > 0 && head[2] > 0);
  const std::size_t nt = (std::size_t)head[0], ns = (std::size_t)head[1], B = (std::size_t)head[2];
  std::vector<double> tp, tc, sp, sc, res, T0, want, want_alone;
  REQUIRE(read_d(f, tp, nt * 4) && read_d(f, tc, nt * 16) && read_d(f, sp, ns * 4) && read_d(f, sc, ns * 16) && read_d(f, res, 1) && read_d(f, T0, B * 12) &&
          read_d(f, want, B * 53) && read_d(f, want_alone, B * 53));
  std::fclose(f);
  auto target = glim_amd::PointCloudGPU::clone(tp.data(), tc.data(), nullptr, (std::int64_t)nt);
  auto source = glim_amd::PointCloudGPU::clone(sp.data(), sc.data(), nullptr, (std::int64_t)ns);
  glim_amd::GaussianVoxelMapGPU voxels((float)res[0]);
  voxels.insert(*target);
  std::vector<glim_amd::VGICPAlignProblem> problems;
  for (std::size_t i = 0; i < B; i++) {
    glim_amd::Isometry3d T;
    for (int k = 0; k < 12; k++) T.m[k] = T0[12 * i + k];
    problems.push_back({&voxels, source.get(), T});
  }
  const auto batch = glim_amd::align_vgicp(problems);
  REQUIRE(batch.size() == B);
  for (std::size_t i = 0; i < B; i++) {
    REQUIRE(same(batch[i], want.data() + 53 * i));
    REQUIRE(same(glim_amd::align_vgicp(voxels, *source, problems[i].T_init), want_alone.data() + 53 * i));
    REQUIRE(batch[i].status >= GLIM_AMD_ALIGN_CONVERGED && batch[i].status <= GLIM_AMD_ALIGN_LAMBDA_BOUND && batch[i].num_inliers > 0);
  }
  std::printf("test_vgicp_align OK (%zu x %zu points, %zu problems)\n", nt, ns, B);
  return 0;
}
