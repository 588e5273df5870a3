// The C++ mirror of the CT-GICP frame alignment (include/glim_amd/ct_align.hpp) on a case the Python test dumped: glim_amd::align_ct and the
// compat class's align return the bytes IntegratedCT_GICPFactor.align returned in that process.
//   test_ct_align <case.bin>   int32 n_target, int32 n_source, then doubles: n_target x 4 points, n_target x 16 covariances (column-major
//                              4 x 4), the same for the source, n_source times, max_correspondence_distance, 12 + 12 of the initial pair,
//                              26 of the terms, then the bytes of the expected glim_amd_ct_align_result
// Without an argument: the compile-and-link check only (no device is touched).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <glim_amd/ct_align.hpp>

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
  static_assert(sizeof(glim_amd_ct_align_terms) == 208 && sizeof(glim_amd_ct_align_result) == 1216, "the layouts glim_amd/_lib.py binds");
  {
    glim_amd_lm_params d;
    REQUIRE(glim_amd_ct_align_default_params(&d) == GLIM_AMD_OK);
    const glim_amd_lm_params m = glim_amd::ct_align_params().c();
    REQUIRE(std::memcmp(&d, &m, sizeof(d)) == 0);
  }
  if (argc < 2) {
    std::printf("test_ct_align OK (no case given: nothing run)\n");
    return 0;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f != nullptr);
  std::int32_t head[2];
  REQUIRE(std::fread(head, sizeof(std::int32_t), 2, f) == 2 && head[0] > 0 && head[1] > 0);
  const std::size_t nt = (std::size_t)head[0], ns = (std::size_t)head[1];
  std::vector<double> tp, tc, sp, sc, times, dist, XY, terms;
  REQUIRE(read_d(f, tp, nt * 4) && read_d(f, tc, nt * 16) && read_d(f, sp, ns * 4) && read_d(f, sc, ns * 16) && read_d(f, times, ns) && read_d(f, dist, 1) &&
          read_d(f, XY, 24) && read_d(f, terms, 26));
  glim_amd_ct_align_result want;
  REQUIRE(std::fread(&want, sizeof(want), 1, f) == 1);
  std::fclose(f);
  auto target = glim_amd::PointCloudGPU::clone(tp.data(), tc.data(), nullptr, (std::int64_t)nt);
  auto source = glim_amd::PointCloudGPU::clone(sp.data(), sc.data(), nullptr, (std::int64_t)ns);
  auto tree = std::make_shared<glim_amd::NearestNeighborSearchGPU>(target, dist[0]);
  glim_amd::IntegratedCT_GICPFactor factor(0, 1, target, source, tree, times.data());
  factor.set_max_correspondence_distance(dist[0]);
  glim_amd::Values values;
  glim_amd::Isometry3d P, D;
  for (int k = 0; k < 12; k++) {
    values[0].m[k] = XY[k];
    values[1].m[k] = XY[12 + k];
    P.m[k] = terms[k];
    D.m[k] = terms[13 + k];
  }
  glim_amd::CtAlignTerms t;
  t.location(P, terms[12]).between(D, terms[25]);
  const glim_amd::CtAlignResult a = glim_amd::align_ct(factor, values, t);
  const glim_amd::CtAlignResult b = factor.align(values, t, glim_amd::ct_align_params());
  for (const glim_amd::CtAlignResult* r : {&a, &b}) {
    REQUIRE(std::memcmp(&r->raw, &want, sizeof(want)) == 0);
    REQUIRE(std::memcmp(r->X.m.data(), want.X, sizeof(want.X)) == 0 && std::memcmp(r->Y.m.data(), want.Y, sizeof(want.Y)) == 0);
    REQUIRE(r->status == want.status && r->iterations == want.iterations && r->trials == want.trials && r->cost == want.cost);
    REQUIRE(r->num_inliers == want.linearized.num_inliers && r->num_inliers > 0);
  }
  std::printf("test_ct_align OK (%zu x %zu points, status %d, %d iterations)\n", nt, ns, a.status, a.iterations);
  return 0;
}
