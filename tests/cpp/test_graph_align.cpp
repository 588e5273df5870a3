// The C++ mirror of the global-graph optimisation (include/glim_amd/graph_align.hpp): the compile-and-link check, the caps, the defaults and
// an empty problem (no device is touched).
#include <cstdio>
#include <cstring>
#include <vector>

#include <glim_amd/graph_align.hpp>

#define REQUIRE(c)                                                \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s (%s:%d)\n", #c, __FILE__, __LINE__); \
      return 1;                                                   \
    }                                                             \
  } while (0)

int main() {
  static_assert(GLIM_AMD_GRAPH_MAX_POSES == 256 && GLIM_AMD_GRAPH_MAX_FACTORS >= 32640 && GLIM_AMD_GRAPH_MAX_TERMS >= 1024,
                "configs[3]: 256 sub-maps, all 32 640 pairs");
  glim_amd_lm_params d, b;
  REQUIRE(glim_amd_graph_align_default_params(&d) == GLIM_AMD_OK && glim_amd_bundle_align_default_params(&b) == GLIM_AMD_OK);
  REQUIRE(!std::memcmp(&d, &b, sizeof(d)));
  const glim_amd_lm_params m = glim_amd::graph_params().c();
  REQUIRE(d.lambda_initial == m.lambda_initial && d.lambda_factor == m.lambda_factor && d.lambda_upper_bound == m.lambda_upper_bound &&
          d.lambda_lower_bound == m.lambda_lower_bound && d.relative_error_tol == m.relative_error_tol && d.absolute_error_tol == m.absolute_error_tol &&
          d.max_iterations == 20 && m.max_iterations == 20 && d.max_trials == m.max_trials && d.error_scale == m.error_scale);
  glim_amd::BundleGraph g;
  g.add_prior(0, glim_amd::Isometry3d(), glim_amd::BundleGraph::isotropic(1e6));
  const glim_amd::BundleResult r = glim_amd::optimize_graph(g, {});  // no poses: answered before any device call
  REQUIRE(r.poses.empty() && r.status == 0 && r.iterations == 0);
  const glim_amd::BundleResult r2 = glim_amd::optimize_bundle(g, {});
  REQUIRE(r2.poses.empty());
  std::printf("test_graph_align OK\n");
  return 0;
}
