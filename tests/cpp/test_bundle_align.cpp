// The C++ mirror of the sub-map bundle optimisation (include/glim_amd/bundle_align.hpp): the compile-and-link check, the defaults and an empty
// problem (no device is touched).
#include <cstdio>
#include <cstring>
#include <vector>

#include <glim_amd/bundle_align.hpp>

#define REQUIRE(c)                                                \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s (%s:%d)\n", #c, __FILE__, __LINE__); \
      return 1;                                                   \
    }                                                             \
  } while (0)

int main() {
  static_assert(sizeof(glim_amd_bundle_prior) == 392 && sizeof(glim_amd_bundle_between) == 392 && sizeof(glim_amd_bundle_result) == 64,
                "the layouts glim_amd/_lib.py binds");
  static_assert(GLIM_AMD_BUNDLE_MAX_POSES >= 20 && GLIM_AMD_BUNDLE_MAX_FACTORS >= 380, "configs[2]: 20 keyframes, 380 factors");
  glim_amd_lm_params d;
  REQUIRE(glim_amd_bundle_align_default_params(&d) == GLIM_AMD_OK);
  const glim_amd_lm_params m = glim_amd::bundle_params().c();
  REQUIRE(d.lambda_initial == m.lambda_initial && d.lambda_factor == m.lambda_factor && d.lambda_upper_bound == m.lambda_upper_bound &&
          d.lambda_lower_bound == m.lambda_lower_bound && d.relative_error_tol == m.relative_error_tol && d.absolute_error_tol == m.absolute_error_tol &&
          d.max_iterations == 20 && m.max_iterations == 20 && d.max_trials == m.max_trials && d.error_scale == m.error_scale);
  glim_amd::BundleGraph g;
  g.add_prior(0, glim_amd::Isometry3d(), glim_amd::BundleGraph::isotropic(1e6));
  REQUIRE(g.priors.size() == 1 && g.priors[0].information[7] == 1e6 && g.priors[0].information[1] == 0.0);
  const glim_amd::BundleResult r = glim_amd::optimize_bundle(g, {});  // no poses: answered before any device call
  REQUIRE(r.poses.empty() && r.status == 0 && r.iterations == 0);
  std::printf("test_bundle_align OK (no case given: nothing run)\n");
  return 0;
}
