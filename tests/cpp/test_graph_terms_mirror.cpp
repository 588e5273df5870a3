// The C++ mirror of the damping terms and the Huber widths (include/glim_amd/bundle_align.hpp, graph_align.hpp): the compile-and-link check,
// what the graph records, which entry point it selects, and an empty problem (no device is touched).
#include <cstdio>
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
  static_assert(sizeof(glim_amd_graph_damping) == 56 && sizeof(glim_amd_graph_terms) == 24, "the layout of the new structs");
  glim_amd::BundleGraph g;
  const auto info = glim_amd::BundleGraph::isotropic(400.0);
  g.add_between(0, 1, glim_amd::Isometry3d(), info);  // the odometry chain stays Gaussian
  REQUIRE(!g.has_terms() && g.between_huber_width.size() == 1 && g.between_huber_width[0] == 0.0);
  g.add_between(1, 0, glim_amd::Isometry3d(), glim_amd::BundleGraph::isotropic(100.0), 1.0);  // a loop factor under Robust(Huber(1.0), ...)
  REQUIRE(g.has_terms() && g.between_huber_width.size() == g.betweens.size() && g.between_huber_width[1] == 1.0);
  glim_amd::BundleGraph h;
  h.add_between(0, 1, glim_amd::Isometry3d(), info);
  h.add_damping(0, 1e6);  // LinearDampingFactor(X(0), 6, 1e6)
  h.add_damping(1, {0.0, 0.0, 1e6, 0.0, 0.0, 0.0});  // the per-axis form
  REQUIRE(h.has_terms() && h.dampings.size() == 2 && h.dampings[0].pose == 0 && h.dampings[1].pose == 1);
  for (int k = 0; k < 6; k++) REQUIRE(h.dampings[0].diagonal[k] == 1e6 && h.dampings[1].diagonal[k] == (k == 2 ? 1e6 : 0.0));
  const glim_amd::BundleResult r = glim_amd::optimize_graph(h, {});  // no poses: answered before any device call
  REQUIRE(r.poses.empty() && r.between_weights.empty() && r.status == 0);
  const glim_amd::BundleResult r2 = glim_amd::optimize_bundle(g, {});
  REQUIRE(r2.poses.empty() && r2.between_weights.empty());
  std::printf("test_graph_terms_mirror OK\n");
  return 0;
}
