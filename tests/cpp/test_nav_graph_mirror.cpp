// The C++ mirror of the graph with velocity and bias nodes (include/glim_amd/graph_align.hpp: NavGraph, ImuTerm, optimize_nav_graph): the
// compile-and-link check, what the graph records, and an empty problem (no device is touched).
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
  static_assert(sizeof(glim_amd_nav_vector_prior) == 344 && sizeof(glim_amd_nav_vector_between) == 344 && sizeof(glim_amd_nav_imu_term) == 1256 &&
                    sizeof(glim_amd_nav_terms) == 48 && sizeof(glim_amd_nav_result) == 88,
                "the layout of the new structs");
  glim_amd::NavGraph g;
  const int x0 = g.add_pose(glim_amd::Isometry3d()), v0 = g.add_velocity({1.0, 2.0, 3.0}), b0 = g.add_bias({1.0, 2.0, 3.0, 4.0, 5.0, 6.0});
  const int x1 = g.add_pose(glim_amd::Isometry3d()), v1 = g.add_velocity({0.0, 0.0, 0.0}), b1 = g.add_bias({0.0, 0.0, 0.0, 0.0, 0.0, 0.0});
  REQUIRE(x0 == 0 && v0 == 1 && b0 == 2 && x1 == 3 && v1 == 4 && b1 == 5 && g.values.size() == 72);
  REQUIRE(g.kinds[v0] == GLIM_AMD_NODE_VELOCITY && g.kinds[b0] == GLIM_AMD_NODE_BIAS && g.kinds[x1] == GLIM_AMD_NODE_POSE);
  REQUIRE(g.values[12 * v0 + 2] == 3.0 && g.values[12 * v0 + 3] == 0.0 && g.values[12 * b0 + 5] == 6.0 && g.values[12 * b0 + 6] == 0.0);
  g.add_velocity_prior(v0, {1.0, 2.0, 3.0}, {1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0});
  REQUIRE(g.vector_priors[0].information[0] == 1.0 && g.vector_priors[0].information[6] == 4.0 && g.vector_priors[0].information[14] == 9.0 &&
          g.vector_priors[0].information[3] == 0.0);
  g.add_bias_prior(b0, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, glim_amd::BundleGraph::isotropic(1e6));
  g.add_bias_between(b0, b1, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, glim_amd::BundleGraph::isotropic(1e6));
  g.add_velocity_between(v0, v1, {0.0, 0.0, 0.0}, {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0});
  REQUIRE(g.vector_betweens.size() == 2 && g.vector_betweens[1].node_j == v1 && g.vector_betweens[1].information[7] == 1.0);
  glim_amd::ImuTerm t;
  t.pose_i = x0, t.velocity_i = v0, t.pose_j = x1, t.velocity_j = v1, t.bias = b0;
  t.dt = 0.1;
  t.gravity = {0.0, 0.0, -9.81};
  t.mode = GLIM_AMD_IMU_MANIFOLD;
  g.add_imu(t);
  REQUIRE(g.imu_terms.size() == 1 && g.imu_terms[0].bias == b0 && g.imu_terms[0].dt == 0.1 && g.imu_terms[0].gravity[2] == -9.81 && g.imu_terms[0].mode == 1);
  g.graph.add_damping(b0, 1e6);  // LinearDampingFactor(B(0), 6, 1e6)
  REQUIRE(g.graph.dampings.size() == 1);
  const glim_amd::NavGraphResult r = glim_amd::optimize_nav_graph(glim_amd::NavGraph());  // no nodes: answered before any device call
  REQUIRE(r.values.empty() && r.status == 0 && r.imu_cost == 0.0);
  std::printf("test_nav_graph_mirror OK\n");
  return 0;
}
