// graph_align.hpp -- header-only C++17 mirror, over the C ABI (glim_amd.h "Global-graph optimisation"), of one batch optimisation over the
// poses of GLIM's global graph: Levenberg-Marquardt over the sub-map poses on the pairwise binary VGICP factors between sub-maps
// (global_mapping.cpp:430-484) and that file's pose-only relative-pose factors -- graph in, poses out, one call.  The graph, the result and the
// parameters are bundle_align.hpp's; the caps are GLIM_AMD_GRAPH_MAX_*.  Within the bundle's caps the result is optimize_bundle's, bit for bit.
// BundleGraph::add_damping (LinearDampingFactor) and add_between's Huber width send the graph through glim_amd_graph_align_terms.
// NavGraph and optimize_nav_graph below: the same optimisation over pose, velocity and bias nodes with vector priors, vector betweens and
// IMU terms (glim_amd.h "Graph optimisation with velocity and bias variables"; glim_amd_graph_align_nav).
// Out of scope: ISAM2, pose marginals, CombinedImuFactor, IMU terms in the LDS bundle, robust priors, M-estimators other than Huber, several
// devices, translating a gtsam::NonlinearFactorGraph.
//
//   glim_amd::BundleGraph g;
//   g.add_factor(*submaps[i]->voxelmaps.back(), *submaps[j]->frame, i, j);   // IntegratedVGICPFactorGPU(X(i), X(j), ...)
//   g.add_between(i, i + 1, delta, information);                            // BetweenFactor<Pose3>(X(i), X(i + 1), delta, ...)
//   g.add_between(i, j, loop, information, 1.0);                            // ... with Robust(Huber(1.0), ...): a loop factor
//   g.add_damping(0, 1e6);                                                  // LinearDampingFactor(X(0), 6, init_pose_damping_scale)
//   g.add_prior(0, T0, information);
//   auto r = glim_amd::optimize_graph(g, initial_poses);                     // r.poses[k], r.cost, r.status
#pragma once

#include "bundle_align.hpp"

namespace glim_amd {

inline LMParams graph_params() { return bundle_params(); }  // glim_amd_graph_align_default_params

inline BundleResult optimize_graph(const BundleGraph& g, const std::vector<Isometry3d>& initial, const LMParams& params = graph_params()) {
  return detail::optimize_poses([](auto... a) { return glim_amd_graph_align(a...); }, [](auto... a) { return glim_amd_graph_align_terms(a...); },
                                "optimize_graph", g, initial, params);
}

// ---- pose, velocity and bias nodes (sub_mapping.cpp:218-243, global_mapping.cpp:168-216 with enable_imu = true) ----
//   glim_amd::NavGraph g;
//   int x = g.add_pose(T), v = g.add_velocity({vx, vy, vz}), b = g.add_bias({ax, ay, az, gx, gy, gz});   // X(i), V(i), B(i)
//   g.add_velocity_prior(v, v0, info3);  g.add_bias_prior(b, b0, info6);                                 // PriorFactor<Vector3>, <ConstantBias>
//   g.add_bias_between(b, b2, {}, info6);                                                                // BetweenFactor<ConstantBias>
//   g.add_imu(term);                                                                                     // ImuFactor(X, V, X2, V2, B)
//   g.graph.add_factor(...), add_prior(...), add_between(...), add_damping(...)                           // the pose terms, by node index
//   auto r = glim_amd::optimize_nav_graph(g);                                                            // r.values[12 k ..], r.imu_cost
struct ImuTerm {  // glim_amd_nav_imu_term with plain members; information: (rot, pos, vel) order, the inverse of preintMeasCov
  int pose_i = 0, velocity_i = 0, pose_j = 0, velocity_j = 0, bias = 0;
  int mode = GLIM_AMD_IMU_TANGENT;
  double dt = 0.0;
  std::array<double, 3> gravity{};
  std::array<double, 6> bias_hat{};
  std::array<double, 9> delta{};
  std::array<double, 54> H_bias{};
  std::array<double, 81> information{};
};

struct NavGraph {
  BundleGraph graph;                // factors, pose priors, pose betweens and dampings, by node index
  std::vector<std::int32_t> kinds;  // GLIM_AMD_NODE_* per node
  std::vector<double> values;       // 12 per node: a pose, or 6 / 3 leading values and +0.0
  std::vector<glim_amd_nav_vector_prior> vector_priors;
  std::vector<glim_amd_nav_vector_between> vector_betweens;
  std::vector<glim_amd_nav_imu_term> imu_terms;

  int add_pose(const Isometry3d& T) {
    kinds.push_back(GLIM_AMD_NODE_POSE);
    for (int u = 0; u < 12; u++) values.push_back(T.m[u]);
    return (int)kinds.size() - 1;
  }
  int add_bias(const std::array<double, 6>& acc_gyro) {
    kinds.push_back(GLIM_AMD_NODE_BIAS);
    for (int u = 0; u < 12; u++) values.push_back(u < 6 ? acc_gyro[u] : 0.0);
    return (int)kinds.size() - 1;
  }
  int add_velocity(const std::array<double, 3>& v) {
    kinds.push_back(GLIM_AMD_NODE_VELOCITY);
    for (int u = 0; u < 12; u++) values.push_back(u < 3 ? v[u] : 0.0);
    return (int)kinds.size() - 1;
  }
  void add_bias_prior(int node, const std::array<double, 6>& value, const std::array<double, 36>& information) {
    glim_amd_nav_vector_prior p{};
    p.node = node;
    for (int k = 0; k < 6; k++) p.value[k] = value[k];
    for (int k = 0; k < 36; k++) p.information[k] = information[k];
    vector_priors.push_back(p);
  }
  void add_velocity_prior(int node, const std::array<double, 3>& value, const std::array<double, 9>& information) {
    glim_amd_nav_vector_prior p{};
    p.node = node;
    for (int k = 0; k < 3; k++) p.value[k] = value[k];
    for (int k = 0; k < 9; k++) p.information[6 * (k / 3) + k % 3] = information[k];
    vector_priors.push_back(p);
  }
  void add_bias_between(int i, int j, const std::array<double, 6>& measurement, const std::array<double, 36>& information) {
    glim_amd_nav_vector_between b{};
    b.node_i = i, b.node_j = j;
    for (int k = 0; k < 6; k++) b.measurement[k] = measurement[k];
    for (int k = 0; k < 36; k++) b.information[k] = information[k];
    vector_betweens.push_back(b);
  }
  void add_velocity_between(int i, int j, const std::array<double, 3>& measurement, const std::array<double, 9>& information) {
    glim_amd_nav_vector_between b{};
    b.node_i = i, b.node_j = j;
    for (int k = 0; k < 3; k++) b.measurement[k] = measurement[k];
    for (int k = 0; k < 9; k++) b.information[6 * (k / 3) + k % 3] = information[k];
    vector_betweens.push_back(b);
  }
  void add_imu(const ImuTerm& t) {
    glim_amd_nav_imu_term c{};
    c.pose_i = t.pose_i, c.velocity_i = t.velocity_i, c.pose_j = t.pose_j, c.velocity_j = t.velocity_j, c.bias = t.bias;
    c.mode = t.mode;
    c.dt = t.dt;
    for (int k = 0; k < 3; k++) c.gravity[k] = t.gravity[k];
    for (int k = 0; k < 6; k++) c.bias_hat[k] = t.bias_hat[k];
    for (int k = 0; k < 9; k++) c.delta[k] = t.delta[k];
    for (int k = 0; k < 54; k++) c.H_bias[k] = t.H_bias[k];
    for (int k = 0; k < 81; k++) c.information[k] = t.information[k];
    imu_terms.push_back(c);
  }
};

struct NavGraphResult {
  std::vector<double> values;           // 12 per node: the last kept values
  std::vector<double> compact;          // 29 per factor
  std::vector<double> between_weights;  // one per pose between
  double cost = 0.0, factor_cost = 0.0, prior_cost = 0.0, between_cost = 0.0, vector_prior_cost = 0.0, vector_between_cost = 0.0, imu_cost = 0.0;
  std::int64_t num_inliers = 0;
  int iterations = 0, trials = 0;
  int status = 0;  // GLIM_AMD_ALIGN_*
  glim_amd_nav_result raw{};
  Isometry3d pose(int node) const {
    Isometry3d T;
    for (int u = 0; u < 12; u++) T.m[u] = values[12 * (std::size_t)node + u];
    return T;
  }
};

inline NavGraphResult optimize_nav_graph(const NavGraph& g, const LMParams& params = graph_params()) {
  NavGraphResult r;
  const std::size_t N = g.kinds.size(), F = g.graph.targets.size();
  if (N == 0) return r;  // answered before any device call
  r.values.resize(12 * N);
  r.compact.resize(GLIM_AMD_COMPACT_DOUBLES * F);
  r.between_weights.resize(g.graph.betweens.size());
  const glim_amd_lm_params p = params.c();
  const Context ctx = g.graph.ctx ? g.graph.ctx : StreamTempBufferRoundRobin::default_instance();
  glim_amd_graph_terms terms{};
  terms.dampings = g.graph.dampings.data();
  terms.num_dampings = (std::int32_t)g.graph.dampings.size();
  terms.between_huber_width = g.graph.between_huber_width.size() == g.graph.betweens.size() ? g.graph.between_huber_width.data() : nullptr;
  glim_amd_nav_terms nav{};
  nav.kinds = g.kinds.data();
  nav.vector_priors = g.vector_priors.data();
  nav.vector_betweens = g.vector_betweens.data();
  nav.imu_terms = g.imu_terms.data();
  nav.num_vector_priors = (std::int32_t)g.vector_priors.size();
  nav.num_vector_betweens = (std::int32_t)g.vector_betweens.size();
  nav.num_imu_terms = (std::int32_t)g.imu_terms.size();
  check(glim_amd_graph_align_nav(ctx->context(), g.graph.targets.data(), g.graph.sources.data(), g.graph.target_pose.data(), g.graph.source_pose.data(), (std::int32_t)F,
                                 g.graph.surface_validation ? GLIM_AMD_FACTOR_SURFACE_VALIDATION : 0u, g.graph.priors.data(), (std::int32_t)g.graph.priors.size(),
                                 g.graph.betweens.data(), (std::int32_t)g.graph.betweens.size(), g.values.data(), (std::int32_t)N, &p, r.values.data(),
                                 F ? r.compact.data() : nullptr, &r.raw, &terms, r.between_weights.empty() ? nullptr : r.between_weights.data(), &nav),
        "optimize_nav_graph");
  r.cost = r.raw.cost, r.factor_cost = r.raw.factor_cost, r.prior_cost = r.raw.prior_cost, r.between_cost = r.raw.between_cost;
  r.vector_prior_cost = r.raw.vector_prior_cost, r.vector_between_cost = r.raw.vector_between_cost, r.imu_cost = r.raw.imu_cost;
  r.num_inliers = r.raw.num_inliers;
  r.iterations = r.raw.iterations, r.trials = r.raw.trials, r.status = r.raw.status;
  return r;
}

}  // namespace glim_amd
