// bundle_align.hpp -- header-only C++17 mirror, over the C ABI (glim_amd.h "Sub-map bundle optimisation"), of the optimisation GLIM runs when a
// sub-map is closed (sub_mapping.cpp:430-452): Levenberg-Marquardt over the keyframe poses on the all-pairs binary VGICP factors, the prior on
// the first keyframe (:186) and the relative-pose factors (:210/:212) -- graph in, poses out, one call and one host synchronisation.  LMParams
// is gicp_align.hpp's.  Damping terms (gtsam_points::LinearDampingFactor) and Huber widths on between terms (noiseModel::Robust(Huber)) are
// add_damping and add_between's last argument; a graph that holds one goes through glim_amd_bundle_align_terms.  Out of scope: IMU terms in
// this LDS bundle (velocity and bias nodes are graph_align.hpp's NavGraph), ISAM2, pose marginals, CombinedImuFactor, robust priors, other M-estimators, translating a gtsam::NonlinearFactorGraph.
//
//   glim_amd::BundleGraph g;
//   g.add_factor(*voxels[i], *frames[j], i, j);                       // IntegratedVGICPFactorGPU(X(i), X(j), voxels[i], frames[j])
//   g.add_prior(0, T0, information);                                  // PriorFactor<Pose3>(X(0), T0, Precision(6, 1e6))
//   g.add_between(i, i + 1, delta, information);                      // BetweenFactor<Pose3>(X(i), X(i + 1), delta, ...)
//   g.add_between(i, j, loop, information, 1.0);                      // ... with Robust(Huber(1.0), ...)
//   g.add_damping(0, 1e6);                                            // LinearDampingFactor(X(0), 6, 1e6)
//   auto r = glim_amd::optimize_bundle(g, initial_poses);             // r.poses[k], r.cost, r.status
#pragma once

#include <array>
#include <cstdint>
#include <vector>

#include "gicp_align.hpp"

namespace glim_amd {

inline LMParams bundle_params() {  // glim_amd_bundle_align_default_params
  LMParams p;
  p.max_iterations = 20;
  return p;
}

struct BundleGraph {
  std::vector<const glim_amd_voxelmap*> targets;
  std::vector<const glim_amd_cloud*> sources;
  std::vector<std::int32_t> target_pose, source_pose;
  std::vector<glim_amd_bundle_prior> priors;
  std::vector<glim_amd_bundle_between> betweens;
  std::vector<double> between_huber_width;  // one per between; 0 = Gaussian
  std::vector<glim_amd_graph_damping> dampings;
  Context ctx;  // of the first factor, or the default instance
  bool surface_validation = false;

  void add_factor(const GaussianVoxelMapGPU& target, const PointCloudGPU& source, int target_index, int source_index) {
    if (!ctx) ctx = source.context();
    targets.push_back(target.handle());
    sources.push_back(source.handle());
    target_pose.push_back(target_index);
    source_pose.push_back(source_index);
  }
  // information: row-major 6 x 6 in (omega, v) order
  void add_prior(int index, const Isometry3d& P, const std::array<double, 36>& information) {
    glim_amd_bundle_prior p{};
    p.pose = index;
    for (int k = 0; k < 12; k++) p.T[k] = P.m[k];
    for (int k = 0; k < 36; k++) p.information[k] = information[k];
    priors.push_back(p);
  }
  void add_between(int i, int j, const Isometry3d& D, const std::array<double, 36>& information, double huber_width = 0.0) {
    glim_amd_bundle_between b{};
    b.pose_i = i;
    b.pose_j = j;
    for (int k = 0; k < 12; k++) b.T[k] = D.m[k];
    for (int k = 0; k < 36; k++) b.information[k] = information[k];
    betweens.push_back(b);
    between_huber_width.push_back(huber_width);
  }
  // gtsam_points::LinearDampingFactor(X(index), 6, scale), and its per-axis form ((omega, v) order)
  void add_damping(int index, double scale) { add_damping(index, std::array<double, 6>{scale, scale, scale, scale, scale, scale}); }
  void add_damping(int index, const std::array<double, 6>& diagonal) {
    glim_amd_graph_damping d{};
    d.pose = index;
    for (int k = 0; k < 6; k++) d.diagonal[k] = diagonal[k];
    dampings.push_back(d);
  }
  bool has_terms() const {  // a damping, or a width that is not 0: the graph goes through the `_terms` entry point
    for (double w : between_huber_width)
      if (w != 0.0) return true;
    return !dampings.empty();
  }
  static std::array<double, 36> isotropic(double precision) {  // gtsam::noiseModel::Isotropic::Precision(6, precision)
    std::array<double, 36> m{};
    for (int k = 0; k < 6; k++) m[7 * k] = precision;
    return m;
  }
};

struct BundleResult {
  std::vector<Isometry3d> poses;        // the last kept poses
  std::vector<double> compact;          // 29 per factor: the records there (glim_amd_expand_compact gives the blocks)
  std::vector<double> between_weights;  // the Huber weights at the poses, one per between; empty from a graph without damping and widths
  double cost = 0.0, factor_cost = 0.0, prior_cost = 0.0, between_cost = 0.0;
  std::int64_t num_inliers = 0;
  int iterations = 0, trials = 0;
  int status = 0;  // GLIM_AMD_ALIGN_*
  glim_amd_bundle_result raw{};
};

namespace detail {
// entry: glim_amd_bundle_align, or an entry point with its arguments (graph_align.hpp); terms_entry: its `_terms` form
template <class Entry, class TermsEntry>
inline BundleResult optimize_poses(Entry entry, TermsEntry terms_entry, const char* what, const BundleGraph& g, const std::vector<Isometry3d>& initial,
                                   const LMParams& params) {
  BundleResult r;
  const std::size_t N = initial.size(), F = g.targets.size();
  if (N == 0) return r;  // answered before any device call
  std::vector<double> X(12 * N), out(12 * N);
  for (std::size_t k = 0; k < N; k++)
    for (int u = 0; u < 12; u++) X[12 * k + u] = initial[k].m[u];
  r.compact.resize(GLIM_AMD_COMPACT_DOUBLES * F);
  const glim_amd_lm_params p = params.c();
  const Context ctx = g.ctx ? g.ctx : StreamTempBufferRoundRobin::default_instance();
  const auto call = [&](auto fn, auto... more) {
    return fn(ctx->context(), g.targets.data(), g.sources.data(), g.target_pose.data(), g.source_pose.data(), (std::int32_t)F,
              g.surface_validation ? GLIM_AMD_FACTOR_SURFACE_VALIDATION : 0u, g.priors.data(), (std::int32_t)g.priors.size(), g.betweens.data(),
              (std::int32_t)g.betweens.size(), X.data(), (std::int32_t)N, &p, out.data(), F ? r.compact.data() : nullptr, &r.raw, more...);
  };
  if (g.has_terms()) {
    glim_amd_graph_terms terms{};
    terms.dampings = g.dampings.data();
    terms.num_dampings = (std::int32_t)g.dampings.size();
    terms.between_huber_width = g.between_huber_width.size() == g.betweens.size() ? g.between_huber_width.data() : nullptr;
    r.between_weights.resize(g.betweens.size());
    check(call(terms_entry, (const glim_amd_graph_terms*)&terms, r.between_weights.data()), what);
  } else {
    check(call(entry), what);
  }
  r.poses.resize(N);
  for (std::size_t k = 0; k < N; k++)
    for (int u = 0; u < 12; u++) r.poses[k].m[u] = out[12 * k + u];
  r.cost = r.raw.cost;
  r.factor_cost = r.raw.factor_cost;
  r.prior_cost = r.raw.prior_cost;
  r.between_cost = r.raw.between_cost;
  r.num_inliers = r.raw.num_inliers;
  r.iterations = r.raw.iterations;
  r.trials = r.raw.trials;
  r.status = r.raw.status;
  return r;
}
}  // namespace detail

inline BundleResult optimize_bundle(const BundleGraph& g, const std::vector<Isometry3d>& initial, const LMParams& params = bundle_params()) {
  return detail::optimize_poses([](auto... a) { return glim_amd_bundle_align(a...); }, [](auto... a) { return glim_amd_bundle_align_terms(a...); },
                                "optimize_bundle", g, initial, params);
}

}  // namespace glim_amd
