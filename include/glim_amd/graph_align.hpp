// graph_align.hpp -- header-only C++17 mirror, over the C ABI (glim_amd.h "Global-graph optimisation"), of one batch optimisation over the
// poses of GLIM's global graph: Levenberg-Marquardt over the sub-map poses on the pairwise binary VGICP factors between sub-maps
// (global_mapping.cpp:430-484) and that file's pose-only relative-pose factors -- graph in, poses out, one call.  The graph, the result and the
// parameters are bundle_align.hpp's; the caps are GLIM_AMD_GRAPH_MAX_*.  Within the bundle's caps the result is optimize_bundle's, bit for bit.
// BundleGraph::add_damping (LinearDampingFactor) and add_between's Huber width send the graph through glim_amd_graph_align_terms.
// Out of scope: ISAM2, IMU variables, pose marginals, robust priors, M-estimators other than Huber, several devices, translating a
// gtsam::NonlinearFactorGraph.
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

}  // namespace glim_amd
