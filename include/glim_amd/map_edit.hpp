// map_edit.hpp -- header-only C++17 mirror, over the C ABI (glim_amd.h "Map editing"), of the data-parallel steps of GLIM's map editor
// (viewer/editor/points_selector.cpp).  Points are named by the reference's packed ids, (uint64(sub-map) << 32) | point (:84).
//
//   auto ids = glim_amd::select_gizmo(submaps, poses, model_matrix, /*sphere=*/false);          // select_points_tool, :623-674
//   auto ids = glim_amd::select_radius(submaps, poses, picked, 2.0);                            // select_points_radius, :677-700
//   auto ids = glim_amd::select_outliers(submaps, poses, picked, 2.0);                          // select_outlier_points_radius, :703-759
//   auto seg = glim_amd::region_growing(submaps, poses, picked, glim_amd::RegionGrowingParams());  // select_points_segmentation, :798-810
//   auto cut = glim_amd::select_min_cut(submaps, poses, picked, glim_amd::MinCutParams());       // select_points_segmentation, :774-797
//   auto upd = glim_amd::remove_selected(submaps, seg.ids);                                     // remove_selected_points, :513-562
//
// No gtsam_points drop-in exists for this tool: points_selector.cpp needs Iridescence.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "gtsam_points_compat.hpp"

namespace glim_amd {

using Affine12 = std::array<double, 12>;  // 3x4 row-major [A | a]

namespace edit_detail {
struct Args {
  std::vector<const glim_amd_cloud*> handles;
  std::vector<double> M12;
  std::int64_t total = 0;
};
inline Args args(const std::vector<PointCloudGPU::ConstPtr>& submaps, const std::vector<Isometry3d>& poses, const Affine12* left = nullptr) {
  if (submaps.size() != poses.size()) throw std::invalid_argument("one pose per sub-map");
  Args a;
  for (std::size_t s = 0; s < submaps.size(); s++) {
    a.handles.push_back(submaps[s]->handle());
    a.total += (std::int64_t)submaps[s]->size();
    Affine12 m = poses[s].m;
    if (left) {  // left * pose, both affine
      const Affine12& l = *left;
      const Affine12& p = poses[s].m;
      for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) m[4 * r + c] = l[4 * r] * p[c] + l[4 * r + 1] * p[4 + c] + l[4 * r + 2] * p[8 + c];
        m[4 * r + 3] = l[4 * r] * p[3] + l[4 * r + 1] * p[7] + l[4 * r + 2] * p[11] + l[4 * r + 3];
      }
    }
    a.M12.insert(a.M12.end(), m.begin(), m.end());
  }
  return a;
}
// inverse of an affine map (the gizmo's model matrix: rotation, scale and shear)
inline Affine12 inverse(const Affine12& m) {
  const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
  const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
  if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) throw std::invalid_argument("singular model matrix");
  const double A[9] = {(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det, (f * g - d * i) / det, (a * i - c * g) / det,
                       (c * d - a * f) / det, (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det};
  Affine12 o;
  for (int r = 0; r < 3; r++) {
    for (int k = 0; k < 3; k++) o[4 * r + k] = A[3 * r + k];
    o[4 * r + 3] = -(A[3 * r] * m[3] + A[3 * r + 1] * m[7] + A[3 * r + 2] * m[11]);
  }
  return o;
}
inline glim_amd_edit_window window(const std::array<double, 3>& center, double resolution, int cells) {
  glim_amd_edit_window w;
  for (int k = 0; k < 3; k++) w.center[k] = center[k];
  w.resolution = resolution;
  w.window = cells;
  w.reserved = 0;
  return w;
}
inline std::vector<std::uint64_t> pack(const std::vector<std::int32_t>& flat, std::size_t n) {
  std::vector<std::uint64_t> ids(n);
  for (std::size_t k = 0; k < n; k++) ids[k] = ((std::uint64_t)(std::uint32_t)flat[2 * k] << 32) | (std::uint64_t)(std::uint32_t)flat[2 * k + 1];
  return ids;
}
inline std::vector<std::uint64_t> run_select(const Args& a, int mode, const glim_amd_edit_window* w, double radius, const char* what) {
  std::vector<std::int32_t> flat(2 * (std::size_t)a.total + 2);
  std::int64_t count = 0;
  check(glim_amd_edit_select(a.handles.data(), (std::int32_t)a.handles.size(), a.M12.data(), mode, w, radius, a.total, flat.data(), &count), what);
  return pack(flat, (std::size_t)count);
}
}  // namespace edit_detail

// the unit box (or sphere) of the gizmo's model matrix, 3x4 row-major
inline std::vector<std::uint64_t> select_gizmo(const std::vector<PointCloudGPU::ConstPtr>& submaps, const std::vector<Isometry3d>& poses,
                                               const Affine12& model_matrix, bool sphere) {
  const Affine12 inv = edit_detail::inverse(model_matrix);
  const auto a = edit_detail::args(submaps, poses, &inv);
  return edit_detail::run_select(a, sphere ? GLIM_AMD_EDIT_SPHERE : GLIM_AMD_EDIT_BOX, nullptr, 0.0, "select_gizmo");
}

// collect_neighbor_point_ids (:85-112), as a set in ascending id order
inline std::vector<std::uint64_t> select_window(const std::vector<PointCloudGPU::ConstPtr>& submaps, const std::vector<Isometry3d>& poses,
                                                const std::array<double, 3>& point, double map_cell_resolution = 2.0, int cell_selection_window = 5) {
  const auto a = edit_detail::args(submaps, poses);
  const glim_amd_edit_window w = edit_detail::window(point, map_cell_resolution, cell_selection_window);
  return edit_detail::run_select(a, GLIM_AMD_EDIT_WINDOW, &w, 0.0, "select_window");
}

inline std::vector<std::uint64_t> select_radius(const std::vector<PointCloudGPU::ConstPtr>& submaps, const std::vector<Isometry3d>& poses,
                                                const std::array<double, 3>& picked_point, double select_radius, double map_cell_resolution = 2.0,
                                                int cell_selection_window = 5) {
  const auto a = edit_detail::args(submaps, poses);
  const glim_amd_edit_window w = edit_detail::window(picked_point, map_cell_resolution, cell_selection_window);
  return edit_detail::run_select(a, GLIM_AMD_EDIT_WINDOW_BALL, &w, select_radius, "select_radius");
}

// status (may be null): GLIM_AMD_EDIT_OK or GLIM_AMD_EDIT_FEW_POINTS
inline std::vector<std::uint64_t> select_outliers(const std::vector<PointCloudGPU::ConstPtr>& submaps, const std::vector<Isometry3d>& poses,
                                                  const std::array<double, 3>& picked_point, double select_radius, double outlier_radius_offset = 1.0,
                                                  int outlier_num_neighbors = 10, double outlier_stddev_thresh = 2.0, double map_cell_resolution = 2.0,
                                                  int cell_selection_window = 5, std::int32_t* status = nullptr) {
  const auto a = edit_detail::args(submaps, poses);
  const glim_amd_edit_window w = edit_detail::window(picked_point, map_cell_resolution, cell_selection_window);
  const glim_amd_edit_outlier_params prm = {outlier_radius_offset, outlier_stddev_thresh, outlier_num_neighbors, 0};
  std::vector<std::int32_t> flat(2 * (std::size_t)a.total + 2);
  std::int64_t count = 0;
  check(glim_amd_edit_select_outliers(a.handles.data(), (std::int32_t)a.handles.size(), a.M12.data(), &w, select_radius, &prm, a.total, flat.data(), &count,
                                      status),
        "select_outliers");
  return edit_detail::pack(flat, (std::size_t)count);
}

// The three thresholds' defaults are a recollection of gtsam_points::RegionGrowingParams, which is not in the reference tree.
struct RegionGrowingParams {
  double distance_threshold = 0.5;
  double angle_threshold = 10.0 * 3.14159265358979323846 / 180.0;  // radians; its cosine is taken once, on the host
  double dilation_radius = 0.5;                                    // 0: no dilation
  bool use_normals = false;
  int max_hops = 0;  // 0: unlimited
};
struct RegionGrowingResult {
  std::vector<std::uint64_t> ids;    // the cluster, ascending
  std::vector<std::int32_t> levels;  // hops from the seed, per id
  glim_amd_edit_region_result info;
};
inline RegionGrowingResult region_growing(const std::vector<PointCloudGPU::ConstPtr>& submaps, const std::vector<Isometry3d>& poses,
                                          const std::array<double, 3>& picked_point, const RegionGrowingParams& params = RegionGrowingParams(),
                                          double map_cell_resolution = 2.0, int cell_selection_window = 5) {
  const auto a = edit_detail::args(submaps, poses);
  const glim_amd_edit_window w = edit_detail::window(picked_point, map_cell_resolution, cell_selection_window);
  const glim_amd_edit_region_growing_params prm = {params.distance_threshold, std::cos(params.angle_threshold), params.dilation_radius,
                                                   params.use_normals ? 1 : 0, params.max_hops};
  std::vector<std::int32_t> flat(2 * (std::size_t)a.total + 2);
  RegionGrowingResult r;
  r.levels.resize((std::size_t)a.total + 1);
  check(glim_amd_edit_region_grow(a.handles.data(), (std::int32_t)a.handles.size(), a.M12.data(), &w, &prm, a.total, flat.data(), r.levels.data(), &r.info),
        "region_growing");
  r.ids = edit_detail::pack(flat, (std::size_t)r.info.count);
  r.levels.resize((std::size_t)r.info.count);
  return r;
}

// The sigmas and k are a recollection of gtsam_points::MinCutParams, which is not in the reference tree; the radii and the weight are the
// editor's (:42-44).  The semantics (glim_amd.h "Map editing", min-cut) are this project's: the minimal source side of a minimum cut.
struct MinCutParams {
  double distance_sigma = 0.25;
  double angle_sigma = 10.0 * 3.14159265358979323846 / 180.0;  // radians, as the reference's params; used only with use_normals
  double foreground_mask_radius = 0.5;
  double background_mask_radius = 5.0;
  double foreground_weight = 10.0;
  double background_weight = 0.0;  // 0: the foreground weight
  int k_neighbors = 20;            // <= 31
  bool use_normals = false;
  int max_rounds = 0;  // 0: GLIM_AMD_EDIT_MIN_CUT_MAX_ROUNDS
};
struct MinCutResult {
  std::vector<std::uint64_t> ids;  // the segment, ascending
  glim_amd_edit_min_cut_result info;
};
inline MinCutResult select_min_cut(const std::vector<PointCloudGPU::ConstPtr>& submaps, const std::vector<Isometry3d>& poses,
                                   const std::array<double, 3>& picked_point, const MinCutParams& params = MinCutParams(),
                                   double map_cell_resolution = 2.0, int cell_selection_window = 5) {
  const auto a = edit_detail::args(submaps, poses);
  const glim_amd_edit_window w = edit_detail::window(picked_point, map_cell_resolution, cell_selection_window);
  const glim_amd_edit_min_cut_params prm = {params.distance_sigma,    params.angle_sigma,       params.foreground_mask_radius, params.background_mask_radius,
                                            params.foreground_weight, params.background_weight, params.k_neighbors,            params.use_normals ? 1 : 0,
                                            params.max_rounds,        0};
  std::vector<std::int32_t> flat(2 * (std::size_t)a.total + 2);
  MinCutResult r;
  check(glim_amd_edit_min_cut(a.handles.data(), (std::int32_t)a.handles.size(), a.M12.data(), &w, &prm, a.total, flat.data(), &r.info), "select_min_cut");
  r.ids = edit_detail::pack(flat, (std::size_t)r.info.count);
  return r;
}

// a new cloud without the listed points; the input cloud is untouched
inline PointCloudGPU::Ptr remove_points(const PointCloudGPU::ConstPtr& cloud, const std::vector<std::int32_t>& indices) {
  if (!cloud) throw std::invalid_argument("null cloud");
  glim_amd_cloud* h = nullptr;
  check(glim_amd_edit_remove_points(cloud->handle(), (std::int64_t)indices.size(), indices.empty() ? nullptr : indices.data(), &h), "remove_points");
  return PointCloudGPU::adopt(h, cloud->context());
}

// remove_selected_points (:513-562): the ids are sorted and partitioned by sub-map; -> (sub-map index, its new cloud) for the sub-maps touched
inline std::vector<std::pair<int, PointCloudGPU::Ptr>> remove_selected(const std::vector<PointCloudGPU::ConstPtr>& submaps, std::vector<std::uint64_t> ids) {
  std::sort(ids.begin(), ids.end());
  std::vector<std::pair<int, PointCloudGPU::Ptr>> out;
  std::size_t k = 0;
  while (k < ids.size()) {
    const std::uint64_t s = ids[k] >> 32;
    if (s >= submaps.size()) throw std::invalid_argument("sub-map index out of range");
    std::vector<std::int32_t> idx;
    for (; k < ids.size() && (ids[k] >> 32) == s; k++) idx.push_back((std::int32_t)(ids[k] & 0xffffffffull));
    out.emplace_back((int)s, remove_points(submaps[(std::size_t)s], idx));
  }
  return out;
}

}  // namespace glim_amd
