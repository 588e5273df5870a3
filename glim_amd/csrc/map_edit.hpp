// map_edit.hpp -- the map editor's point predicates (src/glim/viewer/editor/points_selector.cpp) and its packed point ids, in one place for
// the kernels of map_edit.hip and for a stand-alone host program (tests/cpp/test_map_edit_host.cpp, plain and under the address /
// undefined-behaviour sanitizers).  Plain C++ as well as HIP.  Every product and sum is rounded on its own: no FMA contraction, and the
// operation order is the one include/glim_amd.h "Map editing" states, so that a NumPy restatement reproduces every boolean.
// Also the edge weights and integer capacities of the min-cut segmentation (tests/cpp/test_min_cut_host.cpp runs them the same way).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define GLIM_AMD_EDIT_HD __host__ __device__
#else
#define GLIM_AMD_EDIT_HD
#endif

namespace glim_amd {
namespace edit {

enum { MODE_BOX = 0, MODE_SPHERE = 1, MODE_WINDOW = 2, MODE_WINDOW_BALL = 3 };

// the reference's point id (points_selector.cpp:84): (sub-map << 32) | point
GLIM_AMD_EDIT_HD inline uint64_t pack_id(int32_t submap, int32_t point) { return ((uint64_t)(uint32_t)submap << 32) | (uint64_t)(uint32_t)point; }
GLIM_AMD_EDIT_HD inline int32_t id_submap(uint64_t id) { return (int32_t)(id >> 32); }
GLIM_AMD_EDIT_HD inline int32_t id_point(uint64_t id) { return (int32_t)(id & 0xffffffffull); }

// what a predicate needs besides the point: the window's cell bounds (inclusive, as doubles: a cell coordinate is compared, never cast),
// 1 / resolution, the centre and the squared radius
struct Predicate {
  int mode;
  int pad;
  double lo[3], hi[3];
  double inv_resolution;
  double center[3];
  double r2;
};

// collect_neighbor_point_ids (:85-112): the window's centre cell is floor(c_k / resolution) -- a division, :87 -- and the window reaches
// `window` cells to either side
GLIM_AMD_EDIT_HD inline void window_bounds(const double* center, double resolution, int window, Predicate* p) {
#pragma clang fp contract(off)
  p->inv_resolution = 1.0 / resolution;
  for (int k = 0; k < 3; k++) {
    const double c = floor(center[k] / resolution);
    p->lo[k] = c - (double)window;
    p->hi[k] = c + (double)window;
    p->center[k] = center[k];
  }
}

// out_k = ((T[4k] x + T[4k+1] y) + T[4k+2] z) + T[4k+3]
GLIM_AMD_EDIT_HD inline void transform(const double* T, double x, double y, double z, double* out) {
#pragma clang fp contract(off)
  for (int k = 0; k < 3; k++) out[k] = ((T[4 * k] * x + T[4 * k + 1] * y) + T[4 * k + 2] * z) + T[4 * k + 3];
}
// the rotation alone (normals)
GLIM_AMD_EDIT_HD inline void rotate(const double* T, double x, double y, double z, double* out) {
#pragma clang fp contract(off)
  for (int k = 0; k < 3; k++) out[k] = (T[4 * k] * x + T[4 * k + 1] * y) + T[4 * k + 2] * z;
}

GLIM_AMD_EDIT_HD inline double sq3(double x, double y, double z) {
#pragma clang fp contract(off)
  return (x * x + y * y) + z * z;
}

// squared distance of w to the predicate's centre: e = w - c first, then the squares
GLIM_AMD_EDIT_HD inline double center_qq(const Predicate& p, const double* w) {
#pragma clang fp contract(off)
  return sq3(w[0] - p.center[0], w[1] - p.center[1], w[2] - p.center[2]);
}

// the cell of update_cells (:177 / :593) is floor(w_k * inv_resolution) -- a product
GLIM_AMD_EDIT_HD inline bool in_window(const Predicate& p, const double* w) {
#pragma clang fp contract(off)
  for (int k = 0; k < 3; k++) {
    const double cell = floor(w[k] * p.inv_resolution);
    if (!(cell >= p.lo[k] && cell <= p.hi[k])) return false;
  }
  return true;
}

// v: the transformed point -- gizmo-local for BOX / SPHERE (:644), world otherwise
GLIM_AMD_EDIT_HD inline bool selected(const Predicate& p, const double* v) {
  switch (p.mode) {
    case MODE_BOX: return v[0] > -0.5 && v[0] < 0.5 && v[1] > -0.5 && v[1] < 0.5 && v[2] > -0.5 && v[2] < 0.5;  // :648
    case MODE_SPHERE: return sq3(v[0], v[1], v[2]) < 1.0;                                                        // :654
    case MODE_WINDOW: return in_window(p, v);
    default: return in_window(p, v) && center_qq(p, v) < p.r2;  // :690-691
  }
}

// edge of the region-growing graph: strict in the distance; with normals, |n_i . n_j| >= cos_angle (estimated normals carry no sign)
GLIM_AMD_EDIT_HD inline bool edge(const double* a, const double* b, double thr2, const double* na, const double* nb, double cos_angle) {
#pragma clang fp contract(off)
  if (!(sq3(a[0] - b[0], a[1] - b[1], a[2] - b[2]) < thr2)) return false;
  if (!na) return true;
  return fabs((na[0] * nb[0] + na[1] * nb[1]) + na[2] * nb[2]) >= cos_angle;
}

// ---- min-cut segmentation: edge weights and their integer capacities (include/glim_amd.h "Map editing", min-cut) ----
constexpr double CAP_SCALE = 65536.0;  // GLIM_AMD_EDIT_CAP_SCALE

// exp(-(dd / (sigma sigma))), dd = (dx dx + dy dy) + dz dz, the denominator rounded once
GLIM_AMD_EDIT_HD inline double min_cut_distance_weight(const double* a, const double* b, double sigma) {
#pragma clang fp contract(off)
  const double dd = sq3(a[0] - b[0], a[1] - b[1], a[2] - b[2]);
  const double ss = sigma * sigma;
  return exp(-(dd / ss));
}
// exp(-((t t) / (sigma sigma))), t = acos(min(1, |n_i . n_j|)) (estimated normals carry no sign)
GLIM_AMD_EDIT_HD inline double min_cut_normal_weight(const double* na, const double* nb, double sigma) {
#pragma clang fp contract(off)
  const double d = fabs((na[0] * nb[0] + na[1] * nb[1]) + na[2] * nb[2]);
  const double t = acos(fmin(1.0, d));
  const double tt = t * t;
  const double ss = sigma * sigma;
  return exp(-(tt / ss));
}
// floor(w * 65536 + 0.5) as a double: what quantize_capacity casts, and what the parameter check compares with 2^31
GLIM_AMD_EDIT_HD inline double scaled_weight(double w) {
#pragma clang fp contract(off)
  return floor(w * CAP_SCALE + 0.5);
}
GLIM_AMD_EDIT_HD inline bool capacity_fits(double w) { return scaled_weight(w) >= 0.0 && scaled_weight(w) < 2147483648.0; }
GLIM_AMD_EDIT_HD inline int32_t quantize_capacity(double w) { return (int32_t)scaled_weight(w); }
GLIM_AMD_EDIT_HD inline int32_t min_cut_edge_capacity(const double* a, const double* b, double sigma_d, const double* na, const double* nb, double sigma_a) {
#pragma clang fp contract(off)
  double w = min_cut_distance_weight(a, b, sigma_d);
  if (na) w = w * min_cut_normal_weight(na, nb, sigma_a);
  return quantize_capacity(w);
}

}  // namespace edit
}  // namespace glim_amd
