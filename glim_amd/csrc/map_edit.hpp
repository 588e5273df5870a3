// map_edit.hpp -- the map editor's point predicates (src/glim/viewer/editor/points_selector.cpp) and its packed point ids, in one place for
// the kernels of map_edit.hip and for a stand-alone host program (tests/cpp/test_map_edit_host.cpp, plain and under the address /
// undefined-behaviour sanitizers).  Plain C++ as well as HIP.  Every product and sum is rounded on its own: no FMA contraction, and the
// operation order is the one include/glim_amd.h "Map editing" states, so that a NumPy restatement reproduces every boolean.
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

}  // namespace edit
}  // namespace glim_amd
