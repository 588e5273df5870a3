// The C++ mirror of the map-editing entry points (include/glim_amd/map_edit.hpp) compiles as C++17, links against the library and turns a
// refused call into an exception.  No device is needed: every call below is refused before the library touches one.
#include <cstdio>
#include <stdexcept>

#include <glim_amd/map_edit.hpp>

template <class F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const std::runtime_error&) {
    return true;
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

int main() {
  using namespace glim_amd;
  const std::array<double, 3> c{{0.0, 0.0, 0.0}};
  const std::vector<PointCloudGPU::ConstPtr> none;
  const std::vector<Isometry3d> no_poses;
  const Affine12 model{{2, 0, 0, 1, 0, 4, 0, 2, 0, 0, 8, 3}};
  int failed = 0;
  // one pose, no sub-map: refused by the mirror; a singular model matrix likewise; a null cloud likewise
  failed += !throws([&] { select_window(none, {Isometry3d::Identity()}, c); });
  failed += !throws([&] { select_radius(none, {Isometry3d::Identity()}, c, 2.0); });
  failed += !throws([&] { select_outliers(none, {Isometry3d::Identity()}, c, 2.0); });
  failed += !throws([&] { region_growing(none, {Isometry3d::Identity()}, c); });
  failed += !throws([&] { select_gizmo(none, no_poses, Affine12{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0}}, false); });
  failed += !throws([&] { remove_points(nullptr, {}); });
  failed += !throws([&] { remove_selected(none, {1ull << 32}); });
  // a resolution of zero: refused by the library (or, without a device, by its first check)
  failed += !throws([&] { select_window(none, no_poses, c, 0.0); });
  // the inverse of a scaling: A^-1 = diag(1/2, 1/4, 1/8), a' = -A^-1 a
  const Affine12 inv = edit_detail::inverse(model);
  failed += !(inv[0] == 0.5 && inv[5] == 0.25 && inv[10] == 0.125 && inv[3] == -0.5 && inv[7] == -0.5 && inv[11] == -0.375 && inv[1] == 0.0);
  const auto ids = edit_detail::pack({3, 7, 0, 1}, 2);
  failed += !(ids[0] == ((3ull << 32) | 7ull) && ids[1] == 1ull);
  std::printf("map_edit mirror: %s\n", failed ? "FAILED" : "ok");
  return failed;
}
