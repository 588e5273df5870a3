// The C++ mirror of the min-cut entry point (include/glim_amd/map_edit.hpp, select_min_cut) compiles as C++17, links against the library and
// turns a refused call into an exception.  No device is needed: every call below is refused before the library touches one.
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
  int failed = 0;
  // one pose, no sub-map: refused by the mirror
  failed += !throws([&] { select_min_cut(none, {Isometry3d::Identity()}, c); });
  // radii in the wrong order: refused by the library (or, without a device, by its first check)
  MinCutParams bad;
  bad.foreground_mask_radius = 6.0;
  failed += !throws([&] { select_min_cut(none, no_poses, c, bad); });
  // the defaults: the editor's radii and weight, the angle in radians
  const MinCutParams p;
  failed += !(p.foreground_mask_radius == 0.5 && p.background_mask_radius == 5.0 && p.foreground_weight == 10.0 && p.k_neighbors == 20 && !p.use_normals);
  failed += !(p.angle_sigma > 0.1745 && p.angle_sigma < 0.1746 && p.distance_sigma == 0.25 && p.max_rounds == 0);
  failed += !(GLIM_AMD_EDIT_NO_SEED == 3 && GLIM_AMD_EDIT_ROUND_LIMIT == 4 && GLIM_AMD_EDIT_CAP_SCALE == 65536);
  failed += !(sizeof(glim_amd_edit_min_cut_params) == 64 && sizeof(glim_amd_edit_min_cut_result) == 64);
  std::printf("min_cut mirror: %s\n", failed ? "FAILED" : "ok");
  return failed;
}
