// The C++ mirror of the plane bundle-adjustment entry points (include/glim_amd/plane_ba.hpp) compiles as C++17, links against the library and
// turns a refused call into an exception.  No device is needed: every call below is refused before the library touches one.
#include <cstdio>
#include <stdexcept>

#include <glim_amd/plane_ba.hpp>

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
  failed += !throws([&] { extract_ball(none, no_poses, c, 1.0); });
  failed += !throws([&] { ball_eigenvalues(none, no_poses, c, 1.0); });
  failed += !throws([&] { auto_radius(none, no_poses, c, 1.0); });
  failed += !throws([&] { PlaneEVMFactorHIP::from_ball(none, no_poses, c, 1.0); });
  failed += !throws([&] { extract_ball(none, {Isometry3d::Identity()}, c, 1.0); });
  // the member functions are instantiated without being called
  auto lin = &PlaneEVMFactorHIP::linearize;
  auto err = &EdgeEVMFactorHIP::error;
  auto pts = &EdgeEVMFactorHIP::from_points;
  auto fr = &PlaneEVMFactorHIP::frames;
  auto mo = &PlaneEVMFactorHIP::moments;
  glim_amd_ba_params prm;
  failed += glim_amd_ba_default_params(&prm) != GLIM_AMD_OK || prm.max_radius != 5.0;
  std::printf("plane_ba mirror: %s (%d)\n", failed ? "FAILED" : "ok", (int)(lin && err && pts && fr && mo));
  return failed;
}
