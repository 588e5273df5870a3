// The C++ mirror of the resampling entry points (include/glim_amd/resample.hpp) compiles as C++17, links against the library and turns a
// refused call into an exception.  No device is needed: every call below is refused before the library touches one.
#include <cstdio>
#include <random>
#include <stdexcept>

#include <glim_amd/resample.hpp>

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
  int failed = 0;
  std::mt19937 mt(7);
  // a null cloud: refused by the mirror
  failed += !throws([&] { random_sampling(nullptr, 0.5, 1); });
  failed += !throws([&] { random_sampling(nullptr, 0.5, mt); });
  failed += !throws([&] { sample(nullptr, {0, 1}); });
  failed += !throws([&] { transform(nullptr, Isometry3d::Identity()); });
  // ... and by the library, with the code the header states
  glim_amd_cloud* h = nullptr;
  const double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  failed += glim_amd_cloud_random_sample(nullptr, 0.5, 1, &h) != GLIM_AMD_ERR_INVALID;
  failed += glim_amd_cloud_sample(nullptr, 0, nullptr, &h) != GLIM_AMD_ERR_INVALID;
  failed += glim_amd_cloud_transform(nullptr, T, &h) != GLIM_AMD_ERR_INVALID;
  failed += h != nullptr;
  // the generator overload takes one 64-bit seed as two draws, the first one the upper half, and leaves the generator two draws on
  std::mt19937 a(7), b(7);
  const std::uint64_t hi = a(), lo = a();
  failed += draw_seed(b) != ((hi << 32) | lo);
  failed += a() != b();
  std::printf("resample mirror: %s\n", failed ? "FAILED" : "ok");
  return failed;
}
