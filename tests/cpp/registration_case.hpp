// The known-answer case that the Python GPU tests dump for test_ransac.cpp and test_gnc.cpp (tests/registration_cases.py, write_drop_in_case):
//   int32 n_target, int32 n_source, int32 dof, uint64 seed, n_target x 4 doubles, n_source x 4 doubles (points),
//   n_target x 33 doubles, n_source x 33 doubles (descriptors), 12 doubles expected T_target_source, double inlier_rate
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include <gtsam_points/features/fpfh_estimation.hpp>

#define REQUIRE(c)                                                \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s (%s:%d)\n", #c, __FILE__, __LINE__); \
      return 1;                                                   \
    }                                                             \
  } while (0)

template <class T>
static bool read_n(std::FILE* f, T* p, std::size_t n) {
  return std::fread(p, sizeof(T), n, f) == n;
}

struct Case {
  std::int32_t nt = 0, ns = 0, dof = 0;
  std::uint64_t seed = 0;
  std::vector<Eigen::Vector4d> tp, sp;
  std::vector<gtsam_points::FPFHSignature> tf, sf;
  double T[12] = {}, rate = 0.0;

  // 0 when the whole file was read
  int load(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    REQUIRE(f != nullptr);
    const int rc = read(f);
    std::fclose(f);
    return rc;
  }

 private:
  int read(std::FILE* f) {
    REQUIRE(read_n(f, &nt, 1) && read_n(f, &ns, 1) && read_n(f, &dof, 1) && read_n(f, &seed, 1) && nt > 0 && ns > 0);
    tp.resize((std::size_t)nt), sp.resize((std::size_t)ns), tf.resize((std::size_t)nt), sf.resize((std::size_t)ns);
    REQUIRE(read_n(f, tp[0].data(), (std::size_t)nt * 4) && read_n(f, sp[0].data(), (std::size_t)ns * 4));
    for (auto& d : tf) REQUIRE(read_n(f, d.data(), 33));
    for (auto& d : sf) REQUIRE(read_n(f, d.data(), 33));
    REQUIRE(read_n(f, T, 12) && read_n(f, &rate, 1));
    return 0;
  }
};
