// The host-callable rules of glim_amd/csrc/resample.hpp -- the key a point is drawn by, the number of points a rate keeps, and the transform
// of a point, a covariance and a normal -- run from a stand-alone program.  tests/test_resample.py builds it plain and under the address /
// undefined-behaviour sanitizers and compares every output with the NumPy restatement for equality.
//
//   input : seed num_keys
//           num_counts, then num_counts lines "n rate"
//           the 12 entries of T
//           num_points, then num_points lines of 4 point + 6 covariance + 3 normal doubles
//           (every double as a hexadecimal floating constant)
//   output: one line of keys; one line of counts; per point one line of the bit patterns of 4 + 6 + 3 transformed doubles
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../glim_amd/csrc/resample.hpp"

static uint64_t bits(double v) {
  uint64_t u;
  std::memcpy(&u, &v, sizeof(u));
  return u;
}

int main(int argc, char** argv) {
  using namespace glim_amd::resample;
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "r");
  FILE* out = std::fopen(argv[2], "w");
  if (!in || !out) return 2;
  uint64_t seed = 0;
  long long num_keys = 0, num_counts = 0, num_points = 0;
  if (std::fscanf(in, "%" SCNu64 " %lld", &seed, &num_keys) != 2) return 3;
  for (long long i = 0; i < num_keys; i++) std::fprintf(out, "%u ", (unsigned)sample_key(seed, (uint64_t)i));
  std::fprintf(out, "\n");
  if (std::fscanf(in, "%lld", &num_counts) != 1) return 3;
  for (long long i = 0; i < num_counts; i++) {
    long long n = 0;
    double rate = 0.0;
    if (std::fscanf(in, "%lld %la", &n, &rate) != 2) return 3;
    std::fprintf(out, "%lld ", (long long)sample_count((int64_t)n, rate));
  }
  std::fprintf(out, "\n");
  double T[12];
  for (int k = 0; k < 12; k++)
    if (std::fscanf(in, "%la", &T[k]) != 1) return 3;
  if (std::fscanf(in, "%lld", &num_points) != 1) return 3;
  std::vector<double> row(13);
  for (long long i = 0; i < num_points; i++) {
    for (int k = 0; k < 13; k++)
      if (std::fscanf(in, "%la", &row[(size_t)k]) != 1) return 3;
    double q[4], d[6], m[3];
    transform_point(T, row.data(), q);
    transform_cov(T, row.data() + 4, d);
    transform_normal(T, row.data() + 10, m);
    for (int k = 0; k < 4; k++) std::fprintf(out, "%" PRIu64 " ", bits(q[k]));
    for (int k = 0; k < 6; k++) std::fprintf(out, "%" PRIu64 " ", bits(d[k]));
    for (int k = 0; k < 3; k++) std::fprintf(out, "%" PRIu64 " ", bits(m[k]));
    std::fprintf(out, "\n");
  }
  std::fclose(in);
  std::fclose(out);
  return 0;
}
