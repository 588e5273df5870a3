// resample.hpp -- the rules of the cloud resampling (include/glim_amd.h "Resampling a resident cloud") in one place, for the kernels of
// resample.hip and for a stand-alone host program (tests/cpp/test_resample_host.cpp, plain and under the address / undefined-behaviour
// sanitizers): the key a point is drawn by, the number of points a rate keeps, and the transform of a point, a covariance and a normal.
// Plain C++ as well as HIP.  Every product and sum is rounded on its own: no FMA contraction, and the operation order is the one
// oracle/preprocess_oracle.c states for the sub-map merge (:301-308), so that a NumPy restatement reproduces every bit.
#pragma once

#include <math.h>
#include <stdint.h>

#include "sample_hash.hpp"

#if defined(__HIP__)
#define GLIM_AMD_RESAMPLE_HD __host__ __device__
#else
#define GLIM_AMD_RESAMPLE_HD
#endif

namespace glim_amd {
namespace resample {

constexpr double FULL_RATE = 0.99;  // a rate from here on keeps the whole cloud

// the key point i is drawn by: the upper half of the generator's word, the rule of the merge's draw (oracle/preprocess_oracle.c:282-285)
GLIM_AMD_RESAMPLE_HD inline uint32_t sample_key(uint64_t seed, uint64_t i) { return (uint32_t)(sample_hash(seed, i) >> 32); }

// points a finite rate >= 0 keeps of n: the truncation of `frame->size() * sampling_rate`
GLIM_AMD_RESAMPLE_HD inline int64_t sample_count(int64_t n, double rate) {
#pragma clang fp contract(off)
  if (rate >= FULL_RATE) return n;
  return (int64_t)((double)n * rate);
}

// out_r = ((T[4r] p0 + T[4r+1] p1) + T[4r+2] p2) + T[4r+3] p3, out_3 = p3
GLIM_AMD_RESAMPLE_HD inline void transform_point(const double* T, const double* p, double* out) {
#pragma clang fp contract(off)
  for (int r = 0; r < 3; r++) out[r] = ((T[4 * r] * p[0] + T[4 * r + 1] * p[1]) + T[4 * r + 2] * p[2]) + T[4 * r + 3] * p[3];
  out[3] = p[3];
}

// out_r = (T[4r] n0 + T[4r+1] n1) + T[4r+2] n2: the linear part alone
GLIM_AMD_RESAMPLE_HD inline void transform_normal(const double* T, const double* n, double* out) {
#pragma clang fp contract(off)
  for (int r = 0; r < 3; r++) out[r] = (T[4 * r] * n[0] + T[4 * r + 1] * n[1]) + T[4 * r + 2] * n[2];
}

// c, out: c00 c01 c02 c11 c12 c22.  (L C) L^T, rows by columns, left to right; only the upper triangle of the product is formed
GLIM_AMD_RESAMPLE_HD inline void transform_cov(const double* T, const double* c, double* out) {
#pragma clang fp contract(off)
  const double C[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
  double LC[3][3];
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) LC[r][k] = (T[4 * r] * C[0][k] + T[4 * r + 1] * C[1][k]) + T[4 * r + 2] * C[2][k];
  int o = 0;
  for (int r = 0; r < 3; r++)
    for (int k = r; k < 3; k++) out[o++] = (LC[r][0] * T[4 * k] + LC[r][1] * T[4 * k + 1]) + LC[r][2] * T[4 * k + 2];
}

}  // namespace resample
}  // namespace glim_amd
