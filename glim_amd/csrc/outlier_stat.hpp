// outlier_stat.hpp -- the statistical outlier rule of gtsam_points::remove_outliers / find_inlier_points: mean distance to the k nearest
// neighbours against mean + std_mul * std over the cloud.  Shared by the scan preprocessing (preprocess.hip, cloud_preprocessor.cpp:162-164)
// and the map editor's outlier selection (map_edit.hip, points_selector.cpp:746).  FP64, deterministic sums (fixed butterfly per block,
// block order across blocks).
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "internal.hpp"

namespace glim_amd {
namespace outlier_detail {

static __global__ __launch_bounds__(256) void pp_mean_dist_kernel(int f, const double4* __restrict__ P, const int* __restrict__ nb, int k,
                                                                  double* __restrict__ d, double* __restrict__ partial) {
  __shared__ double s_sum[4], s_sq[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double di = 0.0;
  if (i < f) {
    const double4 p = P[i];
    double s = 0.0;
    for (int j = 0; j < k; j++) {
      const double4 q = P[nb[(size_t)i * k + j]];
      const double dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
      s += __dsqrt_rn(dadd(dadd(dmul(dx, dx), dmul(dy, dy)), dmul(dz, dz)));
    }
    di = s / (double)k;
    d[i] = di;
  }
  // deterministic block sums of d and d^2 (fixed butterfly order), one partial pair per block
  double a = di, b = dmul(di, di);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_sum[threadIdx.x >> 6] = a;
    s_sq[threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    partial[2 * blockIdx.x + 1] = (s_sq[0] + s_sq[1]) + (s_sq[2] + s_sq[3]);
  }
}

static __global__ void pp_outlier_thresh_kernel(int f, int blocks, const double* __restrict__ partial, double std_mul, double* __restrict__ thresh) {
  double sum = 0.0, sq = 0.0;
  for (int b = 0; b < blocks; b++) {  // block order: deterministic
    sum += partial[2 * b];
    sq += partial[2 * b + 1];
  }
  const double mean = sum / (double)f;
  const double var = sq / (double)f - dmul(mean, mean);
  *thresh = dadd(mean, dmul(std_mul, sqrt(var > 0.0 ? var : 0.0)));
}

static __global__ __launch_bounds__(256) void pp_inlier_flag_kernel(int f, const double* __restrict__ d, const double* __restrict__ thresh,
                                                                    int* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > f) return;
  flags[i] = (i < f && d[i] < *thresh) ? 1 : 0;
}

}  // namespace outlier_detail

// scratch of outlier_inlier_flags: allocated there, to be kept until the kernels have run
struct OutlierScratch {
  DeviceTemp d, partial, thresh;
};

// flags[i] = 1 iff the mean distance d_i of point i to its k neighbours is below mean(d) + std_mul * std(d) over the f points; flags[f] = 0.
// Enqueues on `st`; no synchronisation.
inline hipError_t outlier_inlier_flags(hipStream_t st, int f, const double4* points, const int* neighbors, int k, double std_mul, OutlierScratch* scratch,
                                       int* flags) {
  const int blocks = (f + 255) / 256;
  hipError_t e = pool_malloc(&scratch->d.p, (size_t)(f > 0 ? f : 1) * sizeof(double));
  if (e == hipSuccess) e = pool_malloc(&scratch->partial.p, (size_t)(blocks > 0 ? blocks : 1) * 2 * sizeof(double));
  if (e == hipSuccess) e = pool_malloc(&scratch->thresh.p, sizeof(double));
  if (e != hipSuccess) return e;
  if (f > 0) outlier_detail::pp_mean_dist_kernel<<<blocks, 256, 0, st>>>(f, points, neighbors, k, scratch->d.as<double>(), scratch->partial.as<double>());
  outlier_detail::pp_outlier_thresh_kernel<<<1, 1, 0, st>>>(f, blocks, scratch->partial.as<double>(), std_mul, scratch->thresh.as<double>());
  outlier_detail::pp_inlier_flag_kernel<<<(f + 256) / 256, 256, 0, st>>>(f, scratch->d.as<double>(), scratch->thresh.as<double>(), flags);
  return hipGetLastError();
}

}  // namespace glim_amd
