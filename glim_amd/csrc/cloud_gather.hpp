// cloud_gather.hpp -- a new cloud from some points of a resident one: the allocation of every per-point array the input holds, and the gather
// of those arrays bit for bit.  Shared by the map editor's removal (map_edit.hip) and by the resampling of a cloud (resample.hip).
// Lazily built members (factor streams, Hilbert rank) and neighbour lists are not carried over: they are rebuilt on first use, and the
// neighbours' indices would be wrong.
#pragma once

#include <algorithm>

#include "internal.hpp"

namespace glim_amd {

struct GatherArgs {
  const float4 *pts, *covA, *normals;
  const float2* covB;
  const double4* pts64;
  const double *times, *intensities, *cov64;
  float4 *o_pts, *o_covA, *o_normals;
  float2* o_covB;
  double4* o_pts64;
  double *o_times, *o_intensities, *o_cov64;
  int* o_index;  // compaction form only: o_index[o] = the input index of output point o (null: not wanted)
};

// Two forms, one copy:
//   idx != null   index form: `count` outputs, output t = input idx[t] (any order, duplicates allowed)
//   idx == null   compaction form: `count` inputs, input t goes to output pos[t] iff keep[t]
static __global__ __launch_bounds__(256) void cloud_gather_kernel(int count, const int* __restrict__ keep, const int* __restrict__ pos,
                                                                  const int* __restrict__ idx, GatherArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= count) return;
  int i, o;
  if (idx) {
    i = idx[t], o = t;
  } else {
    if (!keep[t]) return;
    i = t, o = pos[t];
    if (a.o_index) a.o_index[o] = i;
  }
  a.o_pts[o] = a.pts[i];
  if (a.covA) a.o_covA[o] = a.covA[i];
  if (a.covB) a.o_covB[o] = a.covB[i];
  if (a.normals) a.o_normals[o] = a.normals[i];
  if (a.pts64) a.o_pts64[o] = a.pts64[i];
  if (a.times) a.o_times[o] = a.times[i];
  if (a.intensities) a.o_intensities[o] = a.intensities[i];
  if (a.cov64)
    for (int c = 0; c < 6; c++) a.o_cov64[6 * (size_t)o + c] = a.cov64[6 * (size_t)i + c];
}

// destroys the cloud it still holds when it leaves scope; declare it BEFORE the lock of the context's mutex (the destruction takes none, but
// it quiesces the device)
struct CloudGuard {
  glim_amd_cloud* c = nullptr;
  ~CloudGuard() {
    if (c) glim_amd_cloud_destroy(c);
  }
};

// A cloud of m points in src's context with every per-point array src holds, uninitialised; has_covs / has_normals / plane_form follow src.
// The cloud is handed to `guard` at once, so that a failed allocation leaves nothing behind.  Caller holds the context's mutex, device set.
inline int alloc_cloud_like(const glim_amd_cloud* src, int64_t m, CloudGuard* guard) {
  glim_amd_cloud* c = new glim_amd_cloud();
  guard->c = c;
  c->ctx = (glim_amd_ctx*)src->ctx;
  c->n = m;
  const size_t nn = (size_t)std::max<int64_t>(m, 1);
  GA_HIP(pool_malloc(&c->pts, nn * sizeof(float4)));
  if (src->covA) GA_HIP(pool_malloc(&c->covA, nn * sizeof(float4)));
  if (src->covB) GA_HIP(pool_malloc(&c->covB, nn * sizeof(float2)));
  if (src->normals) GA_HIP(pool_malloc(&c->normals, nn * sizeof(float4)));
  if (src->pts64) GA_HIP(pool_malloc(&c->pts64, nn * sizeof(double4)));
  if (src->times) GA_HIP(pool_malloc(&c->times, nn * sizeof(double)));
  if (src->intensities) GA_HIP(pool_malloc(&c->intensities, nn * sizeof(double)));
  if (src->cov64) GA_HIP(pool_malloc(&c->cov64, nn * 6 * sizeof(double)));
  c->has_covs = src->has_covs;
  c->has_normals = src->has_normals;
  c->plane_form = src->plane_form;
  return GLIM_AMD_OK;
}

inline GatherArgs gather_args(const glim_amd_cloud* src, glim_amd_cloud* c) {
  GatherArgs a;
  a.pts = src->pts, a.covA = src->covA, a.covB = src->covB, a.normals = src->normals, a.pts64 = src->pts64, a.times = src->times;
  a.intensities = src->intensities, a.cov64 = src->cov64;
  a.o_pts = c->pts, a.o_covA = c->covA, a.o_covB = c->covB, a.o_normals = c->normals, a.o_pts64 = c->pts64, a.o_times = c->times;
  a.o_intensities = c->intensities, a.o_cov64 = c->cov64;
  a.o_index = nullptr;
  return a;
}

// enqueues the gather on `st` (nothing when count is 0); see cloud_gather_kernel for the two forms
inline hipError_t cloud_gather(hipStream_t st, int count, const int* keep, const int* pos, const int* idx, const GatherArgs& a) {
  if (count <= 0) return hipSuccess;
  cloud_gather_kernel<<<(count + 255) / 256, 256, 0, st>>>(count, keep, pos, idx, a);
  return hipGetLastError();
}

}  // namespace glim_amd
