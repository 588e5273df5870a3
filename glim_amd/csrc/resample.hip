// resample.hip -- a new cloud derived from a resident one without leaving the device: gtsam_points::random_sampling, gtsam_points::sample and
// gtsam_points::transform.  Semantics: include/glim_amd.h "Resampling a resident cloud"; the rules themselves (key, count, transform
// expressions): resample.hpp; allocation and gather of the result: cloud_gather.hpp, shared with the map editor's removal.
//
// Random sampling keeps the m points with the smallest (key, index), key = sample_hash(seed, index) >> 32, in ascending index.  That is a
// SELECTION, not a sort: the m-th smallest key t is found by radix-select passes, then keep[i] = key < t, or key == t and i is among the
// first r points with that key.
//   sample_key_kernel     key of every point, stored once (4 B per point)
//   select_hist_kernel    x 3: digits of 11 / 11 / 10 bits from the top; a block counts the digits of the keys that agree with the prefix found
//                         so far in a 2048-bin LDS histogram and adds its non-empty bins to the global one (integer atomics: any order, same sum)
//   select_pick_kernel    x 3, one block: the bin that holds rank `remaining`; (prefix, remaining) stay in device memory
//   select_tie_kernel     tie[i] = key == t  -> scan.hpp's exclusive prefix sum: the rank of i among the ties
//   select_keep_kernel    the keep flags      -> the same prefix sum: the output positions -> cloud_gather.hpp
// The host knows m before anything is launched, allocates the result up front and synchronises once, at the end.
//
// Keys are stored once and not recomputed per pass: a pass then reads 4 B per point, where the generator is two 64-bit multiplies (sixteen
// 32-bit ones on this hardware) and four 64-bit shifts; five kernels read the key, and the diagnostic entry that selects on a caller's
// keys runs the very same passes.  Neither form has been timed against the other.
// A block of select_hist_kernel takes 8192 keys, so that the 2048 atomics of its flush are few next to its reads; after the first pass only
// about n / 2048 keys still agree with the prefix and nearly every bin is empty.
#include <algorithm>
#include <cmath>

#include "cloud_gather.hpp"
#include "internal.hpp"
#include "resample.hpp"
#include "scan.hpp"
#include "scope_sync.hpp"

namespace glim_amd {
namespace resample {

using u32 = unsigned int;
using u64 = unsigned long long;

constexpr int MAX_BINS = 2048;
constexpr int KEYS_PER_BLOCK = 8192;
constexpr int64_t MAX_POINTS = (int64_t)1 << 28;  // what a cloud may hold (cloud.hip)
// the three digits: shift, bins, mask of the digits above
constexpr int PASS_SHIFT[3] = {21, 10, 0};
constexpr int PASS_BINS[3] = {2048, 2048, 1024};
constexpr u32 PASS_ABOVE[3] = {0u, 0xFFE00000u, 0xFFFFFC00u};

static __global__ __launch_bounds__(256) void sample_key_kernel(int n, u64 seed, u32* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) keys[i] = sample_key(seed, (u64)i);
}

// hist[bins] += digits of the keys with (key & above) == prefix; state[0] = prefix (not read in the first pass, above == 0)
static __global__ __launch_bounds__(256) void select_hist_kernel(const u32* __restrict__ keys, int n, int shift, int bins, u32 above,
                                                                 const u32* __restrict__ state, u32* __restrict__ hist) {
  __shared__ u32 s_hist[MAX_BINS];
  for (int b = threadIdx.x; b < bins; b += 256) s_hist[b] = 0u;
  __syncthreads();
  const u32 prefix = above ? state[0] : 0u;
  const int begin = blockIdx.x * KEYS_PER_BLOCK, end = min(n, begin + KEYS_PER_BLOCK);
  for (int i = begin + (int)threadIdx.x; i < end; i += 256) {
    const u32 k = keys[i];
    if ((k & above) == prefix) atomicAdd(&s_hist[(k >> shift) & (u32)(bins - 1)], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < bins; b += 256) {
    const u32 v = s_hist[b];
    if (v) atomicAdd(&hist[b], v);
  }
}

// One block.  With k = remaining (k_init in the first pass) and c(b) = hist[0] + ... + hist[b - 1]: the bin b with c(b) < k <= c(b) + hist[b];
// prefix |= b << shift, remaining = k - c(b).  After the last pass prefix is the m-th smallest key and remaining how many keys equal to it
// are among the m smallest.
static __global__ __launch_bounds__(256) void select_pick_kernel(const u32* __restrict__ hist, int bins, int shift, u32 k_init, int first, u32* state) {
  __shared__ u32 s_sum[256];
  const int t = threadIdx.x, per = bins / 256;
  const u32 k = first ? k_init : state[1];
  u32 s = 0u;
  for (int j = 0; j < per; j++) s += hist[t * per + j];
  s_sum[t] = s;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const u32 v = t >= off ? s_sum[t - off] : 0u;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  const u32 incl = s_sum[t];
  u32 c = incl - s;
  if (s > 0u && c < k && k <= incl) {  // exactly one thread when 1 <= k <= the histogram's total
    for (int j = 0; j < per; j++) {
      const u32 h = hist[t * per + j];
      if (k <= c + h) {
        state[0] = (first ? 0u : state[0]) | ((u32)(t * per + j) << shift);
        state[1] = k - c;
        break;
      }
      c += h;
    }
  }
}

static __global__ __launch_bounds__(256) void select_tie_kernel(const u32* __restrict__ keys, int n, const u32* __restrict__ state, int* __restrict__ tie) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) tie[i] = keys[i] == state[0] ? 1 : 0;
}

// keep[n] = 0: the prefix sum over n + 1 entries ends with the number kept
static __global__ __launch_bounds__(256) void select_keep_kernel(const u32* __restrict__ keys, int n, const u32* __restrict__ state,
                                                                 const int* __restrict__ rank, int* __restrict__ keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  int f = 0;
  if (i < n) {
    const u32 k = keys[i], t = state[0];
    f = (k < t || (k == t && (u32)rank[i] < state[1])) ? 1 : 0;
  }
  keep[i] = f;
}

struct Pose12 {
  double m[12];
};

// one lane per point; FP64 arrays are transformed where the cloud holds them and the FP32 ones are their roundings, else the FP32 ones are
// promoted, transformed and rounded.  Times and intensities are copied.
static __global__ __launch_bounds__(256) void transform_kernel(int n, Pose12 T, GatherArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double p[4], q[4];
  if (a.pts64) {
    const double4 v = a.pts64[i];
    p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
  } else {
    const float4 v = a.pts[i];
    p[0] = (double)v.x, p[1] = (double)v.y, p[2] = (double)v.z, p[3] = (double)v.w;
  }
  transform_point(T.m, p, q);
  if (a.pts64) a.o_pts64[i] = make_double4(q[0], q[1], q[2], q[3]);
  a.o_pts[i] = make_float4((float)q[0], (float)q[1], (float)q[2], (float)q[3]);
  if (a.cov64 || (a.covA && a.covB)) {
    double c[6], d[6];
    if (a.cov64) {
      for (int k = 0; k < 6; k++) c[k] = a.cov64[6 * (size_t)i + k];
    } else {
      const float4 ca = a.covA[i];
      const float2 cb = a.covB[i];
      c[0] = (double)ca.x, c[1] = (double)ca.y, c[2] = (double)ca.z, c[3] = (double)ca.w, c[4] = (double)cb.x, c[5] = (double)cb.y;
    }
    transform_cov(T.m, c, d);
    if (a.cov64)
      for (int k = 0; k < 6; k++) a.o_cov64[6 * (size_t)i + k] = d[k];
    if (a.covA) a.o_covA[i] = make_float4((float)d[0], (float)d[1], (float)d[2], (float)d[3]);
    if (a.covB) a.o_covB[i] = make_float2((float)d[4], (float)d[5]);
  }
  if (a.normals) {
    const float4 v = a.normals[i];
    const double nv[3] = {(double)v.x, (double)v.y, (double)v.z};
    double r[3];
    transform_normal(T.m, nv, r);
    a.o_normals[i] = make_float4((float)r[0], (float)r[1], (float)r[2], v.w);
  }
  if (a.times) a.o_times[i] = a.times[i];
  if (a.intensities) a.o_intensities[i] = a.intensities[i];
}

static inline int grid_for(int n) { return (n + 255) / 256; }

// the selection's scratch; `keep` holds n + 1 flags, the last 0
struct Selection {
  DeviceTemp hist, tie, rank, keep, tiles;
};

// keep flags of the m smallest (key, index) of keys[n], 1 <= m <= n: enqueued on st, no synchronisation
static int select_enqueue(hipStream_t st, const u32* keys, int n, int m, Selection* s) {
  const size_t words = 3 * (size_t)MAX_BINS + 2;  // three histograms, then (prefix, remaining)
  GA_HIP(pool_malloc(&s->hist.p, words * sizeof(u32)));
  GA_HIP(pool_malloc(&s->tie.p, (size_t)n * sizeof(int)));
  GA_HIP(pool_malloc(&s->rank.p, (size_t)n * sizeof(int)));
  GA_HIP(pool_malloc(&s->keep.p, ((size_t)n + 1) * sizeof(int)));
  GA_HIP(pool_malloc(&s->tiles.p, scan_scratch_ints((unsigned int)n + 1u) * sizeof(int)));
  u32* state = s->hist.as<u32>() + 3 * MAX_BINS;
  GA_HIP(hipMemsetAsync(s->hist.p, 0, words * sizeof(u32), st));
  const int blocks = (n + KEYS_PER_BLOCK - 1) / KEYS_PER_BLOCK;
  for (int p = 0; p < 3; p++) {
    u32* hist = s->hist.as<u32>() + p * MAX_BINS;
    select_hist_kernel<<<blocks, 256, 0, st>>>(keys, n, PASS_SHIFT[p], PASS_BINS[p], PASS_ABOVE[p], state, hist);
    select_pick_kernel<<<1, 256, 0, st>>>(hist, PASS_BINS[p], PASS_SHIFT[p], (u32)m, p == 0, state);
  }
  select_tie_kernel<<<grid_for(n), 256, 0, st>>>(keys, n, state, s->tie.as<int>());
  GA_HIP(hipGetLastError());
  GA_HIP(exclusive_scan_int(st, s->tie.as<int>(), (unsigned int)n, s->tiles.as<int>(), s->rank.as<int>()));
  select_keep_kernel<<<grid_for(n + 1), 256, 0, st>>>(keys, n, state, s->rank.as<int>(), s->keep.as<int>());
  GA_HIP(hipGetLastError());
  return GLIM_AMD_OK;
}

// every per-point array of src copied into c (same size), on st
static int copy_arrays(hipStream_t st, const glim_amd_cloud* src, glim_amd_cloud* c) {
  const size_t n = (size_t)src->n;
  if (n == 0) return GLIM_AMD_OK;
  GA_HIP(hipMemcpyAsync(c->pts, src->pts, n * sizeof(float4), hipMemcpyDeviceToDevice, st));
  if (src->covA) GA_HIP(hipMemcpyAsync(c->covA, src->covA, n * sizeof(float4), hipMemcpyDeviceToDevice, st));
  if (src->covB) GA_HIP(hipMemcpyAsync(c->covB, src->covB, n * sizeof(float2), hipMemcpyDeviceToDevice, st));
  if (src->normals) GA_HIP(hipMemcpyAsync(c->normals, src->normals, n * sizeof(float4), hipMemcpyDeviceToDevice, st));
  if (src->pts64) GA_HIP(hipMemcpyAsync(c->pts64, src->pts64, n * sizeof(double4), hipMemcpyDeviceToDevice, st));
  if (src->times) GA_HIP(hipMemcpyAsync(c->times, src->times, n * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (src->intensities) GA_HIP(hipMemcpyAsync(c->intensities, src->intensities, n * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (src->cov64) GA_HIP(hipMemcpyAsync(c->cov64, src->cov64, n * 6 * sizeof(double), hipMemcpyDeviceToDevice, st));
  return GLIM_AMD_OK;
}

}  // namespace resample
}  // namespace glim_amd

extern "C" {

int glim_amd_cloud_random_sample(const glim_amd_cloud* cloud, double rate, uint64_t seed, glim_amd_cloud** out) {
  using namespace glim_amd;
  using namespace glim_amd::resample;
  if (!cloud || !out || !std::isfinite(rate) || rate < 0.0) return GLIM_AMD_ERR_INVALID;
  *out = nullptr;
  if (cloud->n > MAX_POINTS) return GLIM_AMD_ERR_INVALID;
  const int n = (int)cloud->n;
  const int m = (int)sample_count(n, rate);
  glim_amd_ctx* ctx = cloud->ctx;
  const bool host_times = n > 0 && cloud->h_times.size() == (size_t)n;
  CloudGuard result;  // destroyed after the lock
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  GA_TRY(alloc_cloud_like(cloud, m, &result));
  glim_amd_cloud* c = result.c;
  if (m == n) {  // the whole cloud (rate >= FULL_RATE, or an empty cloud)
    SyncOnExit in_flight(st);
    GA_TRY(copy_arrays(st, cloud, c));
    if (host_times) c->h_times = cloud->h_times;
    GA_HIP(hipStreamSynchronize(st));
    in_flight.dismiss();
  } else if (m > 0) {
    DeviceTemp keys, pos, index;
    Selection sel;
    std::vector<int> h_index;
    GA_HIP(pool_malloc(&keys.p, (size_t)n * sizeof(u32)));
    GA_HIP(pool_malloc(&pos.p, ((size_t)n + 1) * sizeof(int)));
    if (host_times) {
      GA_HIP(pool_malloc(&index.p, (size_t)m * sizeof(int)));
      h_index.resize((size_t)m);
    }
    SyncOnExit in_flight(st);
    sample_key_kernel<<<grid_for(n), 256, 0, st>>>(n, (u64)seed, keys.as<u32>());
    GA_HIP(hipGetLastError());
    GA_TRY(select_enqueue(st, keys.as<u32>(), n, m, &sel));
    GA_HIP(exclusive_scan_int(st, sel.keep.as<int>(), (unsigned int)n + 1u, sel.tiles.as<int>(), pos.as<int>()));
    GatherArgs a = gather_args(cloud, c);
    a.o_index = index.as<int>();
    GA_HIP(cloud_gather(st, n, sel.keep.as<int>(), pos.as<int>(), nullptr, a));
    if (host_times) GA_HIP(hipMemcpyAsync(h_index.data(), index.p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, st));
    GA_HIP(hipStreamSynchronize(st));
    in_flight.dismiss();
    if (host_times) {
      c->h_times.resize((size_t)m);
      for (int j = 0; j < m; j++) {
        if (h_index[(size_t)j] < 0 || h_index[(size_t)j] >= n) return GLIM_AMD_ERR_HIP;
        c->h_times[(size_t)j] = cloud->h_times[(size_t)h_index[(size_t)j]];
      }
    }
  }
  *out = c;
  result.c = nullptr;
  return GLIM_AMD_OK;
}

int glim_amd_cloud_sample(const glim_amd_cloud* cloud, int64_t m, const int32_t* indices, glim_amd_cloud** out) {
  using namespace glim_amd;
  using namespace glim_amd::resample;
  if (!cloud || !out || m < 0 || (m > 0 && !indices) || m > MAX_POINTS) return GLIM_AMD_ERR_INVALID;
  *out = nullptr;
  const int64_t n = cloud->n;
  for (int64_t j = 0; j < m; j++)
    if (indices[j] < 0 || indices[j] >= n) return GLIM_AMD_ERR_INVALID;
  glim_amd_ctx* ctx = cloud->ctx;
  CloudGuard result;  // destroyed after the lock
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  GA_TRY(alloc_cloud_like(cloud, m, &result));
  glim_amd_cloud* c = result.c;
  if (m > 0) {
    DeviceTemp idx;
    GA_HIP(pool_malloc(&idx.p, (size_t)m * sizeof(int)));
    SyncOnExit in_flight(st);
    GA_HIP(hipMemcpyAsync(idx.p, indices, (size_t)m * sizeof(int), hipMemcpyHostToDevice, st));
    GA_HIP(cloud_gather(st, (int)m, nullptr, nullptr, idx.as<int>(), gather_args(cloud, c)));
    if (cloud->h_times.size() == (size_t)n) {
      c->h_times.resize((size_t)m);
      for (int64_t j = 0; j < m; j++) c->h_times[(size_t)j] = cloud->h_times[(size_t)indices[j]];
    }
    GA_HIP(hipStreamSynchronize(st));
    in_flight.dismiss();
  }
  *out = c;
  result.c = nullptr;
  return GLIM_AMD_OK;
}

int glim_amd_cloud_transform(const glim_amd_cloud* cloud, const double* T12, glim_amd_cloud** out) {
  using namespace glim_amd;
  using namespace glim_amd::resample;
  if (!cloud || !out || !T12) return GLIM_AMD_ERR_INVALID;
  *out = nullptr;
  Pose12 T;
  for (int k = 0; k < 12; k++) {
    if (!std::isfinite(T12[k])) return GLIM_AMD_ERR_INVALID;
    T.m[k] = T12[k];
  }
  if (cloud->n > MAX_POINTS) return GLIM_AMD_ERR_INVALID;
  const int n = (int)cloud->n;
  glim_amd_ctx* ctx = cloud->ctx;
  CloudGuard result;  // destroyed after the lock
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  GA_TRY(alloc_cloud_like(cloud, n, &result));
  glim_amd_cloud* c = result.c;
  c->plane_form = false;
  if (n > 0) {
    SyncOnExit in_flight(st);
    transform_kernel<<<grid_for(n), 256, 0, st>>>(n, T, gather_args(cloud, c));
    GA_HIP(hipGetLastError());
    if (cloud->h_times.size() == (size_t)n) c->h_times = cloud->h_times;
    GA_HIP(hipStreamSynchronize(st));
    in_flight.dismiss();
    GA_TRY(detect_plane_form(c, st));  // on the result's arrays, as an upload of them would decide
  }
  *out = c;
  result.c = nullptr;
  return GLIM_AMD_OK;
}

int glim_amd_debug_select_smallest(glim_amd_ctx* ctx, int64_t n, const uint32_t* keys32, int64_t m, int32_t* keep_out) {
  using namespace glim_amd;
  using namespace glim_amd::resample;
  if (!ctx || n < 0 || n > MAX_POINTS || m < 0 || m > n || (n > 0 && (!keys32 || !keep_out))) return GLIM_AMD_ERR_INVALID;
  if (n == 0) return GLIM_AMD_OK;
  if (m == 0) {  // nothing to select: what glim_amd_cloud_random_sample does, too
    std::fill(keep_out, keep_out + n, 0);
    return GLIM_AMD_OK;
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  DeviceTemp keys;
  Selection sel;
  GA_HIP(pool_malloc(&keys.p, (size_t)n * sizeof(u32)));
  SyncOnExit in_flight(st);
  GA_HIP(hipMemcpyAsync(keys.p, keys32, (size_t)n * sizeof(u32), hipMemcpyHostToDevice, st));
  GA_TRY(select_enqueue(st, keys.as<u32>(), (int)n, (int)m, &sel));
  GA_HIP(hipMemcpyAsync(keep_out, sel.keep.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  return GLIM_AMD_OK;
}

}  // extern "C"
