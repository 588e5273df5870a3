// gicp.hip -- the GICP (nearest-neighbour correspondence) matching-cost factor on gfx950.
//
// Replaces gtsam_points::IntegratedGICPFactor::{linearize, error, inlier_fraction} as constructed at
// src/glim/mapping/sub_mapping.cpp:202 (between factors), src/glim/mapping/global_mapping.cpp:400 (10 LM iterations between
// consecutive submaps) and src/glim/mapping/global_mapping_pose_graph.cpp:393 (loop-candidate validation, with the target's
// pre-built search tree `candidate.target->tree`).  Same cost as the VGICP factor (vgicp.hip) except for the correspondence:
//
//   q = R p + t                                   FP64, the oracle's fma order (shared with the VGICP factor)
//   j = argmin_j |q - b_j|^2 over the target      exact: FP64 (dx^2 + dy^2) + dz^2 with separate roundings, ties to the smaller index
//   valid iff |q - b_j|^2 <= max_correspondence_distance^2
//   M = (C_B[j] + R C_A R^T)^-1,  r = b_j - q,  e = r^T M r,  H_ss += J_s^T M J_s, b_s += J_s^T M r      (as vgicp.hip)
//
// Search structure = the kd-tree's stand-in (glim_amd_nn_index, built once per target cloud and reused by every linearisation,
// like `candidate.target->tree`): the target points counting-sorted into a uniform grid.  The sort is the stable radix sort of
// sort.hip on cell keys compacted to the bounding box, so the sorted order -- (cell, original index) -- is deterministic; an
// open-addressing table maps a cell key to its [begin, end) run.  A query walks growing Chebyshev rings of cells around q's cell
// and stops as soon as the best distance is provably inside the scanned cube, or the cube already covers the correspondence
// radius (nothing farther can be accepted).  One lane per source point; the per-point algebra and the block reduction are the
// VGICP ones (source-frame form, 28 FP32 accumulators, DPP wave sums, fixed-order FP64 finalisation: bit-reproducible).
//
// The continuous-time factor (gtsam_points::IntegratedCT_GICPFactor with a point-cloud target, odometry_estimation_ct.cpp:158-195) runs the same
// search and per-point algebra with one pose per time bucket, T_k = X Exp(t_k Log(X^-1 Y)); its chain rule to the keys X and Y is applied per
// bucket in FP64 (ct_gicp_kernel, ct_bucket_kernel, ct_sum_kernel below; semantics in include/glim_amd.h, layout in DESIGN.md 4.6).
//
// Both factors also run over a device iVox (gtsam_points::IncrementalVoxelMap<FlatContainer>, ivox.hip: the container and its insert): the
// factor kernels take the target kind as a template parameter -- IndexSearch = the exact search above, IvoxSearch = the map's bounded search of
// the voxels of its neighbour mode -- and share everything behind the correspondence.  What ivox.hip, gicp_align.hip and ct_align.hip use as well -- the
// searches, the per-point algebra, the block epilogue, the target description -- is gicp_factor.hpp's; the map object is ivox_map.hpp's.
//
// The ICP factors (gtsam_points::IntegratedICPFactor, IntegratedPointToPlaneICPFactor; manual_loop_close_modal.cpp:485-490) are the rigid factor
// with another metric: icp_kernel below runs the same search and epilogue over icp_factor.hpp's per-point algebra, through run_gicp with a metric
// argument.  Neither cloud needs covariances; point-to-plane reads the target's normals through the original index of the matched point.
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "ct_factor.hpp"
#include "device_math.hpp"
#include "gicp_factor.hpp"
#include "icp_factor.hpp"
#include "internal.hpp"
#include "ivox_map.hpp"
#include "scan.hpp"
#include "scope_sync.hpp"

using namespace glim_amd;

namespace {

// ---- index build ----
__global__ __launch_bounds__(256) void gi_key_kernel(int n, const float4* __restrict__ pts, double inv_h, u64* __restrict__ vkey, int* __restrict__ bb) {
  __shared__ int s_tmp[16];
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float4 p = pts[i];
    const double t[3] = {(double)p.x * inv_h, (double)p.y * inv_h, (double)p.z * inv_h};
    bool valid = true;
#pragma unroll
    for (int a = 0; a < 3; a++) valid = valid && (t[a] >= -1048576.0 && t[a] < 1048576.0);
    u64 key = EMPTY_KEY;
    if (valid) {
      int c[3];
#pragma unroll
      for (int a = 0; a < 3; a++) {
        c[a] = fast_floor_d(t[a]) + KEY_OFFSET;
        lo[a] = min(lo[a], c[a]);
        hi[a] = max(hi[a], c[a]);
      }
      key = (u64)c[0] | ((u64)c[1] << 21) | ((u64)c[2] << 42);
    }
    vkey[i] = key;
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = block_reduce_i<0>(lo[a], s_tmp);
    hi[a] = block_reduce_i<1>(hi[a], s_tmp);
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      if (lo[a] != 0x7fffffff) atomicMin(&bb[a], lo[a]);
      if (hi[a] != (int)0x80000000) atomicMax(&bb[3 + a], hi[a]);
    }
  }
}

__global__ __launch_bounds__(256) void gi_compact_key_kernel(int n, const u64* __restrict__ vkey, int xmin, int ymin, int zmin, int bx, int by, int vbits,
                                                             u64* __restrict__ ckey) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u64 k = vkey[i];
  if (k == EMPTY_KEY) {
    ckey[i] = 1ull << vbits;  // points without a cell (non-finite / out of range) sort last and are never indexed
    return;
  }
  const u64 x = (k & 0x1FFFFFull) - (u64)xmin, y = ((k >> 21) & 0x1FFFFFull) - (u64)ymin, z = ((k >> 42) & 0x1FFFFFull) - (u64)zmin;
  ckey[i] = (z << (bx + by)) | (y << bx) | x;
}

// sorted order -> gather the points / covariances, and register every cell run in the table
__global__ __launch_bounds__(256) void gi_gather_kernel(int n, const u64* __restrict__ ckey_sorted, const u32* __restrict__ order, u64 invalid,
                                                        const u64* __restrict__ vkey, const float4* __restrict__ pts, const float4* __restrict__ covA,
                                                        const float2* __restrict__ covB, float4* __restrict__ sorted, float4* __restrict__ sA,
                                                        float2* __restrict__ sB, u64* __restrict__ keys, int2* __restrict__ runs, u32 mask) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const u32 i = order[j];
  const float4 p = pts[i];
  sorted[j] = make_float4(p.x, p.y, p.z, __int_as_float((int)i));
  if (covA) {
    sA[j] = covA[i];
    sB[j] = covB[i];
  }
  const u64 ck = ckey_sorted[j];
  if (ck == invalid) return;
  const bool head = j == 0 || ckey_sorted[j - 1] != ck;
  const bool tail = j == n - 1 || ckey_sorted[j + 1] != ck;
  if (!head && !tail) return;
  // the full (uncompacted) cell key identifies the cell; the head claims the slot, head and tail fill begin / end
  const u64 key = vkey[i];
  u32 s = cell_hash(key) & mask;
  for (;;) {
    const u64 prev = atomicCAS(&keys[s], EMPTY_KEY, key);
    if (prev == EMPTY_KEY || prev == key) break;
    s = (s + 1) & mask;
  }
  if (head) runs[s].x = j;
  if (tail) runs[s].y = j + 1;
}

template <bool LINEARIZE, class NN>
__global__ __launch_bounds__(BLOCK) void gicp_kernel(const GicpArgs a, float* __restrict__ partials, int32_t* __restrict__ corr, const NN nn) {
  __shared__ float s_red[4][PARTIAL_STRIDE];
  const double* T = a.T;
  const Rot32 R(T);
  float acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; j++) acc[j] = 0.f;
  int inliers = 0;
  const int base = blockIdx.x * (BLOCK * a.ppt) + threadIdx.x;
  for (int it = 0; it < a.ppt; it++) {
    const int i = base + it * BLOCK;
    if (i >= a.n) break;
    const float4 p = a.pts[i];
    double qx, qy, qz;
    transform_point_d(T, (double)p.x, (double)p.y, (double)p.z, qx, qy, qz);
    double best_d;
    const int j = nn.find(a, qx, qy, qz, best_d);
    if (corr) corr[i] = j >= 0 ? __float_as_int(a.sorted[j].w) : -1;
    if (j < 0) continue;
    inliers++;
    float A[6];
    gicp_point<LINEARIZE>(acc, R.r00, R.r01, R.r02, R.r10, R.r11, R.r12, R.r20, R.r21, R.r22, p, a.sorted[j], a.tA[j], a.tB[j], a.covA[i], a.covB[i], qx, qy, qz,
                          A);
  }
  store_partial_row(acc, inliers, s_red, partials);
}

// The ICP factors (IntegratedICPFactor, IntegratedPointToPlaneICPFactor; include/glim_amd.h "ICP factors") over a search index: gicp_kernel's
// cut of the source, its search and its epilogue, with icp_factor.hpp's per-point algebra.  normals: the target cloud's, in its original order
// (PLANE only)
template <bool LINEARIZE, bool PLANE>
__global__ __launch_bounds__(BLOCK) void icp_kernel(const GicpArgs a, const float4* __restrict__ normals, float* __restrict__ partials, int32_t* __restrict__ corr) {
  __shared__ float s_red[4][PARTIAL_STRIDE];
  const double* T = a.T;
  const Rot32 R(T);
  const IndexSearch nn{};
  float acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; j++) acc[j] = 0.f;
  int inliers = 0;
  const int base = blockIdx.x * (BLOCK * a.ppt) + threadIdx.x;
  for (int it = 0; it < a.ppt; it++) {
    const int i = base + it * BLOCK;
    if (i >= a.n) break;
    const float4 p = a.pts[i];
    double qx, qy, qz;
    transform_point_d(T, (double)p.x, (double)p.y, (double)p.z, qx, qy, qz);
    double best_d;
    const int j = nn.find(a, qx, qy, qz, best_d);
    if (corr) corr[i] = j >= 0 ? __float_as_int(a.sorted[j].w) : -1;
    if (j < 0) continue;
    inliers++;
    const float4 b = a.sorted[j];
    icp_point<LINEARIZE, PLANE>(acc, R, p, b, PLANE ? icp_normal(normals, b) : make_float4(0.f, 0.f, 0.f, 0.f), qx, qy, qz);
  }
  store_partial_row(acc, inliers, s_red, partials);
}

// fixed-order FP64 sum of the block partials -> compact record (one block of 256 threads)
__global__ __launch_bounds__(256) void gicp_finalize_kernel(const float* __restrict__ partials, int nb, int linearize, double* __restrict__ out) {
  __shared__ double s_part[8][PARTIAL_STRIDE];
  __shared__ double s_sum[PARTIAL_STRIDE];
  sum_partial_rows(partials, nb, s_part, s_sum);
  const int t = threadIdx.x;
  if (t < COMPACT) out[t] = (linearize || t < 2) ? compact_entry(s_sum, t) : 0.0;
}

// ---- the continuous-time factor (IntegratedCT_GICPFactor): the same per-point algebra, one pose per time bucket ----
// The layout, the arguments and the bodies of the three passes are ct_factor.hpp's (ct_align.hip runs them inside its rounds as well).
template <bool LINEARIZE, class NN>
__global__ __launch_bounds__(BLOCK) void ct_gicp_kernel(const GicpArgs a, const CtArgs c, float* __restrict__ partials, const NN nn) {
  __shared__ float s_red[4][PARTIAL_STRIDE];
  ct_gicp_block<LINEARIZE, NN>(a, c, partials, nn, s_red);
}

// error(): the kept correspondences and M at new poses -- e = sum r^T M r, r = b_j - T_k p_i (FP64, then FP32).  Partial rows hold e (27) and the
// count (28) only, so gicp_finalize_kernel (linearize = 0) turns them into the record.
__global__ __launch_bounds__(BLOCK) void ct_error_kernel(const GicpArgs a, const CtArgs c, float* __restrict__ partials) {
  __shared__ float s_red[4][2];
  const int4 blk = c.blocks[blockIdx.x];
  const double* T = c.poses + (size_t)blk.x * CT_POSE_STRIDE;
  float e = 0.f;
  int inliers = 0;
  for (int i = blk.y + (int)threadIdx.x; i < blk.z; i += BLOCK) {
    const int j = c.keep_corr[i];
    if (j < 0) continue;
    const float4 p = a.pts[i];
    double qx, qy, qz;
    transform_point_d(T, (double)p.x, (double)p.y, (double)p.z, qx, qy, qz);
    const float4 b = a.sorted[j];
    const float rx = (float)((double)b.x - qx), ry = (float)((double)b.y - qy), rz = (float)((double)b.z - qz);
    const float4 m0 = c.keep_m0[i];
    const float2 m1 = c.keep_m1[i];
    const float ux = m0.x * rx + m0.y * ry + m0.z * rz;
    const float uy = m0.y * rx + m0.w * ry + m1.x * rz;
    const float uz = m0.z * rx + m1.x * ry + m1.y * rz;
    e += rx * ux + ry * uy + rz * uz;
    inliers++;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float se = wave_sum_to_lane63(e);
  const float si = wave_sum_to_lane63((float)inliers);
  if (lane == 63) {
    s_red[wave][0] = se;
    s_red[wave][1] = si;
  }
  __syncthreads();
  if (threadIdx.x < PARTIAL_STRIDE) {
    const int j = threadIdx.x;
    float v = 0.f;
    if (j == 27) v = sum_of_waves(s_red, 0);
    if (j == 28) v = sum_of_waves(s_red, 1);
    partials[(size_t)blockIdx.x * PARTIAL_STRIDE + j] = v;
  }
}

// one block of 64 threads per bucket (ct_factor.hpp)
__global__ __launch_bounds__(64) void ct_bucket_kernel(const float* __restrict__ partials, const int* __restrict__ bucket_first, const double* __restrict__ poses,
                                                       double* __restrict__ rows) {
  __shared__ CtBucketShared s;
  ct_bucket_block(partials, bucket_first, poses, rows, s);
}

// one block: the bucket rows summed in a fixed order -> the record
__global__ __launch_bounds__(CT_SUM_THREADS) void ct_sum_kernel(const double* __restrict__ rows, int nbk, double* __restrict__ out) {
  __shared__ double s_part[8][96];
  ct_sum_rows<CT_SUM_THREADS>(rows, nbk, s_part, out);
}

// deskewed_source_points: T[time_index[i]] p_i in FP64 (the source's exact points where it keeps them), table of 12 doubles per bucket
__global__ __launch_bounds__(256) void ct_deskew_kernel(int n, const double4* __restrict__ pts64, const float4* __restrict__ pts, const int* __restrict__ time_index,
                                                        const double* __restrict__ table, double4* __restrict__ out64, float4* __restrict__ out32) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double4 p;
  if (pts64) {
    p = pts64[i];
  } else {
    const float4 f = pts[i];
    p = make_double4((double)f.x, (double)f.y, (double)f.z, 1.0);
  }
  const double* T = table + 12 * (size_t)time_index[i];
  double4 q;
  q.x = dadd(dadd(dadd(dmul(T[0], p.x), dmul(T[1], p.y)), dmul(T[2], p.z)), T[3]);
  q.y = dadd(dadd(dadd(dmul(T[4], p.x), dmul(T[5], p.y)), dmul(T[6], p.z)), T[7]);
  q.z = dadd(dadd(dadd(dmul(T[8], p.x), dmul(T[9], p.y)), dmul(T[10], p.z)), T[11]);
  q.w = 1.0;
  out64[i] = q;
  if (out32) out32[i] = make_float4((float)q.x, (float)q.y, (float)q.z, 1.0f);
}

inline int bits_for(int range) {
  int b = 0;
  while (range > 0) {
    b++;
    range >>= 1;
  }
  return b;
}

// one synchronous evaluation of the rigid factor over either kind of target; corr_host: n positions (original target index / the map's
// slot * cap + place, or -1), or null.  metric: the GICP factor (both clouds need covariances), or one of the ICP factors over a search index
// (no covariances; point-to-plane needs the target's normals)
int run_gicp(const GicpTarget& t, const glim_amd_cloud* source, const double* T12, double max_dist, bool linearize, double* compact_host,
             int32_t* corr_host, Metric metric = Metric::GICP) {
  if (!t.ctx || !source || !T12 || !(max_dist >= 0.0)) return GLIM_AMD_ERR_INVALID;
  if (source->ctx->device != t.ctx->device) return GLIM_AMD_ERR_INVALID;
  if (source->n > t.max_source) return GLIM_AMD_ERR_INVALID;
  GA_TRY(metric_state(metric, t, source));
  glim_amd_ctx* ctx = t.ctx;
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  const int n = (int)source->n;
  for (int i = 0; i < COMPACT; i++) compact_host[i] = 0.0;
  if (n == 0 || t.empty) {
    if (corr_host)
      for (int i = 0; i < n; i++) corr_host[i] = -1;
    return GLIM_AMD_OK;
  }
  GicpArgs a = t.args;
  set_source(&a, source, points_per_thread(ctx, n), max_dist);
  memcpy(a.T, T12, sizeof(a.T));
  a.max_ring = t.rings(max_dist);
  if (a.max_ring < 0) return GLIM_AMD_ERR_UNSUPPORTED;
  const int nb = (n + BLOCK * a.ppt - 1) / (BLOCK * a.ppt);
  DeviceTemp partials, compact, corr;
  SyncOnExit in_flight(st);  // an error exit after the launches waits for the stream before the scratch goes back to the pool
  GA_HIP(pool_malloc(&partials.p, (size_t)nb * PARTIAL_STRIDE * sizeof(float)));
  GA_HIP(pool_malloc(&compact.p, COMPACT * sizeof(double)));
  if (corr_host) GA_HIP(pool_malloc(&corr.p, (size_t)n * sizeof(int32_t)));
  if (metric == Metric::GICP) {
    with_search(t, [&](auto nn) {
      if (linearize) gicp_kernel<true, decltype(nn)><<<nb, BLOCK, 0, st>>>(a, partials.as<float>(), corr.as<int32_t>(), nn);
      else gicp_kernel<false, decltype(nn)><<<nb, BLOCK, 0, st>>>(a, partials.as<float>(), corr.as<int32_t>(), nn);
    });
  } else {
    const bool plane = metric == Metric::ICP_PLANE;
    auto launch = [&](auto kernel) { kernel<<<nb, BLOCK, 0, st>>>(a, t.normals, partials.as<float>(), corr.as<int32_t>()); };
    if (linearize) plane ? launch(icp_kernel<true, true>) : launch(icp_kernel<true, false>);
    else plane ? launch(icp_kernel<false, true>) : launch(icp_kernel<false, false>);
  }
  gicp_finalize_kernel<<<1, 256, 0, st>>>(partials.as<float>(), nb, linearize ? 1 : 0, compact.as<double>());
  GA_HIP(hipGetLastError());
  GA_HIP(hipMemcpyAsync(compact_host, compact.p, COMPACT * sizeof(double), hipMemcpyDeviceToHost, st));
  if (corr_host) GA_HIP(hipMemcpyAsync(corr_host, corr.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  return GLIM_AMD_OK;
}

// the three entry points of the rigid factor, over the description of either kind
int gicp_linearize(const GicpTarget& t, const glim_amd_cloud* source, const double* T12, double max_dist, uint32_t flags, glim_amd_linearized6* out,
                   Metric metric = Metric::GICP) {
  if (!out) return GLIM_AMD_ERR_INVALID;
  double compact[COMPACT];
  GA_TRY(run_gicp(t, source, T12, max_dist, true, compact, nullptr, metric));
  return glim_amd_expand_compact(compact, T12, flags, out);
}

int gicp_error(const GicpTarget& t, const glim_amd_cloud* source, const double* T12, double max_dist, double* error, int64_t* num_inliers,
               Metric metric = Metric::GICP) {
  double compact[COMPACT];
  GA_TRY(run_gicp(t, source, T12, max_dist, false, compact, nullptr, metric));
  if (error) *error = compact[1];
  if (num_inliers) *num_inliers = (int64_t)llround(compact[0]);
  return GLIM_AMD_OK;
}

// ---- CT factor, host side: the time table and the bucket poses with their derivatives (FP64, gtsam::Pose3 conventions: ct_se3.hpp) ----
using namespace glim_amd::ct_se3;

// T_k, D0_k, D1_k of every bucket at (X, Y): CT_POSE_STRIDE doubles per bucket
void ct_poses(const std::vector<double>& table, const double* X, const double* Y, double* out) { ct_pose_table(table.data(), table.size(), X, Y, out); }

enum { CT_LINEARIZE = 0, CT_ERROR = 1, CT_CORR = 2 };

// the search pass of the factor: correspondences (and, with keep_* set, the M of every point) at the bucket poses
void launch_ct_search(const GicpTarget& t, const glim_amd_ct_gicp_factor* f, const GicpArgs& a, const CtArgs& c, bool linearize, hipStream_t st) {
  with_search(t, [&](auto nn) {
    if (linearize) ct_gicp_kernel<true, decltype(nn)><<<f->nb, BLOCK, 0, st>>>(a, c, f->d_partials, nn);
    else ct_gicp_kernel<false, decltype(nn)><<<f->nb, BLOCK, 0, st>>>(a, c, f->d_partials, nn);
  });
}

// one synchronous evaluation; caller has validated the arguments.  out: CT_ROW doubles (CT_LINEARIZE) or the 29-double compact record (CT_ERROR)
int run_ct(glim_amd_ct_gicp_factor* f, const double* X, const double* Y, int mode, double* out, int32_t* corr_host) {
  const GicpTarget t = ct_target(f);
  if (!f->src->has_covs || !t.usable) return GLIM_AMD_ERR_STATE;
  GicpArgs a = t.args;
  set_source(&a, f->src, 1, f->max_dist);
  a.max_ring = t.rings(f->max_dist);
  if (a.max_ring < 0) return GLIM_AMD_ERR_UNSUPPORTED;
  glim_amd_ctx* ctx = f->ctx;
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  if (f->n == 0 || t.empty) {
    if (corr_host)
      for (int i = 0; i < f->n; i++) corr_host[i] = -1;
    return GLIM_AMD_OK;
  }
  ct_poses(f->table, X, Y, f->h_poses);
  // correspondences kept before an insert into the map (or a change of its neighbour mode) are positions in a map that is gone
  if (f->kept_gen != t.generation) f->kept = false;
  f->kept_gen = t.generation;
  CtArgs c{};
  c.blocks = f->d_blocks;
  c.poses = f->d_poses;
  if (mode != CT_CORR) {
    c.keep_corr = f->keep_corr;
    c.keep_m0 = f->keep_m0;
    c.keep_m1 = f->keep_m1;
  }
  DeviceTemp corr;
  SyncOnExit in_flight(st);
  GA_HIP(hipMemcpyAsync(f->d_poses, f->h_poses, (size_t)f->nbk * CT_POSE_STRIDE * sizeof(double), hipMemcpyHostToDevice, st));
  if (mode == CT_LINEARIZE) {
    f->kept = false;
    launch_ct_search(t, f, a, c, true, st);
    ct_bucket_kernel<<<f->nbk, 64, 0, st>>>(f->d_partials, f->d_bucket_first, f->d_poses, f->d_rows);
    ct_sum_kernel<<<1, 768, 0, st>>>(f->d_rows, f->nbk, f->d_out);
    GA_HIP(hipGetLastError());
    GA_HIP(read_back_sync(ctx, st, out, f->d_out, CT_ROW * sizeof(double)));
    f->kept = true;
  } else if (mode == CT_ERROR) {
    if (!f->kept) launch_ct_search(t, f, a, c, false, st);
    ct_error_kernel<<<f->nb, BLOCK, 0, st>>>(a, c, f->d_partials);
    gicp_finalize_kernel<<<1, 256, 0, st>>>(f->d_partials, f->nb, 0, f->d_out);
    GA_HIP(hipGetLastError());
    GA_HIP(read_back_sync(ctx, st, out, f->d_out, COMPACT * sizeof(double)));
    f->kept = true;
  } else {
    GA_HIP(pool_malloc(&corr.p, (size_t)f->n * sizeof(int32_t)));
    c.corr_out = corr.as<int32_t>();
    launch_ct_search(t, f, a, c, false, st);
    GA_HIP(hipGetLastError());
    GA_HIP(hipMemcpyAsync(corr_host, corr.p, (size_t)f->n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GA_HIP(hipStreamSynchronize(st));
  }
  in_flight.dismiss();
  return GLIM_AMD_OK;
}

// the deskewed points into out64 (device, n double4) and, when out32 is set, their FP32 image; caller holds ctx->mu
int run_ct_deskew(glim_amd_ct_gicp_factor* f, const double* X, const double* Y, bool local, double4* out64, float4* out32, hipStream_t st) {
  std::vector<double> full((size_t)f->nbk * CT_POSE_STRIDE);
  ct_poses(f->table, X, Y, full.data());
  double T0i[12];
  se3_inverse(full.data(), T0i);
  for (int k = 0; k < f->nbk; k++) {
    double* dst = f->h_poses + 12 * (size_t)k;
    if (local) se3_compose(T0i, full.data() + (size_t)k * CT_POSE_STRIDE, dst);
    else memcpy(dst, full.data() + (size_t)k * CT_POSE_STRIDE, 12 * sizeof(double));
  }
  GA_HIP(hipMemcpyAsync(f->d_poses, f->h_poses, (size_t)f->nbk * 12 * sizeof(double), hipMemcpyHostToDevice, st));
  ct_deskew_kernel<<<grid_for(f->n), 256, 0, st>>>(f->n, f->src->pts64, f->src->pts, f->d_time_index, f->d_poses, out64, out32);
  GA_HIP(hipGetLastError());
  return GLIM_AMD_OK;
}
}  // namespace

extern "C" {

int glim_amd_nn_index_create(const glim_amd_cloud* target, double max_correspondence_distance_hint, glim_amd_nn_index** out) {
  if (!target || !out) return GLIM_AMD_ERR_INVALID;
  *out = nullptr;
  if (target->n > (int64_t)(1 << 28)) return GLIM_AMD_ERR_INVALID;
  glim_amd_ctx* ctx = target->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  const int n = (int)target->n;
  std::unique_ptr<glim_amd_nn_index, int (*)(glim_amd_nn_index*)> ix(new glim_amd_nn_index(), glim_amd_nn_index_destroy);
  ix->ctx = ctx;
  ix->cloud = target;
  ix->n = n;
  ix->h = 1.0;
  ix->mask = 0;
  const size_t nn = (size_t)std::max(n, 1);
  GA_HIP(pool_malloc(&ix->sorted, nn * sizeof(float4)));
  if (target->has_covs) {
    GA_HIP(pool_malloc(&ix->covA, nn * sizeof(float4)));
    GA_HIP(pool_malloc(&ix->covB, nn * sizeof(float2)));
  }
  if (n == 0) {
    GA_HIP(pool_malloc(&ix->keys, sizeof(u64)));
    GA_HIP(pool_malloc(&ix->runs, sizeof(int2)));
    GA_HIP(hipMemsetAsync(ix->keys, 0xff, sizeof(u64), st));
    GA_HIP(hipStreamSynchronize(st));
    *out = ix.release();
    return GLIM_AMD_OK;
  }
  DeviceTemp vkey, bb, ka, kb, va, vb, hist;
  // (declared after the index object too: an error exit waits for the stream before scratch AND the half-built index are released)
  SyncOnExit in_flight(st);
  GA_HIP(pool_malloc(&vkey.p, nn * sizeof(u64)));
  GA_HIP(pool_malloc(&bb.p, 6 * sizeof(int)));
  GA_HIP(pool_malloc(&ka.p, nn * sizeof(u64)));
  GA_HIP(pool_malloc(&kb.p, nn * sizeof(u64)));
  GA_HIP(pool_malloc(&va.p, nn * sizeof(u32)));
  GA_HIP(pool_malloc(&vb.p, nn * sizeof(u32)));
  GA_HIP(pool_malloc(&hist.p, radix_sort_scratch_bytes(n)));
  const int blocks = std::max(1, std::min((n + 2047) / 2048, 128));
  int h_bb[6];
  // pass 1 with a provisional cell edge to learn the extent, then the edge that gives ~3 points per occupied cell of a surface-like
  // cloud, clamped to [R / 3, R] (R = the correspondence radius hint): at most 4 rings are ever scanned
  const double R = max_correspondence_distance_hint > 0.0 ? max_correspondence_distance_hint : 1.0;
  double h = R;
  for (int pass = 0; pass < 2; pass++) {
    init_bbox_kernel<<<1, 64, 0, st>>>(bb.as<int>());
    gi_key_kernel<<<blocks, 256, 0, st>>>(n, target->pts, 1.0 / h, vkey.as<u64>(), bb.as<int>());
    GA_HIP(hipGetLastError());
    GA_HIP(read_back_sync(ctx, st, h_bb, bb.p, sizeof(h_bb)));
    if (pass == 1 || h_bb[0] > h_bb[3]) break;
    const double ex = (h_bb[3] - h_bb[0] + 1) * h, ey = (h_bb[4] - h_bb[1] + 1) * h, ez = (h_bb[5] - h_bb[2] + 1) * h;
    const double area = ex * ey + ey * ez + ex * ez;
    const double h_density = std::sqrt(3.0 * 2.0 * area / (double)n);
    const double h_new = std::min(R, std::max(R / 3.0, h_density));
    if (h_new == h) break;
    h = h_new;
  }
  ix->h = h;
  int bx = 0, by = 0, bz = 0;
  if (h_bb[0] <= h_bb[3]) {
    bx = bits_for(h_bb[3] - h_bb[0]);
    by = bits_for(h_bb[4] - h_bb[1]);
    bz = bits_for(h_bb[5] - h_bb[2]);
  } else {
    h_bb[0] = h_bb[1] = h_bb[2] = 0;
  }
  const int vbits = bx + by + bz;
  gi_compact_key_kernel<<<grid_for(n), 256, 0, st>>>(n, vkey.as<u64>(), h_bb[0], h_bb[1], h_bb[2], bx, by, vbits, ka.as<u64>());
  u64* ks = nullptr;
  u32* vs = nullptr;
  GA_HIP(radix_sort_pairs(st, n, vbits + 1, ka.as<u64>(), va.as<u32>(), kb.as<u64>(), vb.as<u32>(), true, hist.as<int>(), &ks, &vs));
  const unsigned int T = next_pow2((unsigned long long)n * 2);
  ix->mask = T - 1;
  GA_HIP(pool_malloc(&ix->keys, (size_t)T * sizeof(u64)));
  GA_HIP(pool_malloc(&ix->runs, (size_t)T * sizeof(int2)));
  GA_HIP(hipMemsetAsync(ix->keys, 0xff, (size_t)T * sizeof(u64), st));
  gi_gather_kernel<<<grid_for(n), 256, 0, st>>>(n, ks, vs, 1ull << vbits, vkey.as<u64>(), target->pts, target->has_covs ? target->covA : nullptr,
                                                target->has_covs ? target->covB : nullptr, ix->sorted, ix->covA, ix->covB, ix->keys, ix->runs, ix->mask);
  GA_HIP(hipGetLastError());
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  *out = ix.release();
  return GLIM_AMD_OK;
}

int glim_amd_nn_index_destroy(glim_amd_nn_index* ix) {
  if (!ix) return GLIM_AMD_OK;
  if (ix->ctx) (void)hipSetDevice(ix->ctx->device);
  if (ix->keys) (void)pool_free(ix->keys);
  if (ix->runs) (void)pool_free(ix->runs);
  if (ix->sorted) (void)pool_free(ix->sorted);
  if (ix->covA) (void)pool_free(ix->covA);
  if (ix->covB) (void)pool_free(ix->covB);
  delete ix;
  return GLIM_AMD_OK;
}

int glim_amd_gicp_linearize(const glim_amd_nn_index* target, const glim_amd_cloud* source, const double* T_target_source12,
                            double max_correspondence_distance, uint32_t flags, glim_amd_linearized6* out) {
  return gicp_linearize(gicp_target(target), source, T_target_source12, max_correspondence_distance, flags, out);
}

int glim_amd_gicp_error(const glim_amd_nn_index* target, const glim_amd_cloud* source, const double* T_target_source12,
                        double max_correspondence_distance, double* error, int64_t* num_inliers) {
  return gicp_error(gicp_target(target), source, T_target_source12, max_correspondence_distance, error, num_inliers);
}

int glim_amd_gicp_correspondences(const glim_amd_nn_index* target, const glim_amd_cloud* source, const double* T_target_source12,
                                  double max_correspondence_distance, int32_t* correspondences) {
  if (!correspondences) return GLIM_AMD_ERR_INVALID;
  double compact[COMPACT];
  // the correspondences are the search's alone: clouds without covariances (the ICP factors' case) get them through the point-to-point kernel
  const GicpTarget t = gicp_target(target);
  const bool covs = source && source->has_covs && t.usable;
  return run_gicp(t, source, T_target_source12, max_correspondence_distance, false, compact, correspondences, covs ? Metric::GICP : Metric::ICP_POINT);
}

// IntegratedICPFactor / IntegratedPointToPlaneICPFactor over the GICP factor's search index
int glim_amd_icp_linearize(const glim_amd_nn_index* target, const glim_amd_cloud* source, const double* T_target_source12,
                           double max_correspondence_distance, uint32_t flags, glim_amd_linearized6* out) {
  if (flags & ~(uint32_t)(GLIM_AMD_FACTOR_BINARY | GLIM_AMD_ICP_POINT_TO_PLANE)) return GLIM_AMD_ERR_INVALID;
  return gicp_linearize(gicp_target(target), source, T_target_source12, max_correspondence_distance, flags & GLIM_AMD_FACTOR_BINARY, out, icp_metric(flags));
}

int glim_amd_icp_error(const glim_amd_nn_index* target, const glim_amd_cloud* source, const double* T_target_source12,
                       double max_correspondence_distance, uint32_t flags, double* error, int64_t* num_inliers) {
  if (flags & ~(uint32_t)(GLIM_AMD_FACTOR_BINARY | GLIM_AMD_ICP_POINT_TO_PLANE)) return GLIM_AMD_ERR_INVALID;
  return gicp_error(gicp_target(target), source, T_target_source12, max_correspondence_distance, error, num_inliers, icp_metric(flags));
}

// IntegratedGICPFactor_<iVox, PointCloud>: the rigid factor over the map
int glim_amd_ivox_gicp_linearize(const glim_amd_ivox* target, const glim_amd_cloud* source, const double* T_target_source12,
                                 double max_correspondence_distance, uint32_t flags, glim_amd_linearized6* out) {
  return gicp_linearize(gicp_target(target), source, T_target_source12, max_correspondence_distance, flags, out);
}

int glim_amd_ivox_gicp_error(const glim_amd_ivox* target, const glim_amd_cloud* source, const double* T_target_source12,
                             double max_correspondence_distance, double* error, int64_t* num_inliers) {
  return gicp_error(gicp_target(target), source, T_target_source12, max_correspondence_distance, error, num_inliers);
}

int glim_amd_ivox_gicp_correspondences(const glim_amd_ivox* target, const glim_amd_cloud* source, const double* T_target_source12,
                                       double max_correspondence_distance, int64_t* correspondences) {
  if (!correspondences || !source) return GLIM_AMD_ERR_INVALID;
  // the kernels write 32-bit positions; this entry point owns the 64-bit buffer and widens (a longer source is refused by run_gicp)
  std::vector<int32_t> corr32((size_t)std::min<int64_t>(source->n, IVOX_MAX_SOURCE));
  double compact[COMPACT];
  GA_TRY(run_gicp(gicp_target(target), source, T_target_source12, max_correspondence_distance, false, compact, corr32.data()));
  std::copy(corr32.begin(), corr32.end(), correspondences);
  return GLIM_AMD_OK;
}

}  // extern "C"

// ---- continuous-time GICP factor (IntegratedCT_GICPFactor_<PointCloud, PointCloud>) ----
extern "C" {

int glim_amd_ct_gicp_destroy(glim_amd_ct_gicp_factor* f) {
  if (!f) return GLIM_AMD_OK;
  if (f->ctx) (void)hipSetDevice(f->ctx->device);
  void* dev[] = {f->d_blocks, f->d_bucket_first, f->d_time_index, f->d_table, f->d_poses, f->d_partials, f->d_rows, f->d_out, f->keep_corr, f->keep_m0, f->keep_m1};
  for (void* p : dev)
    if (p) (void)pool_free(p);
  if (f->h_poses) (void)pinned_free(f->h_poses);
  if (f->iv) f->iv->live_factors--;
  delete f;
  return GLIM_AMD_OK;
}

}  // extern "C"

namespace {
// the factor over either target kind: exactly one of `target` / `map` is set, `ctx` is its context
int ct_factor_create(glim_amd_ctx* ctx, const glim_amd_nn_index* target, glim_amd_ivox* map, const glim_amd_cloud* source, const double* times,
                     glim_amd_ct_gicp_factor** out) {
  if (!source || !out) return GLIM_AMD_ERR_INVALID;
  *out = nullptr;
  if (source->ctx->device != ctx->device) return GLIM_AMD_ERR_INVALID;
  if (source->n > (int64_t)(1 << 28)) return GLIM_AMD_ERR_INVALID;
  const int n = (int)source->n;
  if (!times && (int64_t)source->h_times.size() != source->n) return GLIM_AMD_ERR_STATE;  // no per-point times
  if (!source->has_covs) return GLIM_AMD_ERR_STATE;
  const double* t = times ? times : source->h_times.data();
  std::unique_ptr<glim_amd_ct_gicp_factor, int (*)(glim_amd_ct_gicp_factor*)> f(new glim_amd_ct_gicp_factor(), glim_amd_ct_gicp_destroy);
  f->ctx = ctx;
  f->ix = target;
  if (map) {
    f->iv = map;
    map->live_factors++;
  }
  f->src = source;
  f->n = n;
  // the time table (IntegratedCT_ICPFactor's constructor): a new bucket when the time moves on by more than 1e-3, entries / the last one
  f->time_index.resize((size_t)n);
  for (int i = 0; i < n; i++) {
    if (f->table.empty() || t[i] - f->table.back() > 1e-3) f->table.push_back(t[i]);
    f->time_index[i] = (int)f->table.size() - 1;
  }
  if (!f->table.empty()) {
    const double last = std::max(1e-9, f->table.back());
    for (double& v : f->table) v /= last;
  }
  f->nbk = (int)f->table.size();
  // blocks: each bucket's index run cut into pieces of BLOCK * ppt points (ppt as run_gicp picks it for the whole cloud)
  const int ppt = points_per_thread(ctx, n);
  std::vector<int4> blocks;
  std::vector<int> first((size_t)f->nbk + 1, 0);
  for (int i = 0; i < n;) {
    const int k = f->time_index[i];
    int e = i;
    while (e < n && f->time_index[e] == k) e++;
    first[k] = (int)blocks.size();
    for (int b = i; b < e; b += BLOCK * ppt) blocks.push_back(make_int4(k, b, std::min(e, b + BLOCK * ppt), 0));
    i = e;
  }
  f->nb = (int)blocks.size();
  first[f->nbk] = f->nb;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  const size_t nn = (size_t)std::max(n, 1), nk = (size_t)std::max(f->nbk, 1), nbb = (size_t)std::max(f->nb, 1);
  GA_HIP(pool_malloc(&f->d_blocks, nbb * sizeof(int4)));
  GA_HIP(pool_malloc(&f->d_bucket_first, (nk + 1) * sizeof(int)));
  GA_HIP(pool_malloc(&f->d_time_index, nn * sizeof(int)));
  GA_HIP(pool_malloc(&f->d_table, nk * sizeof(double)));
  GA_HIP(pool_malloc(&f->d_poses, nk * CT_POSE_STRIDE * sizeof(double)));
  GA_HIP(pinned_malloc(&f->h_poses, nk * CT_POSE_STRIDE * sizeof(double)));
  GA_HIP(pool_malloc(&f->d_partials, nbb * PARTIAL_STRIDE * sizeof(float)));
  GA_HIP(pool_malloc(&f->d_rows, nk * CT_ROW * sizeof(double)));
  GA_HIP(pool_malloc(&f->d_out, CT_ROW * sizeof(double)));
  GA_HIP(pool_malloc(&f->keep_corr, nn * sizeof(int32_t)));
  GA_HIP(pool_malloc(&f->keep_m0, nn * sizeof(float4)));
  GA_HIP(pool_malloc(&f->keep_m1, nn * sizeof(float2)));
  if (n > 0) {
    SyncOnExit in_flight(st);
    GA_HIP(hipMemcpyAsync(f->d_blocks, blocks.data(), blocks.size() * sizeof(int4), hipMemcpyHostToDevice, st));
    GA_HIP(hipMemcpyAsync(f->d_bucket_first, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice, st));
    GA_HIP(hipMemcpyAsync(f->d_time_index, f->time_index.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    GA_HIP(hipMemcpyAsync(f->d_table, f->table.data(), (size_t)f->nbk * sizeof(double), hipMemcpyHostToDevice, st));
    GA_HIP(hipStreamSynchronize(st));
    in_flight.dismiss();
  }
  *out = f.release();
  return GLIM_AMD_OK;
}
}  // namespace

extern "C" {

int glim_amd_ct_gicp_create(const glim_amd_nn_index* target, const glim_amd_cloud* source, const double* times, glim_amd_ct_gicp_factor** out) {
  if (!target) return GLIM_AMD_ERR_INVALID;
  return ct_factor_create(target->ctx, target, nullptr, source, times, out);
}

int glim_amd_ivox_ct_factor_create(glim_amd_ivox* target, const glim_amd_cloud* source, const double* times, glim_amd_ct_gicp_factor** out) {
  if (!target) return GLIM_AMD_ERR_INVALID;
  return ct_factor_create(target->ctx, nullptr, target, source, times, out);
}

int glim_amd_ct_gicp_set_max_correspondence_distance(glim_amd_ct_gicp_factor* f, double d) {
  if (!f || !(d >= 0.0)) return GLIM_AMD_ERR_INVALID;
  const GicpTarget t = ct_target(f);
  if (t.rings(d) < 0) return GLIM_AMD_ERR_UNSUPPORTED;
  f->max_dist = d;
  f->kept = false;
  return GLIM_AMD_OK;
}

int glim_amd_ct_gicp_linearize(glim_amd_ct_gicp_factor* f, const double* X12, const double* Y12, glim_amd_ct_linearized* out) {
  if (!f || !X12 || !Y12 || !out) return GLIM_AMD_ERR_INVALID;
  double rec[CT_ROW] = {};
  GA_TRY(run_ct(f, X12, Y12, CT_LINEARIZE, rec, nullptr));
  ct_expand_record(rec, out);
  return GLIM_AMD_OK;
}

int glim_amd_ct_gicp_error(glim_amd_ct_gicp_factor* f, const double* X12, const double* Y12, double* error, int64_t* num_inliers) {
  if (!f || !X12 || !Y12 || !error) return GLIM_AMD_ERR_INVALID;
  double rec[COMPACT] = {};
  GA_TRY(run_ct(f, X12, Y12, CT_ERROR, rec, nullptr));
  *error = rec[1];
  if (num_inliers) *num_inliers = (int64_t)llround(rec[0]);
  return GLIM_AMD_OK;
}

int glim_amd_ct_gicp_correspondences(glim_amd_ct_gicp_factor* f, const double* X12, const double* Y12, int32_t* correspondences) {
  if (!f || !X12 || !Y12 || (!correspondences && f->n > 0)) return GLIM_AMD_ERR_INVALID;
  return run_ct(f, X12, Y12, CT_CORR, nullptr, correspondences);
}

int glim_amd_ct_gicp_deskewed_points(glim_amd_ct_gicp_factor* f, const double* X12, const double* Y12, int32_t local, double* points4) {
  if (!f || !X12 || !Y12 || (!points4 && f->n > 0)) return GLIM_AMD_ERR_INVALID;
  if (f->n == 0) return GLIM_AMD_OK;
  glim_amd_ctx* ctx = f->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  DeviceTemp d;
  SyncOnExit in_flight(st);
  GA_HIP(pool_malloc(&d.p, (size_t)f->n * sizeof(double4)));
  GA_TRY(run_ct_deskew(f, X12, Y12, local != 0, d.as<double4>(), nullptr, st));
  GA_HIP(hipMemcpyAsync(points4, d.p, (size_t)f->n * sizeof(double4), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  return GLIM_AMD_OK;
}

int glim_amd_ct_gicp_deskewed_cloud(glim_amd_ct_gicp_factor* f, const double* X12, const double* Y12, int32_t local, glim_amd_cloud** out) {
  if (!f || !X12 || !Y12 || !out) return GLIM_AMD_ERR_INVALID;
  *out = nullptr;
  const glim_amd_cloud* src = f->src;
  glim_amd_ctx* ctx = f->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  std::unique_ptr<glim_amd_cloud, int (*)(glim_amd_cloud*)> c(new glim_amd_cloud(), glim_amd_cloud_destroy);
  c->ctx = static_cast<glim_amd_ctx*>(src->ctx);
  c->n = f->n;
  const size_t nn = (size_t)std::max(f->n, 1);
  GA_HIP(pool_malloc(&c->pts, nn * sizeof(float4)));
  GA_HIP(pool_malloc(&c->pts64, nn * sizeof(double4)));
  if (f->n > 0) {
    SyncOnExit in_flight(st);
    GA_TRY(run_ct_deskew(f, X12, Y12, local != 0, c->pts64, c->pts, st));
    if (src->neighbors && src->k > 0) {
      // the source's neighbour lists travel with the points (odometry_estimation_ct.cpp:194-195 estimates covariances from them)
      GA_HIP(pool_malloc(&c->neighbors, (size_t)f->n * src->k * sizeof(int32_t)));
      GA_HIP(hipMemcpyAsync(c->neighbors, src->neighbors, (size_t)f->n * src->k * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
      c->k = src->k;
    }
    GA_HIP(hipStreamSynchronize(st));
    in_flight.dismiss();
  }
  *out = c.release();
  return GLIM_AMD_OK;
}

int glim_amd_debug_ct_gicp_poses(const glim_amd_ct_gicp_factor* f, const double* X12, const double* Y12, int32_t* num_buckets, int32_t table_cap,
                                 double* table_out, double* T12_out, double* D0_out, double* D1_out, int32_t* time_index_out) {
  if (!f || !X12 || !Y12 || table_cap < 0) return GLIM_AMD_ERR_INVALID;
  if (num_buckets) *num_buckets = f->nbk;
  std::vector<double> full((size_t)f->nbk * CT_POSE_STRIDE);
  ct_poses(f->table, X12, Y12, full.data());
  const int m = std::min(table_cap, f->nbk);
  for (int k = 0; k < m; k++) {
    const double* o = full.data() + (size_t)k * CT_POSE_STRIDE;
    if (table_out) table_out[k] = f->table[k];
    if (T12_out) memcpy(T12_out + 12 * (size_t)k, o, 12 * sizeof(double));
    if (D0_out) memcpy(D0_out + 36 * (size_t)k, o + 12, 36 * sizeof(double));
    if (D1_out) memcpy(D1_out + 36 * (size_t)k, o + 48, 36 * sizeof(double));
  }
  if (time_index_out) memcpy(time_index_out, f->time_index.data(), f->time_index.size() * sizeof(int32_t));
  return GLIM_AMD_OK;
}

}  // extern "C"
