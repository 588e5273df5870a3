// ct_factor.hpp -- the continuous-time GICP factor as the two units that run it see it (gicp.hip: the factor's own entry points; ct_align.hip:
// the CT frame alignment, which runs the factor's linearising pass inside its rounds): the factor object, the arguments and the bodies of its
// search pass, bucket pass and ordered sum, the record's layout and its expansion.  Each of them is defined here, once; like gicp_factor.hpp the
// shared part is in an unnamed namespace and nothing of it is called across units.
//
// Layout: the points of a bucket are a contiguous index run (the time table never goes back), cut into blocks of at most BLOCK * ppt points, so
// the pose is uniform per block.  Block b writes its 28 source-frame sums (in T_k's own tangent) to partial row b; the bucket pass adds the rows
// of each bucket in block order and maps the bucket's 6 x 6 system through the chain rule [D0_k | D1_k] in FP64; the sum adds the buckets in
// bucket order.  No atomics: the record is bit-reproducible, for any number of buckets.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "ct_se3.hpp"
#include "gicp_factor.hpp"
#include "ivox_map.hpp"

struct glim_amd_ct_gicp_factor {
  CtxRef ctx;
  const glim_amd_nn_index* ix = nullptr;  // not owned; null when the target is a device iVox
  glim_amd_ivox* iv = nullptr;            // not owned (counted in its live_factors: the map cannot be destroyed under the factor)
  uint64_t kept_gen = 0;                  // the map's generation the kept correspondences were found in
  const glim_amd_cloud* src = nullptr;    // not owned
  int n = 0;
  double max_dist = 1.0;
  std::vector<double> table;              // normalised bucket times
  std::vector<int> time_index;            // bucket of every point
  int nbk = 0, nb = 0;                    // buckets, blocks
  int4* d_blocks = nullptr;               // (bucket, begin, end, -) per block
  int* d_bucket_first = nullptr;          // first block of every bucket, nbk + 1 entries
  int* d_time_index = nullptr;
  double* d_table = nullptr;              // `table` on the device (the pose table kernel of the CT frame alignment reads it)
  double* d_poses = nullptr;              // CT_POSE_STRIDE per bucket
  double* h_poses = nullptr;              // pinned staging of the same
  float* d_partials = nullptr;            // nb partial rows
  double* d_rows = nullptr;               // nbk bucket rows
  double* d_out = nullptr;                // CT_ROW doubles
  int32_t* keep_corr = nullptr;           // the state linearize keeps for error
  float4* keep_m0 = nullptr;
  float2* keep_m1 = nullptr;
  bool kept = false;
};

namespace {

using glim_amd::ct_se3::CT_POSE_STRIDE;
constexpr int CT_ROW = 92;  // doubles per bucket row / in the record: count, error, 78 upper entries of the 12 x 12 H (row-major), 12 of b

// row-major upper triangle of a symmetric N x N matrix: entry (r, c), r <= c, is at upper_index<N>(r, c); upper_entry<N> is the way back
template <int N>
constexpr int upper_index(int r, int c) {
  return r * N - r * (r - 1) / 2 + (c - r);
}
template <int N>
constexpr void upper_entry(int u, int& r, int& c) {
  for (r = 0; u >= N - r; r++) u -= N - r;
  c = r + u;
}

struct CtArgs {
  const int4* blocks;    // (bucket, begin, end, -) per block
  const double* poses;   // CT_POSE_STRIDE per bucket (the deskewing kernel reads a plain 12-double table instead)
  int32_t* keep_corr;    // kept correspondences (position in the index's sorted order, or -1), or null
  float4* keep_m0;       // kept M = (C_B + R_k C_A R_k^T)^-1 (target frame): m00 m01 m02 m11
  float2* keep_m1;       //                                                      m12 m22
  int32_t* corr_out;     // original target index or -1 per source point, or null
};

// the search pass of one block (BLOCK threads): the points of block blockIdx.x at the pose of its bucket -> partial row blockIdx.x
template <bool LINEARIZE, class NN>
__device__ __forceinline__ void ct_gicp_block(const GicpArgs& a, const CtArgs& c, float* __restrict__ partials, const NN& nn,
                                              float (&s_red)[4][PARTIAL_STRIDE]) {
  const int4 blk = c.blocks[blockIdx.x];
  const double* T = c.poses + (size_t)blk.x * CT_POSE_STRIDE;
  const Rot32 R(T);
  float acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; j++) acc[j] = 0.f;
  int inliers = 0;
  for (int i = blk.y + (int)threadIdx.x; i < blk.z; i += BLOCK) {
    const float4 p = a.pts[i];
    double qx, qy, qz;
    transform_point_d(T, (double)p.x, (double)p.y, (double)p.z, qx, qy, qz);
    double best_d;
    const int j = nn.find(a, qx, qy, qz, best_d);
    if (c.corr_out) c.corr_out[i] = j >= 0 ? __float_as_int(a.sorted[j].w) : -1;
    if (c.keep_corr) c.keep_corr[i] = j;
    if (j < 0) continue;
    inliers++;
    float A[6];
    gicp_point<LINEARIZE>(acc, R.r00, R.r01, R.r02, R.r10, R.r11, R.r12, R.r20, R.r21, R.r22, p, a.sorted[j], a.tA[j], a.tB[j], a.covA[i], a.covB[i], qx, qy, qz,
                          A);
    if (c.keep_m0) {
      // M = R A R^T: the source-frame inverse taken back to the target frame
      const float Rm[9] = {R.r00, R.r01, R.r02, R.r10, R.r11, R.r12, R.r20, R.r21, R.r22};
      const float As[9] = {A[0], A[1], A[2], A[1], A[3], A[4], A[2], A[4], A[5]};
      float W[9];
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) W[3 * r + k] = Rm[3 * r] * As[k] + Rm[3 * r + 1] * As[3 + k] + Rm[3 * r + 2] * As[6 + k];
      float M[6];
      const int mr[6] = {0, 0, 0, 1, 1, 2}, mc[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
      for (int u = 0; u < 6; u++) M[u] = W[3 * mr[u]] * Rm[3 * mc[u]] + W[3 * mr[u] + 1] * Rm[3 * mc[u] + 1] + W[3 * mr[u] + 2] * Rm[3 * mc[u] + 2];
      c.keep_m0[i] = make_float4(M[0], M[1], M[2], M[3]);
      c.keep_m1[i] = make_float2(M[4], M[5]);
    }
  }
  store_partial_row(acc, inliers, s_red, partials);
}

// the LDS of the bucket pass
struct CtBucketShared {
  double sum[PARTIAL_STRIDE];
  double J[6 * 12];
  double H[36];
  double b[6];
  double W[6 * 12];
};

// the bucket pass of one block of 64 threads, bucket blockIdx.x: its partial rows summed in FP64 in block order -> H_k, b_k (T_k's tangent, the
// compact record's convention) -> [D0 | D1]^T H_k [D0 | D1] and [D0 | D1]^T b_k
__device__ __forceinline__ void ct_bucket_block(const float* __restrict__ partials, const int* __restrict__ bucket_first, const double* __restrict__ poses,
                                                double* __restrict__ rows, CtBucketShared& s) {
  const int k = blockIdx.x, t = threadIdx.x;
  const int first = bucket_first[k], last = bucket_first[k + 1];
  if (t <= 28) {
    double v = 0.0;
    for (int r = first; r < last; r++) v += (double)partials[(size_t)r * PARTIAL_STRIDE + t];
    s.sum[t] = v;
  }
  const double* D = poses + (size_t)k * CT_POSE_STRIDE + 12;
  for (int u = t; u < 72; u += 64) {
    const int m = u / 12, col = u % 12;
    s.J[u] = col < 6 ? D[6 * m + col] : D[36 + 6 * m + col - 6];
  }
  __syncthreads();
  if (t < 36) {
    const int r = t / 6, cc = t % 6;
    s.H[t] = s.sum[c_acc_of_upper_g[upper_index<6>(min(r, cc), max(r, cc))]];
  } else if (t < 42) {
    const int m = t - 36;
    s.b[m] = m < 3 ? s.sum[21 + m] : -s.sum[21 + m];
  }
  __syncthreads();
  for (int u = t; u < 72; u += 64) {
    const int m = u / 12, col = u % 12;
    double v = 0.0;
    for (int q = 0; q < 6; q++) v += s.H[6 * m + q] * s.J[12 * q + col];
    s.W[u] = v;
  }
  __syncthreads();
  double* row = rows + (size_t)k * CT_ROW;
  for (int u = t; u < CT_ROW; u += 64) {
    double v;
    if (u == 0) {
      v = s.sum[28];
    } else if (u == 1) {
      v = s.sum[27];
    } else if (u < 80) {
      int r, cc;
      upper_entry<12>(u - 2, r, cc);
      v = 0.0;
      for (int m = 0; m < 6; m++) v += s.J[12 * m + r] * s.W[12 * m + cc];
    } else {
      const int r = u - 80;
      v = 0.0;
      for (int m = 0; m < 6; m++) v += s.J[12 * m + r] * s.b[m];
    }
    row[u] = v;
  }
}

// a block of THREADS threads (768 work items: 8 groups x 96 columns, each the same additions whatever THREADS is): the bucket rows summed in a
// fixed order (8 groups of ordered_column_sum, then the groups in order) -> the record, CT_ROW doubles at `out` (global or LDS; written by
// threads 0 .. CT_ROW - 1, no barrier behind the write)
constexpr int CT_SUM_THREADS = 768;
template <int THREADS>
__device__ __forceinline__ void ct_sum_rows(const double* __restrict__ rows, int nbk, double (&s_part)[8][96], double* out) {
  static_assert(THREADS >= CT_ROW && CT_SUM_THREADS % THREADS == 0, "whole passes over the 768 work items");
  for (int v = threadIdx.x; v < CT_SUM_THREADS; v += THREADS) {
    const int j = v % 96, g = v / 96;
    double s = 0.0;
    if (j < CT_ROW) s = ordered_column_sum<double, CT_ROW, 8>(rows, nbk, j, g);
    s_part[g][j] = s;
  }
  __syncthreads();
  if (threadIdx.x < CT_ROW) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < 8; q++) t += s_part[q][threadIdx.x];
    out[threadIdx.x] = t;
  }
}

// the record as the ABI hands it out
inline void ct_expand_record(const double* rec, glim_amd_ct_linearized* out) {
  memset(out, 0, sizeof(*out));
  out->num_inliers = (int64_t)llround(rec[0]);
  out->error = rec[1];
  double H[144];
  int u = 2;
  for (int r = 0; r < 12; r++)
    for (int c = r; c < 12; c++, u++) H[12 * r + c] = H[12 * c + r] = rec[u];
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) {
      out->H_00[6 * r + c] = H[12 * r + c];
      out->H_01[6 * r + c] = H[12 * r + c + 6];
      out->H_11[6 * r + c] = H[12 * (r + 6) + c + 6];
    }
  for (int r = 0; r < 6; r++) {
    out->b_0[r] = rec[80 + r];
    out->b_1[r] = rec[86 + r];
  }
}

// the factor's target as it is now (the lock of the call comes with it)
GicpTarget ct_target(const glim_amd_ct_gicp_factor* f) { return f->ix ? gicp_target(f->ix) : gicp_target(f->iv); }

}  // namespace
