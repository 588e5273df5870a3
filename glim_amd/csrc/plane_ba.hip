// plane_ba.hip -- device side of the reference's plane bundle-adjustment tool (bundle_adjustment_modal.cpp): ball selection over many
// sub-maps, its statistics, the radius search, and the plane / edge eigenvalue factors over per-frame moments (plane_ba.hpp).
// Semantics: include/glim_amd.h "Plane / edge bundle-adjustment factors and ball selection".
//
// Passes over points (one lane per point, 256-thread blocks, FP64):
//   ba_transform_kernel   q = R p + (t - c) and q.q of every point of every sub-map, kept as double4 (32 B per point)
//   ba_flag_kernel        q.q < r r  ->  0 / 1, then scan.hpp's exclusive prefix sum and ba_scatter_kernel: stable compaction
//   ba_stats_kernel       filtered ten-value reduction: count + 3 + 6 sums per block, by one fixed tree over the block's lanes
//   ba_stats_final_kernel ordered two-level pass over the block sums, covariance, eigenvalues, and -- in the radius search -- the decision
//   ba_moment_*           the factor's per-frame moments, the same two-step ordered sum per frame
// No pass over points after a factor exists: ba_lin_kernel (one block, one thread per frame) and ba_fill_kernel (one thread per H entry).
#include <algorithm>
#include <cmath>
#include <memory>

#include "device_math.hpp"
#include "internal.hpp"
#include "plane_ba.hpp"
#include "scan.hpp"
#include "scope_sync.hpp"

struct glim_amd_ba_factor {
  CtxRef ctx;
  int kind = 0;
  int K = 0;
  int64_t N = 0;
  std::vector<int32_t> kept;
  std::vector<double> moments;  // K x BA_MOM (host copy)
  double* d_moments = nullptr;  // K x BA_MOM
  double* d_poses = nullptr;    // K x 12
  double* d_ws = nullptr;       // ba_workspace_doubles(K)
  double* d_H = nullptr;        // 6 K x 6 K
};

namespace glim_amd {
namespace ba {

struct SubDesc {
  const double4* p64;
  const float4* p32;
  int n;
  int off;       // index of the sub-map's first point in the concatenation
  double T[12];  // rotation, and t - c in the translation column
};

constexpr int MAX_CLOUDS = 4096;
constexpr int ENTRY_DOUBLES = 6;  // device form of a trace entry: radius, count, three eigenvalues, decision
// device state of the radius search (doubles): [0] radius to evaluate  [1] active  [2] current radius  [3] current count  [4..6] current
// eigenvalues  [7] r0  [8] trials evaluated  [9] stop reason  [10] entries filled  [11] N  [12..14] s  [15..20] S  [21..23] eigenvalues of
// the LAST evaluation (the statistics call reads these); then 11 trace entries
constexpr int ST_TRACE = 24;
constexpr int ST_DOUBLES = ST_TRACE + (GLIM_AMD_BA_MAX_TRIALS + 1) * ENTRY_DOUBLES;

__device__ __forceinline__ int find_sub(const SubDesc* __restrict__ d, int S, int i) {
  int lo = 0, hi = S - 1;  // last sub-map whose offset is <= i (empty sub-maps share an offset with their successor: take the last)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].off <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ void load_point(const SubDesc& d, int j, double& x, double& y, double& z) {
  if (d.p64) {
    const double4 p = d.p64[j];
    x = p.x, y = p.y, z = p.z;
  } else {
    const float4 p = d.p32[j];
    x = (double)p.x, y = (double)p.y, z = (double)p.z;
  }
}

static __global__ __launch_bounds__(256) void ba_transform_kernel(const SubDesc* __restrict__ descs, int S, int total, double4* __restrict__ q4) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int s = find_sub(descs, S, i);
  const SubDesc& d = descs[s];
  double x, y, z;
  load_point(d, i - d.off, x, y, z);
  double4 q;
  q.x = dadd(dadd(dadd(dmul(d.T[0], x), dmul(d.T[1], y)), dmul(d.T[2], z)), d.T[3]);
  q.y = dadd(dadd(dadd(dmul(d.T[4], x), dmul(d.T[5], y)), dmul(d.T[6], z)), d.T[7]);
  q.z = dadd(dadd(dadd(dmul(d.T[8], x), dmul(d.T[9], y)), dmul(d.T[10], z)), d.T[11]);
  q.w = dadd(dadd(dmul(q.x, q.x), dmul(q.y, q.y)), dmul(q.z, q.z));
  q4[i] = q;
}

static __global__ __launch_bounds__(256) void ba_flag_kernel(const double4* __restrict__ q4, int total, double r2, int* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < total) flags[i] = q4[i].w < r2 ? 1 : 0;
}

// pairs[2 pos] = (sub-map, point) of the pos-th selected point, for pos < capacity
static __global__ __launch_bounds__(256) void ba_scatter_kernel(const int* __restrict__ flags, const int* __restrict__ pos, int total,
                                                                const SubDesc* __restrict__ descs, int S, int capacity, int* __restrict__ pairs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total || !flags[i]) return;
  const int p = pos[i];
  if (p >= capacity) return;
  const int s = find_sub(descs, S, i);
  pairs[2 * p] = s;
  pairs[2 * p + 1] = i - descs[s].off;
}

// sum of N values over the 256 lanes of a block by ONE fixed tree: lanes l and l + 32, + 16, ... + 1 inside a wavefront, then the four
// wavefronts in order.  Thread j < N returns value j's sum; s_tmp: 4 N doubles.
template <int N>
__device__ __forceinline__ double block_tree_sum(double (&v)[N], double* s_tmp) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
    for (int j = 0; j < N; j++) v[j] = dadd(v[j], __shfl_down(v[j], off, 64));
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int j = 0; j < N; j++) s_tmp[wave * N + j] = v[j];
  __syncthreads();
  double r = 0.0;
  if ((int)threadIdx.x < N) r = dadd(dadd(dadd(s_tmp[threadIdx.x], s_tmp[N + threadIdx.x]), s_tmp[2 * N + threadIdx.x]), s_tmp[3 * N + threadIdx.x]);
  __syncthreads();
  return r;
}

// partials[10 b + 0] = the block's count, [1..3] sum q, [4..9] sum q q^T.  state != null: the radius is state[0] and an idle search does nothing.
static __global__ __launch_bounds__(256) void ba_stats_kernel(const double4* __restrict__ q4, int total, double radius, const double* __restrict__ state,
                                                              double* __restrict__ partials) {
  __shared__ double s_tmp[40];
  if (state) {
    if (state[1] == 0.0) return;
    radius = state[0];
  }
  const double r2 = dmul(radius, radius);
  const int i = blockIdx.x * 256 + threadIdx.x;
  double v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (i < total) {
    const double4 q = q4[i];
    if (q.w < r2) {
      v[0] = 1.0;
      v[1] = q.x, v[2] = q.y, v[3] = q.z;
      v[4] = dmul(q.x, q.x), v[5] = dmul(q.x, q.y), v[6] = dmul(q.x, q.z);
      v[7] = dmul(q.y, q.y), v[8] = dmul(q.y, q.z), v[9] = dmul(q.z, q.z);
    }
  }
  const double r = block_tree_sum<10>(v, s_tmp);
  if (threadIdx.x < 10) partials[10 * (size_t)blockIdx.x + threadIdx.x] = r;
}

__device__ __forceinline__ void put_entry(double* state, int i, double radius, double count, const double* lam, double decision) {
  double* e = state + ST_TRACE + ENTRY_DOUBLES * i;
  e[0] = radius;
  e[1] = count;
  e[2] = lam[0], e[3] = lam[1], e[4] = lam[2];
  e[5] = decision;
}

// ordered pass over the block sums in two levels, then thread 0: covariance, eigenvalues and, with round >= 0, the search's decision.
// The blocks are cut into 64 runs of ceil(nblocks / 64) consecutive blocks; thread (value j, run c) adds run c's sums of value j by ascending
// block, then one thread per value adds the 64 run sums by ascending run.  round < 0: statistics only.
constexpr int FINAL_RUNS = 64;
static __global__ __launch_bounds__(10 * FINAL_RUNS) void ba_stats_final_kernel(const double* __restrict__ partials, int nblocks, double* __restrict__ state,
                                                                                int round, double min_radius, double max_radius, double plane_eps) {
  __shared__ double s_run[10][FINAL_RUNS];
  __shared__ double s_sum[10];
  if (round >= 0 && state[1] == 0.0) return;
  {
    const int j = threadIdx.x / FINAL_RUNS, c = threadIdx.x % FINAL_RUNS;
    const int per = (nblocks + FINAL_RUNS - 1) / FINAL_RUNS;
    const int b0 = c * per, b1 = min(nblocks, b0 + per);
    double a = 0.0;
    for (int b = b0; b < b1; b++) a = dadd(a, partials[10 * (size_t)b + j]);
    s_run[j][c] = a;
  }
  __syncthreads();
  if (threadIdx.x < 10) {
    double a = 0.0;
    for (int c = 0; c < FINAL_RUNS; c++) a = dadd(a, s_run[threadIdx.x][c]);
    s_sum[threadIdx.x] = a;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double N = s_sum[0];
  double lam[3];
  {
#pragma clang fp contract(off)
    // mean = s / N, cov = (S - mean s^T) / N  (bundle_adjustment_modal.cpp:177-178)
    double mean[3], C[9], U[9];
    for (int a = 0; a < 3; a++) mean[a] = s_sum[1 + a] / N;
    const int idx[3][3] = {{4, 5, 6}, {5, 7, 8}, {6, 8, 9}};
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) C[3 * a + b] = (s_sum[idx[a][b]] - mean[a] * s_sum[1 + b]) / N;
    eig3::direct(C, lam, U);
  }
  for (int j = 0; j < 10; j++) state[11 + j] = s_sum[j];
  for (int j = 0; j < 3; j++) state[21 + j] = lam[j];
  if (round < 0) return;
  const double r0 = state[7];
  bool active = true;
  if (round == 0) {
    state[2] = r0, state[3] = N, state[4] = lam[0], state[5] = lam[1], state[6] = lam[2];
    put_entry(state, 0, r0, N, lam, (double)GLIM_AMD_BA_TRACE_INITIAL);
    state[10] = 1.0;
  } else {
    const double trial = state[0];
    state[8] = (double)round;
    state[10] = (double)(round + 1);
    if (N < 10.0) {
      put_entry(state, round, trial, N, lam, (double)GLIM_AMD_BA_TRACE_FEW_POINTS);
      state[9] = (double)GLIM_AMD_BA_STOP_FEW_POINTS;
      active = false;
    } else if (trial > r0 && lam[0] / lam[2] > plane_eps) {
      put_entry(state, round, trial, N, lam, (double)GLIM_AMD_BA_TRACE_PLANE_EPS);
      state[9] = (double)GLIM_AMD_BA_STOP_PLANE_EPS;
      active = false;
    } else {
      put_entry(state, round, trial, N, lam, (double)GLIM_AMD_BA_TRACE_TAKEN);
      state[2] = trial, state[3] = N, state[4] = lam[0], state[5] = lam[1], state[6] = lam[2];
    }
  }
  if (active) {
    if (round == GLIM_AMD_BA_MAX_TRIALS) {
      state[9] = (double)GLIM_AMD_BA_STOP_TRIALS;
      active = false;
    } else {
      const double cur = state[2];
      const double next = (state[4] / state[6] > plane_eps) ? dmul(cur, 0.8) : dmul(cur, 1.1);
      if (next < min_radius || next > max_radius) {
        const double nan3[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
        put_entry(state, round + 1, next, -1.0, nan3, (double)GLIM_AMD_BA_TRACE_RANGE);
        state[10] = (double)(round + 2);
        state[9] = (double)GLIM_AMD_BA_STOP_RANGE;
        active = false;
      } else {
        state[0] = next;
      }
    }
  }
  state[1] = active ? 1.0 : 0.0;
}

// out[s] = pos[off_s] for s < S, out[S] = pos[total]: the rank of every sub-map's first selected point, and the count
static __global__ void ba_offsets_kernel(const int* __restrict__ pos, const SubDesc* __restrict__ descs, int S, int total, int* __restrict__ out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < S) out[s] = pos[descs[s].off];
  else if (s == S) out[S] = pos[total];
}

// P3[3 i ..] = the frame-local coordinates of the i-th selected point
static __global__ __launch_bounds__(256) void ba_gather_local_kernel(const int* __restrict__ pairs, int N, const SubDesc* __restrict__ descs,
                                                                     double* __restrict__ P3) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double x, y, z;
  load_point(descs[pairs[2 * i]], pairs[2 * i + 1], x, y, z);
  P3[3 * (size_t)i] = x, P3[3 * (size_t)i + 1] = y, P3[3 * (size_t)i + 2] = z;
}

// frames[f] = (first point, count, first block, blocks); blockmap[b] = (frame, chunk).  partial[9 b ..]: sum (p - c), sum (p - c)(p - c)^T
static __global__ __launch_bounds__(256) void ba_moment_partial_kernel(const double* __restrict__ P3, const int4* __restrict__ frames,
                                                                       const int2* __restrict__ blockmap, double* __restrict__ partial) {
  __shared__ double s_tmp[36];
  const int2 bm = blockmap[blockIdx.x];
  const int4 fr = frames[bm.x];
  const int j = bm.y * 256 + (int)threadIdx.x;
  double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (j < fr.y) {
    const double* c = P3 + 3 * (size_t)fr.x;
    const double* p = P3 + 3 * (size_t)(fr.x + j);
    const double dx = dadd(p[0], -c[0]), dy = dadd(p[1], -c[1]), dz = dadd(p[2], -c[2]);
    v[0] = dx, v[1] = dy, v[2] = dz;
    v[3] = dmul(dx, dx), v[4] = dmul(dx, dy), v[5] = dmul(dx, dz), v[6] = dmul(dy, dy), v[7] = dmul(dy, dz), v[8] = dmul(dz, dz);
  }
  const double r = block_tree_sum<9>(v, s_tmp);
  if (threadIdx.x < 9) partial[9 * (size_t)blockIdx.x + threadIdx.x] = r;
}

static __global__ __launch_bounds__(64) void ba_moment_final_kernel(const double* __restrict__ P3, const int4* __restrict__ frames,
                                                                    const double* __restrict__ partial, double* __restrict__ moments) {
  const int4 fr = frames[blockIdx.x];
  double* m = moments + (size_t)BA_MOM * blockIdx.x;
  const int t = threadIdx.x;
  if (t == 0) m[0] = (double)fr.y;
  if (t < 3) m[1 + t] = P3[3 * (size_t)fr.x + t];
  if (t < 9) {
    double a = 0.0;
    for (int b = 0; b < fr.w; b++) a = dadd(a, partial[9 * (size_t)(fr.z + b) + t]);
    m[4 + t] = a;
  }
}

// one block, one thread per frame: the frames' sums, the head (thread 0: ordered sum over frames, covariance, eigenpairs, coefficients),
// and -- with terms != 0 -- every frame's gradient, diagonal block and rank-1 vectors into the workspace
static __global__ __launch_bounds__(BA_MAX_FRAMES) void ba_lin_kernel(int K, int kind, const double* __restrict__ moments, const double* __restrict__ poses,
                                                                      double* __restrict__ ws, int terms) {
  __shared__ double s_part[BA_MAX_FRAMES][9];
  __shared__ double s_head[BA_HEAD];
  __shared__ double s_tau0[3];
  const int f = threadIdx.x;
  if (f == 0) {
    double t0[3];
    ba_tau(moments, poses, t0);
    s_tau0[0] = t0[0], s_tau0[1] = t0[1], s_tau0[2] = t0[2];
  }
  __syncthreads();
  const double tau0[3] = {s_tau0[0], s_tau0[1], s_tau0[2]};
  if (f < K) {
    double part[9];
    ba_frame_sums(moments + (size_t)BA_MOM * f, poses + 12 * (size_t)f, tau0, part);
    for (int i = 0; i < 9; i++) s_part[f][i] = part[i];
  }
  __syncthreads();
  if (f == 0) {
    double sums[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, N = 0.0;
    for (int k = 0; k < K; k++) {
      for (int i = 0; i < 9; i++) sums[i] = dadd(sums[i], s_part[k][i]);
      N = dadd(N, moments[(size_t)BA_MOM * k]);
    }
    double head[BA_HEAD];
    for (int i = 0; i < BA_HEAD; i++) head[i] = 0.0;
    ba_head(N, sums, kind, head);
    for (int i = 0; i < BA_HEAD; i++) {
      s_head[i] = head[i];
      ws[i] = head[i];
    }
  }
  __syncthreads();
  if (terms && f < K) ba_frame_terms(f, K, moments + (size_t)BA_MOM * f, poses + 12 * (size_t)f, tau0, s_head, ws);
}

static __global__ __launch_bounds__(256) void ba_fill_kernel(int K, const double* __restrict__ ws, double* __restrict__ H) {
  const int n = 6 * K;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * n) return;
  H[idx] = ba_hessian_entry(idx / n, idx % n, K, ws);
}

static __global__ void ba_eigen3_kernel(int count, const double* __restrict__ m9, double* __restrict__ evals, double* __restrict__ evecs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  double lam[3], U[9];
  eig3::direct(m9 + 9 * (size_t)i, lam, U);
  for (int j = 0; j < 3; j++) evals[3 * (size_t)i + j] = lam[j];
  for (int j = 0; j < 9; j++) evecs[9 * (size_t)i + j] = U[j];
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static bool finite_n(const double* a, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(a[i])) return false;
  return true;
}

static int check_ball_args(const glim_amd_cloud* const* clouds, int32_t S, const double* T12, const double* c3, double radius, int* total) {
  if (!(radius > 0.0) || !std::isfinite(radius)) return GLIM_AMD_ERR_INVALID;
  if (!clouds || !T12 || !c3 || S < 1 || S > MAX_CLOUDS) return GLIM_AMD_ERR_INVALID;
  int64_t sum = 0;
  for (int s = 0; s < S; s++) {
    if (!clouds[s]) return GLIM_AMD_ERR_INVALID;
    if ((glim_amd_ctx*)clouds[s]->ctx != (glim_amd_ctx*)clouds[0]->ctx) return GLIM_AMD_ERR_INVALID;
    sum += clouds[s]->n;
  }
  if (sum > (int64_t)0x7fffffff - 257) return GLIM_AMD_ERR_INVALID;
  if (!finite_n(T12, 12 * (size_t)S) || !finite_n(c3, 3)) return GLIM_AMD_ERR_INVALID;
  *total = (int)sum;
  return GLIM_AMD_OK;
}

// the transformed points of a ball query on the device: descriptors + q4 (caller holds ctx->mu, device set)
struct Ball {
  DeviceTemp descs, q4;
  int S = 0, total = 0, nblocks = 0;
};

static int ball_prepare(hipStream_t st, const glim_amd_cloud* const* clouds, int32_t S, const double* T12, const double* c3, int total, Ball* b) {
  std::vector<SubDesc> h((size_t)S);
  int off = 0;
  for (int s = 0; s < S; s++) {
    SubDesc& d = h[(size_t)s];
    d.p64 = clouds[s]->pts64;
    d.p32 = clouds[s]->pts;
    d.n = (int)clouds[s]->n;
    d.off = off;
    off += d.n;
    for (int i = 0; i < 12; i++) d.T[i] = T12[12 * (size_t)s + i];
    for (int r = 0; r < 3; r++) d.T[4 * r + 3] = T12[12 * (size_t)s + 4 * r + 3] - c3[r];
  }
  b->S = S;
  b->total = total;
  b->nblocks = (total + 255) / 256;
  GA_HIP(pool_malloc(&b->descs.p, (size_t)S * sizeof(SubDesc)));
  GA_HIP(pool_malloc(&b->q4.p, (size_t)std::max(total, 1) * sizeof(double4)));
  GA_HIP(hipMemcpyAsync(b->descs.p, h.data(), (size_t)S * sizeof(SubDesc), hipMemcpyHostToDevice, st));
  GA_HIP(hipStreamSynchronize(st));  // h leaves scope with this call
  if (total > 0) {
    ba_transform_kernel<<<b->nblocks, 256, 0, st>>>(b->descs.as<SubDesc>(), S, total, b->q4.as<double4>());
    GA_HIP(hipGetLastError());
  }
  return GLIM_AMD_OK;
}

// flags + prefix sum + compaction of at most `capacity` pairs; pos has total + 1 entries, pos[total] = the count
struct Selection {
  DeviceTemp flags, pos, tiles, pairs;
};
static int ball_select(hipStream_t st, const Ball& b, double radius, int capacity, Selection* sel) {
  const unsigned int T = (unsigned int)b.total + 1u;
  GA_HIP(pool_malloc(&sel->flags.p, (size_t)T * sizeof(int)));
  GA_HIP(pool_malloc(&sel->pos.p, (size_t)T * sizeof(int)));
  GA_HIP(pool_malloc(&sel->tiles.p, scan_scratch_ints(T) * sizeof(int)));
  GA_HIP(pool_malloc(&sel->pairs.p, (size_t)std::max(capacity, 1) * 2 * sizeof(int)));
  GA_HIP(hipMemsetAsync(sel->flags.as<int>() + b.total, 0, sizeof(int), st));
  if (b.total > 0) ba_flag_kernel<<<b.nblocks, 256, 0, st>>>(b.q4.as<double4>(), b.total, radius * radius, sel->flags.as<int>());
  GA_HIP(exclusive_scan_int(st, sel->flags.as<int>(), T, sel->tiles.as<int>(), sel->pos.as<int>()));
  if (b.total > 0 && capacity > 0)
    ba_scatter_kernel<<<b.nblocks, 256, 0, st>>>(sel->flags.as<int>(), sel->pos.as<int>(), b.total, b.descs.as<SubDesc>(), b.S, capacity, sel->pairs.as<int>());
  GA_HIP(hipGetLastError());
  return GLIM_AMD_OK;
}

static void free_factor(glim_amd_ba_factor* f) {
  if (!f) return;
  if (f->ctx) (void)hipSetDevice(f->ctx->device);
  if (f->d_moments) (void)pool_free(f->d_moments);
  if (f->d_poses) (void)pool_free(f->d_poses);
  if (f->d_ws) (void)pool_free(f->d_ws);
  if (f->d_H) (void)pool_free(f->d_H);
  delete f;
}
using FactorPtr = std::unique_ptr<glim_amd_ba_factor, void (*)(glim_amd_ba_factor*)>;

// moments of N points on the device (P3, grouped by frame) -> a factor.  counts: points of each kept frame, in order.  Caller holds ctx->mu.
static int build_factor(glim_amd_ctx* ctx, hipStream_t st, int kind, const double* d_P3, const std::vector<int>& counts, const std::vector<int32_t>& kept,
                        glim_amd_ba_factor** out) {
  const int K = (int)counts.size();
  FactorPtr f(new glim_amd_ba_factor, free_factor);
  f->ctx = ctx;
  f->kind = kind;
  f->K = K;
  f->kept = kept;
  std::vector<int4> frames((size_t)K);
  std::vector<int2> blockmap;
  int start = 0;
  for (int k = 0; k < K; k++) {
    const int nb = (counts[(size_t)k] + 255) / 256;
    frames[(size_t)k] = make_int4(start, counts[(size_t)k], (int)blockmap.size(), nb);
    for (int c = 0; c < nb; c++) blockmap.push_back(make_int2(k, c));
    start += counts[(size_t)k];
  }
  f->N = start;
  DeviceTemp d_frames, d_map, d_partial;
  GA_HIP(pool_malloc(&d_frames.p, frames.size() * sizeof(int4)));
  GA_HIP(pool_malloc(&d_map.p, blockmap.size() * sizeof(int2)));
  GA_HIP(pool_malloc(&d_partial.p, blockmap.size() * 9 * sizeof(double)));
  GA_HIP(pool_malloc(&f->d_moments, (size_t)K * BA_MOM * sizeof(double)));
  GA_HIP(pool_malloc(&f->d_poses, (size_t)K * 12 * sizeof(double)));
  GA_HIP(pool_malloc(&f->d_ws, ba_workspace_doubles(K) * sizeof(double)));
  GA_HIP(pool_malloc(&f->d_H, (size_t)36 * K * K * sizeof(double)));
  SyncOnExit in_flight(st);
  GA_HIP(hipMemcpyAsync(d_frames.p, frames.data(), frames.size() * sizeof(int4), hipMemcpyHostToDevice, st));
  GA_HIP(hipMemcpyAsync(d_map.p, blockmap.data(), blockmap.size() * sizeof(int2), hipMemcpyHostToDevice, st));
  ba_moment_partial_kernel<<<(unsigned int)blockmap.size(), 256, 0, st>>>(d_P3, d_frames.as<int4>(), d_map.as<int2>(), d_partial.as<double>());
  ba_moment_final_kernel<<<K, 64, 0, st>>>(d_P3, d_frames.as<int4>(), d_partial.as<double>(), f->d_moments);
  GA_HIP(hipGetLastError());
  f->moments.resize((size_t)K * BA_MOM);
  GA_HIP(hipMemcpyAsync(f->moments.data(), f->d_moments, f->moments.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  *out = f.release();
  return GLIM_AMD_OK;
}

static int run_linearize(const glim_amd_ba_factor* f, const double* poses12, double* cost, double* g, double* H, uint32_t* status, bool terms) {
  if (!f || !poses12 || !cost) return GLIM_AMD_ERR_INVALID;
  if (terms && (!g || !H)) return GLIM_AMD_ERR_INVALID;
  const int K = f->K;
  if (!finite_n(poses12, 12 * (size_t)K)) return GLIM_AMD_ERR_INVALID;
  glim_amd_ctx* ctx = f->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  SyncOnExit in_flight(st);
  GA_HIP(hipMemcpyAsync(f->d_poses, poses12, (size_t)K * 12 * sizeof(double), hipMemcpyHostToDevice, st));
  ba_lin_kernel<<<1, BA_MAX_FRAMES, 0, st>>>(K, f->kind, f->d_moments, f->d_poses, f->d_ws, terms ? 1 : 0);
  double head[BA_HEAD];
  if (terms) {
    const int n = 6 * K;
    ba_fill_kernel<<<(n * n + 255) / 256, 256, 0, st>>>(K, f->d_ws, f->d_H);
    GA_HIP(hipGetLastError());
    GA_HIP(hipMemcpyAsync(H, f->d_H, (size_t)n * n * sizeof(double), hipMemcpyDeviceToHost, st));
    GA_HIP(hipMemcpyAsync(g, f->d_ws + BA_HEAD, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  GA_HIP(hipGetLastError());
  GA_HIP(hipMemcpyAsync(head, f->d_ws, sizeof(head), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  *cost = head[0];
  if (status) *status = (uint32_t)head[1];
  return GLIM_AMD_OK;
}

static int run_auto_radius(const glim_amd_cloud* const* clouds, int32_t S, const double* T12, const double* c3, double r0, const glim_amd_ba_params* params,
                           glim_amd_ba_radius_result* out, glim_amd_ba_trace_entry* entries, int32_t* num_entries) {
  int total = 0;
  GA_TRY(check_ball_args(clouds, S, T12, c3, r0, &total));
  if (!out) return GLIM_AMD_ERR_INVALID;
  glim_amd_ba_params prm;
  (void)glim_amd_ba_default_params(&prm);
  if (params) prm = *params;
  if (std::isnan(prm.min_radius) || std::isnan(prm.max_radius) || std::isnan(prm.plane_eps) || prm.min_radius > prm.max_radius) return GLIM_AMD_ERR_INVALID;
  glim_amd_ctx* ctx = clouds[0]->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  Ball b;
  DeviceTemp partials, state;
  SyncOnExit in_flight(st);
  GA_TRY(ball_prepare(st, clouds, S, T12, c3, total, &b));
  GA_HIP(pool_malloc(&partials.p, (size_t)std::max(b.nblocks, 1) * 10 * sizeof(double)));
  GA_HIP(pool_malloc(&state.p, ST_DOUBLES * sizeof(double)));
  double h_state[ST_DOUBLES];
  for (int i = 0; i < ST_DOUBLES; i++) h_state[i] = 0.0;
  h_state[0] = r0, h_state[1] = 1.0, h_state[7] = r0;
  GA_HIP(hipMemcpyAsync(state.p, h_state, sizeof(h_state), hipMemcpyHostToDevice, st));
  // every round up front: a round whose search has stopped leaves at its first instruction
  for (int round = 0; round <= GLIM_AMD_BA_MAX_TRIALS; round++) {
    if (b.nblocks > 0) ba_stats_kernel<<<b.nblocks, 256, 0, st>>>(b.q4.as<double4>(), total, 0.0, state.as<double>(), partials.as<double>());
    ba_stats_final_kernel<<<1, 10 * FINAL_RUNS, 0, st>>>(partials.as<double>(), b.nblocks, state.as<double>(), round, prm.min_radius, prm.max_radius, prm.plane_eps);
  }
  GA_HIP(hipGetLastError());
  GA_HIP(hipMemcpyAsync(h_state, state.p, sizeof(h_state), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));  // the ONE synchronisation of the search
  in_flight.dismiss();
  out->radius = h_state[2];
  out->num_points = (int64_t)h_state[3];
  for (int i = 0; i < 3; i++) out->eigenvalues[i] = h_state[4 + i];
  out->trials = (int32_t)h_state[8];
  out->stop = (int32_t)h_state[9];
  if (entries) {
    const int n = (int)h_state[10];
    for (int i = 0; i < n; i++) {
      const double* e = h_state + ST_TRACE + ENTRY_DOUBLES * i;
      entries[i].radius = e[0];
      entries[i].count = (int64_t)e[1];
      for (int j = 0; j < 3; j++) entries[i].eigenvalues[j] = e[2 + j];
      entries[i].decision = (int32_t)e[5];
      entries[i].reserved = 0;
    }
    if (num_entries) *num_entries = n;
  }
  return GLIM_AMD_OK;
}

}  // namespace ba
}  // namespace glim_amd

extern "C" {

int glim_amd_ba_default_params(glim_amd_ba_params* params) {
  if (!params) return GLIM_AMD_ERR_INVALID;
  params->min_radius = 0.1;
  params->max_radius = 5.0;
  params->plane_eps = 0.01;
  return GLIM_AMD_OK;
}

int glim_amd_ba_ball_select(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12, const double* center3, double radius,
                            int64_t capacity, int32_t* pairs, int64_t* count) {
  using namespace glim_amd;
  using namespace glim_amd::ba;
  if (capacity < 0 || !count || (capacity > 0 && !pairs)) return GLIM_AMD_ERR_INVALID;
  int total = 0;
  GA_TRY(check_ball_args(clouds, num_clouds, T_world_submap12, center3, radius, &total));
  glim_amd_ctx* ctx = clouds[0]->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  Ball b;
  Selection sel;
  SyncOnExit in_flight(st);
  GA_TRY(ball_prepare(st, clouds, num_clouds, T_world_submap12, center3, total, &b));
  const int cap = (int)std::min<int64_t>(capacity, total);
  GA_TRY(ball_select(st, b, radius, cap, &sel));
  int n = 0;
  GA_HIP(read_back_sync(ctx, st, &n, sel.pos.as<int>() + total, sizeof(int)));
  const int wr = std::min(n, cap);
  if (wr > 0) {
    GA_HIP(hipMemcpyAsync(pairs, sel.pairs.p, (size_t)wr * 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    GA_HIP(hipStreamSynchronize(st));
  }
  in_flight.dismiss();
  *count = n;
  return GLIM_AMD_OK;
}

int glim_amd_ba_ball_stats(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12, const double* center3, double radius,
                           glim_amd_ba_stats* out) {
  using namespace glim_amd;
  using namespace glim_amd::ba;
  if (!out) return GLIM_AMD_ERR_INVALID;
  int total = 0;
  GA_TRY(check_ball_args(clouds, num_clouds, T_world_submap12, center3, radius, &total));
  glim_amd_ctx* ctx = clouds[0]->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  Ball b;
  DeviceTemp partials, state;
  SyncOnExit in_flight(st);
  GA_TRY(ball_prepare(st, clouds, num_clouds, T_world_submap12, center3, total, &b));
  GA_HIP(pool_malloc(&partials.p, (size_t)std::max(b.nblocks, 1) * 10 * sizeof(double)));
  GA_HIP(pool_malloc(&state.p, ST_DOUBLES * sizeof(double)));
  if (b.nblocks > 0) ba_stats_kernel<<<b.nblocks, 256, 0, st>>>(b.q4.as<double4>(), total, radius, nullptr, partials.as<double>());
  ba_stats_final_kernel<<<1, 10 * FINAL_RUNS, 0, st>>>(partials.as<double>(), b.nblocks, state.as<double>(), -1, 0.0, 0.0, 0.0);
  GA_HIP(hipGetLastError());
  double h[13];
  GA_HIP(read_back_sync(ctx, st, h, state.as<double>() + 11, sizeof(h)));
  in_flight.dismiss();
  out->num_points = (int64_t)h[0];
  for (int i = 0; i < 3; i++) out->sum[i] = h[1 + i];
  for (int i = 0; i < 6; i++) out->sum_cross[i] = h[4 + i];
  for (int i = 0; i < 3; i++) out->eigenvalues[i] = h[10 + i];
  return GLIM_AMD_OK;
}

int glim_amd_ba_auto_radius(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12, const double* center3, double radius0,
                            const glim_amd_ba_params* params, glim_amd_ba_radius_result* out) {
  return glim_amd::ba::run_auto_radius(clouds, num_clouds, T_world_submap12, center3, radius0, params, out, nullptr, nullptr);
}

int glim_amd_debug_ba_auto_radius_trace(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12, const double* center3,
                                        double radius0, const glim_amd_ba_params* params, glim_amd_ba_radius_result* out, glim_amd_ba_trace_entry* entries,
                                        int32_t* num_entries) {
  if (!entries || !num_entries) return GLIM_AMD_ERR_INVALID;
  return glim_amd::ba::run_auto_radius(clouds, num_clouds, T_world_submap12, center3, radius0, params, out, entries, num_entries);
}

int glim_amd_ba_factor_create(glim_amd_ctx* ctx, int32_t kind, int64_t n, const double* points3, const int32_t* frame_index, int32_t num_frames,
                              glim_amd_ba_factor** out) {
  using namespace glim_amd;
  using namespace glim_amd::ba;
  if (!out) return GLIM_AMD_ERR_INVALID;
  *out = nullptr;
  if (kind != GLIM_AMD_BA_PLANE && kind != GLIM_AMD_BA_EDGE) return GLIM_AMD_ERR_INVALID;
  if (n < 3 || n > (int64_t)(1 << 28) || num_frames < 1 || num_frames > GLIM_AMD_BA_MAX_FRAMES) return GLIM_AMD_ERR_INVALID;
  if (!ctx || !points3 || !frame_index) return GLIM_AMD_ERR_INVALID;
  if (!finite_n(points3, 3 * (size_t)n)) return GLIM_AMD_ERR_INVALID;
  // factor order: ascending frame, then the order given (a stable counting sort)
  std::vector<int> per_frame((size_t)num_frames, 0);
  for (int64_t i = 0; i < n; i++) {
    if (frame_index[i] < 0 || frame_index[i] >= num_frames) return GLIM_AMD_ERR_INVALID;
    per_frame[(size_t)frame_index[i]]++;
  }
  std::vector<int> first((size_t)num_frames, 0), counts;
  std::vector<int32_t> kept;
  int acc = 0;
  for (int f = 0; f < num_frames; f++) {
    first[(size_t)f] = acc;
    acc += per_frame[(size_t)f];
    if (per_frame[(size_t)f] > 0) {
      counts.push_back(per_frame[(size_t)f]);
      kept.push_back(f);
    }
  }
  std::vector<double> sorted(3 * (size_t)n);
  for (int64_t i = 0; i < n; i++) {
    const size_t o = (size_t)first[(size_t)frame_index[i]]++;
    for (int r = 0; r < 3; r++) sorted[3 * o + r] = points3[3 * (size_t)i + r];
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  DeviceTemp P3;
  GA_HIP(pool_malloc(&P3.p, sorted.size() * sizeof(double)));
  GA_HIP(hipMemcpyAsync(P3.p, sorted.data(), sorted.size() * sizeof(double), hipMemcpyHostToDevice, st));
  GA_HIP(hipStreamSynchronize(st));
  return build_factor(ctx, st, kind, P3.as<double>(), counts, kept, out);
}

int glim_amd_ba_factor_create_from_ball(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12, const double* center3,
                                        double radius, int32_t kind, glim_amd_ba_factor** out) {
  using namespace glim_amd;
  using namespace glim_amd::ba;
  if (!out) return GLIM_AMD_ERR_INVALID;
  *out = nullptr;
  if (kind != GLIM_AMD_BA_PLANE && kind != GLIM_AMD_BA_EDGE) return GLIM_AMD_ERR_INVALID;
  int total = 0;
  GA_TRY(check_ball_args(clouds, num_clouds, T_world_submap12, center3, radius, &total));
  glim_amd_ctx* ctx = clouds[0]->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  const int S = num_clouds;
  Ball b;
  Selection sel;
  DeviceTemp d_off, P3;
  SyncOnExit in_flight(st);
  GA_TRY(ball_prepare(st, clouds, S, T_world_submap12, center3, total, &b));
  GA_TRY(ball_select(st, b, radius, total, &sel));
  GA_HIP(pool_malloc(&d_off.p, (size_t)(S + 1) * sizeof(int)));
  ba_offsets_kernel<<<(S + 1 + 255) / 256, 256, 0, st>>>(sel.pos.as<int>(), b.descs.as<SubDesc>(), S, total, d_off.as<int>());
  GA_HIP(hipGetLastError());
  std::vector<int> rank((size_t)S + 1);
  GA_HIP(hipMemcpyAsync(rank.data(), d_off.p, rank.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  const int N = rank[(size_t)S];
  std::vector<int> counts;
  std::vector<int32_t> kept;
  for (int s = 0; s < S; s++) {
    const int c = rank[(size_t)s + 1] - rank[(size_t)s];
    if (c > 0) {
      counts.push_back(c);
      kept.push_back(s);
    }
  }
  if (N < 3 || N > total || (int)counts.size() > GLIM_AMD_BA_MAX_FRAMES) return GLIM_AMD_ERR_INVALID;
  GA_HIP(pool_malloc(&P3.p, (size_t)N * 3 * sizeof(double)));
  ba_gather_local_kernel<<<(N + 255) / 256, 256, 0, st>>>(sel.pairs.as<int>(), N, b.descs.as<SubDesc>(), P3.as<double>());
  GA_HIP(hipGetLastError());
  const int rc = build_factor(ctx, st, kind, P3.as<double>(), counts, kept, out);  // synchronises
  return rc;
}

int glim_amd_ba_factor_info(const glim_amd_ba_factor* f, int32_t* num_frames, int64_t* num_points, int32_t* kind, int32_t* kept_index, double* moments) {
  if (!f) return GLIM_AMD_ERR_INVALID;
  if (num_frames) *num_frames = f->K;
  if (num_points) *num_points = f->N;
  if (kind) *kind = f->kind;
  if (kept_index) std::memcpy(kept_index, f->kept.data(), f->kept.size() * sizeof(int32_t));
  if (moments) std::memcpy(moments, f->moments.data(), f->moments.size() * sizeof(double));
  return GLIM_AMD_OK;
}

int glim_amd_ba_factor_error(const glim_amd_ba_factor* f, const double* poses12, double* cost, uint32_t* status) {
  return glim_amd::ba::run_linearize(f, poses12, cost, nullptr, nullptr, status, false);
}

int glim_amd_ba_factor_linearize(const glim_amd_ba_factor* f, const double* poses12, double* cost, double* g, double* H, uint32_t* status) {
  return glim_amd::ba::run_linearize(f, poses12, cost, g, H, status, true);
}

int glim_amd_ba_factor_destroy(glim_amd_ba_factor* f) {
  glim_amd::ba::free_factor(f);
  return GLIM_AMD_OK;
}

int glim_amd_debug_ba_eigen3(glim_amd_ctx* ctx, int32_t count, const double* m9, double* evals, double* evecs) {
  using namespace glim_amd;
  using namespace glim_amd::ba;
  if (!ctx || count < 0 || (count > 0 && (!m9 || !evals || !evecs))) return GLIM_AMD_ERR_INVALID;
  if (count == 0) return GLIM_AMD_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  DeviceTemp d_m, d_l, d_u;
  GA_HIP(pool_malloc(&d_m.p, (size_t)count * 9 * sizeof(double)));
  GA_HIP(pool_malloc(&d_l.p, (size_t)count * 3 * sizeof(double)));
  GA_HIP(pool_malloc(&d_u.p, (size_t)count * 9 * sizeof(double)));
  SyncOnExit in_flight(st);
  GA_HIP(hipMemcpyAsync(d_m.p, m9, (size_t)count * 9 * sizeof(double), hipMemcpyHostToDevice, st));
  ba_eigen3_kernel<<<(count + 63) / 64, 64, 0, st>>>(count, d_m.as<double>(), d_l.as<double>(), d_u.as<double>());
  GA_HIP(hipGetLastError());
  GA_HIP(hipMemcpyAsync(evals, d_l.p, (size_t)count * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  GA_HIP(hipMemcpyAsync(evecs, d_u.p, (size_t)count * 9 * sizeof(double), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  return GLIM_AMD_OK;
}

}  // extern "C"
