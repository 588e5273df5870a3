// gnc.hip -- GNC global registration on gfx950: gtsam_points::estimate_pose_gnc as viewer/interactive/manual_loop_close_modal.cpp:445-458 calls it,
// the second consumer of fpfh.hip's descriptors and correspondences.  Semantics in include/glim_amd.h ("GNC"), layout in DESIGN.md 4.7b.
//
// It uses ransac.hip's occupancy table, round buffers and scoring launch (ransac_table.hpp), the generator of sample_hash.hpp and
// registration_host.hpp's host scaffold.
//
// select   keep[i] = candidate and matched and both points finite (the candidate marks are plain stores of one value), exclusive scan of scan.hpp,
//          compaction into (source index, target index) pairs in ascending i.
// tuples   one lane per trial: three counter-based draws, the edge rule, a pass flag; scan; the first max_num_tuples passing trials in trial order.
// gather   the list as 24 bytes per entry (source xyz, target xyz in FP32): what the solve kernel streams once per iteration.
// solve    the hot path: ONE launch of ONE block of 512 lanes runs the centroids, the scale and every iteration.  A lane walks its entries at
//          stride 512 in ascending order with 17 FP64 accumulators; the lanes are added by an xor-butterfly written step-major, the 8 wavefront
//          sums through LDS in wavefront order; every lane then computes the pose step (gnc_pose.hpp) from the same LDS sums redundantly: no lane
//          waits for another's pose, and nothing has to be broadcast before the next iteration's first load.
// score    ransac.hip's Table and rs_score_kernel with one hypothesis: the solve kernel leaves its pose where that kernel reads it.
#include <algorithm>
#include <cmath>
#include <vector>

#include "device_math.hpp"
#include "gnc_pose.hpp"
#include "internal.hpp"
#include "ransac_table.hpp"
#include "registration_host.hpp"
#include "sample_hash.hpp"
#include "scan.hpp"
#include "scope_sync.hpp"

namespace glim_amd {
namespace gnc_detail {

using ransac_detail::sample_hash;
using reg_detail::Pair;
using ransac_detail::u32;
using ransac_detail::u64;

constexpr int SOLVE_BLOCK = 512;  // 8 wavefronts, 2 per SIMD: a budget of 256 registers (the pose step needs ~150; at 1024 lanes it is 128 and spills)
constexpr int SOLVE_WAVES = SOLVE_BLOCK / 64;
constexpr int NSUM = 17;   // W | a | b | M | cost
constexpr int NPART = 18;  // the frame pass reduces 18 values (6 sums, 6 minima, 6 maxima)
constexpr int64_t MAX_TRIALS = (int64_t)1 << 22;
constexpr int TRACE_STRIDE = 15;  // mu | W | cost | 12 pose doubles

__device__ __forceinline__ bool finite3(const float4 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

__global__ __launch_bounds__(256) void gnc_mark_kernel(int samples, u64 seed, int n_src, int* __restrict__ mark) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < samples) mark[(int)(sample_hash(seed, (u64)j) % (u64)n_src)] = 1;  // (every writer of a word stores the same value)
}

// keep has n_src + 1 entries: the last one is 0, so that the exclusive scan's last entry is the list length
__global__ __launch_bounds__(256) void gnc_keep_kernel(int n_src, int n_tgt, const int* __restrict__ mark, const float4* __restrict__ spts,
                                                       const float4* __restrict__ tpts, const int* __restrict__ nearest, int* __restrict__ keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > n_src) return;
  int k = 0;
  if (i < n_src && (!mark || mark[i])) {
    const int t = nearest[i];
    if (t >= 0 && t < n_tgt) k = finite3(spts[i]) && finite3(tpts[t]) ? 1 : 0;
  }
  keep[i] = k;
}

__global__ __launch_bounds__(256) void gnc_compact_kernel(int n_src, const int* __restrict__ keep, const int* __restrict__ rank,
                                                          const int* __restrict__ nearest, int2* __restrict__ list) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_src && keep[i]) list[rank[i]] = make_int2(i, nearest[i]);
}

__device__ __forceinline__ double edge_length(const float4 a, const float4 b) {
#pragma clang fp contract(off)
  const double dx = (double)a.x - (double)b.x, dy = (double)a.y - (double)b.y, dz = (double)a.z - (double)b.z;
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

// pass has trials + 1 entries, the last one 0
__global__ __launch_bounds__(256) void gnc_tuple_kernel(int trials, u64 seed1, int C, const int2* __restrict__ list, const float4* __restrict__ spts,
                                                        const float4* __restrict__ tpts, double tuple_thresh, int* __restrict__ pass) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j > trials) return;
  int ok = 0;
  if (j < trials) {
    int c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = (int)(sample_hash(seed1, 3ull * (u64)j + (u64)k) % (u64)C);
    if (c[0] != c[1] && c[1] != c[2] && c[0] != c[2]) {
      float4 s[3], t[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const int2 e = list[c[k]];
        s[k] = spts[e.x];
        t[k] = tpts[e.y];
      }
      ok = 1;
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const int b = (a + 1) % 3;
        const double ds = edge_length(s[a], s[b]), dt = edge_length(t[a], t[b]);
        const double lo = ds < dt ? ds : dt, hi = ds < dt ? dt : ds;
        if (!(hi > 0.0) || !(lo >= tuple_thresh * hi)) ok = 0;
      }
    }
  }
  pass[j] = ok;
}

__global__ __launch_bounds__(256) void gnc_tuple_compact_kernel(int trials, u64 seed1, int C, int max_tuples, const int* __restrict__ pass,
                                                                const int* __restrict__ rank, const int2* __restrict__ list, int2* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= trials || !pass[j]) return;
  const int r = rank[j];
  if (r >= max_tuples) return;
#pragma unroll
  for (int k = 0; k < 3; k++) out[3 * (size_t)r + k] = list[(int)(sample_hash(seed1, 3ull * (u64)j + (u64)k) % (u64)C)];
}

// entry e: pairs[3 e] = (s.x, s.y), [3 e + 1] = (s.z, t.x), [3 e + 2] = (t.y, t.z)
__global__ __launch_bounds__(256) void gnc_gather_kernel(int L, const int2* __restrict__ list, const float4* __restrict__ spts,
                                                         const float4* __restrict__ tpts, float2* __restrict__ pairs) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= L) return;
  const int2 st = list[e];
  const float4 s = spts[st.x], t = tpts[st.y];
  pairs[3 * (size_t)e] = make_float2(s.x, s.y);
  pairs[3 * (size_t)e + 1] = make_float2(s.z, t.x);
  pairs[3 * (size_t)e + 2] = make_float2(t.y, t.z);
}

struct SolveOut {
  double T[12];
  double frame[7];  // c_s | c_t | D^2
  double mu_final, W, cost;
  int iterations_run, pad;
};

enum { OP_SUM = 0, OP_MIN = 1, OP_MAX = 2 };
__device__ __forceinline__ double combine(int op, double x, double y) { return op == OP_SUM ? x + y : op == OP_MIN ? (y < x ? y : x) : (y > x ? y : x); }

// v[0 .. N) of every lane of the block -> the same N block results in every lane.  Entries [0, n_sum) are added, then n_min minima, the rest maxima.
// Butterfly step-major: the N chains of a step are independent of one another.  Ends with a barrier: s_part may be written again at once.
template <int N>
__device__ __forceinline__ void block_reduce(double (&v)[N], int n_sum, int n_min, double* s_part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int b = 0; b < N; b++) v[b] = combine(b < n_sum ? OP_SUM : b < n_sum + n_min ? OP_MIN : OP_MAX, v[b], __shfl_xor(v[b], off, 64));
  }
  if (lane == 0) {
#pragma unroll
    for (int b = 0; b < N; b++) s_part[wave * NPART + b] = v[b];
  }
  __syncthreads();
#pragma unroll
  for (int b = 0; b < N; b++) v[b] = s_part[b];
  for (int w = 1; w < SOLVE_WAVES; w++) {  // wavefront order
#pragma unroll
    for (int b = 0; b < N; b++) v[b] = combine(b < n_sum ? OP_SUM : b < n_sum + n_min ? OP_MIN : OP_MAX, v[b], s_part[w * NPART + b]);
  }
  __syncthreads();
}

__device__ __forceinline__ void load_entry(const float2* __restrict__ pairs, int e, double* s, double* t) {
  const float2 a = pairs[3 * (size_t)e], b = pairs[3 * (size_t)e + 1], c = pairs[3 * (size_t)e + 2];
  s[0] = (double)a.x, s[1] = (double)a.y, s[2] = (double)b.x;
  t[0] = (double)b.y, t[1] = (double)c.x, t[2] = (double)c.y;
}

// ONE block.  trace (max_iterations x 15) and weights (2 x L: iteration k writes half k & 1, so that an iteration that does not complete leaves
// the weights of the one before it alone) may be null.  poses / status / counts: hypothesis 0 of ransac.hip's scoring kernel.
__global__ __launch_bounds__(SOLVE_BLOCK) void gnc_solve_kernel(int L, const float2* __restrict__ pairs, double max_corr_dist, double div_factor,
                                                                 int max_iterations, int dof, SolveOut* __restrict__ out, double* __restrict__ trace,
                                                                 double* __restrict__ weights, double* __restrict__ poses, int* __restrict__ status,
                                                                 int* __restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ double s_part[SOLVE_WAVES * NPART];
  const int tid = threadIdx.x;
  // ---- frame: centroids (the tree of the loop's sums) and the two bounding boxes
  double cs[3], ct[3], D2;
  {
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double f[NPART];
#pragma unroll
    for (int b = 0; b < 6; b++) f[b] = 0.0, f[6 + b] = inf, f[12 + b] = -inf;
    for (int e = tid; e < L; e += SOLVE_BLOCK) {
      double s[3], t[3];
      load_entry(pairs, e, s, t);
#pragma unroll
      for (int b = 0; b < 3; b++) {
        f[b] = f[b] + s[b];
        f[3 + b] = f[3 + b] + t[b];
        f[6 + b] = s[b] < f[6 + b] ? s[b] : f[6 + b];
        f[9 + b] = t[b] < f[9 + b] ? t[b] : f[9 + b];
        f[12 + b] = s[b] > f[12 + b] ? s[b] : f[12 + b];
        f[15 + b] = t[b] > f[15 + b] ? t[b] : f[15 + b];
      }
    }
    block_reduce<NPART>(f, 6, 6, s_part);
    const double n = (double)L;
#pragma unroll
    for (int b = 0; b < 3; b++) cs[b] = f[b] / n, ct[b] = f[3 + b] / n;
    const double sx = f[12] - f[6], sy = f[13] - f[7], sz = f[14] - f[8], tx = f[15] - f[9], ty = f[16] - f[10], tz = f[17] - f[11];
    const double ds = (sx * sx + sy * sy) + sz * sz, dt = (tx * tx + ty * ty) + tz * tz;
    D2 = dt > ds ? dt : ds;
  }
  double mu = D2, mu_min;
  if (max_corr_dist > 0.0) {
    mu_min = max_corr_dist * max_corr_dist;
  } else {
    const double m = 0.025 * sqrt(D2);
    mu_min = m * m;
  }
  double T[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  double mu_last = mu, W_last = 0.0, cost_last = 0.0;
  int k = 0;
  for (; k < max_iterations; k++) {
    double acc[NSUM];
#pragma unroll
    for (int b = 0; b < NSUM; b++) acc[b] = 0.0;
    for (int e = tid; e < L; e += SOLVE_BLOCK) {
      double s[3], t[3];
      load_entry(pairs, e, s, t);
      double x, y, z;
      transform_point_d(T, s[0], s[1], s[2], x, y, z);
      const double dx = t[0] - x, dy = t[1] - y, dz = t[2] - z;
      const double r2 = (dx * dx + dy * dy) + dz * dz;
      const double g = mu / (mu + r2);
      const double w = g * g;
      if (weights) weights[(size_t)(k & 1) * (size_t)L + e] = w;
      acc[0] = acc[0] + w;
      acc[16] = fma(w, r2, acc[16]);
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const double p = s[i] - cs[i], q = t[i] - ct[i];
        acc[1 + i] = fma(w, p, acc[1 + i]);
        acc[4 + i] = fma(w, q, acc[4 + i]);
        const double wp = w * p;
#pragma unroll
        for (int j = 0; j < 3; j++) acc[7 + 3 * i + j] = fma(wp, t[j] - ct[j], acc[7 + 3 * i + j]);
      }
    }
    block_reduce<NSUM>(acc, NSUM, 0, s_part);
    double Tn[12];
    if (!gnc_pose::pose_from_moments(acc[0], acc + 1, acc + 4, acc + 7, cs, ct, dof, Tn)) break;  // (uniform: every lane holds the same sums)
#pragma unroll
    for (int i = 0; i < 12; i++) T[i] = Tn[i];
    mu_last = mu, W_last = acc[0], cost_last = acc[16];
    if (trace && tid == 0) {
      double* row = trace + (size_t)k * TRACE_STRIDE;
      row[0] = mu, row[1] = acc[0], row[2] = acc[16];
#pragma unroll
      for (int i = 0; i < 12; i++) row[3 + i] = T[i];
    }
    if ((k & 3) == 3 && mu > mu_min) {
      const double next = mu / div_factor;
      mu = next > mu_min ? next : mu_min;
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 12; i++) out->T[i] = T[i], poses[i] = T[i];
#pragma unroll
    for (int b = 0; b < 3; b++) out->frame[b] = cs[b], out->frame[3 + b] = ct[b];
    out->frame[6] = D2;
    out->mu_final = mu_last, out->W = W_last, out->cost = cost_last;
    out->iterations_run = k, out->pad = 0;
    status[0] = k > 0 ? 0 : 1;  // (not scored when no iteration completed)
    counts[0] = 0;
  }
}

int check_params(const glim_amd_gnc_params* p) {
  if (!p) return GLIM_AMD_ERR_INVALID;
  if (p->dof != 4 && p->dof != 6) return GLIM_AMD_ERR_INVALID;
  if (p->max_iterations <= 0 || p->max_init_samples <= 0) return GLIM_AMD_ERR_INVALID;
  if (p->tuple_check && p->max_num_tuples <= 0) return GLIM_AMD_ERR_INVALID;
  if (!std::isfinite(p->div_factor) || !(p->div_factor > 1.0)) return GLIM_AMD_ERR_INVALID;
  if (std::isnan(p->tuple_thresh) || !std::isfinite(p->max_corr_dist)) return GLIM_AMD_ERR_INVALID;
  if (!std::isfinite(p->inlier_voxel_resolution) || !(p->inlier_voxel_resolution > 0.0)) return GLIM_AMD_ERR_INVALID;
  return GLIM_AMD_OK;
}

// what glim_amd_gnc_debug_trace hands out (host pointers, any may be null)
struct Trace {
  int64_t list_capacity = 0;
  int32_t* list_pairs = nullptr;
  int64_t* list_length = nullptr;
  double *frame7 = nullptr, *iterations15 = nullptr, *weights = nullptr;
};

using StageClock = reg_detail::StageClock<6>;  // the six boundaries of the five stages (glim_amd_gnc_profile)

inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

// caller holds ctx->mu, the device is set, p.d_nearest is on the device and in range; info is not null
int run(const Pair& p, const glim_amd_gnc_params& prm, glim_amd_registration_result* result, glim_amd_gnc_info* info, const Trace* trace,
        StageClock* clock) {
  hipStream_t st = p.st;
  *info = glim_amd_gnc_info{};
  reg_detail::identity_result(result, 0);
  if (trace && trace->list_length) *trace->list_length = 0;
  StageClock idle;
  if (!clock) clock = &idle;
  clock->mark(0, st);
  if (p.n_src == 0 || p.n_tgt == 0) {
    for (int i = 1; i < 6; i++) clock->mark(i, st);
    return GLIM_AMD_OK;
  }
  SyncOnExit in_flight(st);
  // ---- 1. selection
  const int n = p.n_src;
  DeviceTemp mark, keep, rank, tiles, list;
  GA_HIP(pool_malloc(&keep.p, ((size_t)n + 1) * sizeof(int)));
  GA_HIP(pool_malloc(&rank.p, ((size_t)n + 1) * sizeof(int)));
  GA_HIP(pool_malloc(&tiles.p, scan_scratch_ints((unsigned)n + 1) * sizeof(int)));
  GA_HIP(pool_malloc(&list.p, (size_t)n * sizeof(int2)));
  if (prm.max_init_samples < n) {
    GA_HIP(pool_malloc(&mark.p, (size_t)n * sizeof(int)));
    GA_HIP(hipMemsetAsync(mark.p, 0, (size_t)n * sizeof(int), st));
    gnc_mark_kernel<<<blocks256(prm.max_init_samples), 256, 0, st>>>(prm.max_init_samples, (u64)prm.seed, n, mark.as<int>());
  }
  gnc_keep_kernel<<<blocks256((int64_t)n + 1), 256, 0, st>>>(n, p.n_tgt, mark.as<int>(), p.spts, p.tpts, p.d_nearest, keep.as<int>());
  GA_HIP(exclusive_scan_int(st, keep.as<int>(), (unsigned)n + 1, tiles.as<int>(), rank.as<int>()));
  gnc_compact_kernel<<<blocks256(n), 256, 0, st>>>(n, keep.as<int>(), rank.as<int>(), p.d_nearest, list.as<int2>());
  GA_HIP(hipGetLastError());
  int C = 0;
  GA_HIP(read_back_sync(p.ctx, st, &C, rank.as<int>() + n, sizeof(int)));
  if (C < 0 || C > n) return GLIM_AMD_ERR_STATE;
  info->num_correspondences = C;
  clock->mark(1, st);
  // ---- 2. tuple test
  int L = C;
  DeviceTemp tuples, pass, trank, ttiles;
  const int2* final_list = list.as<int2>();
  if (prm.tuple_check && C >= 3) {
    const int trials = (int)std::min<int64_t>(100ll * C, MAX_TRIALS);
    const u64 seed1 = (u64)prm.seed + 1ull;
    GA_HIP(pool_malloc(&pass.p, ((size_t)trials + 1) * sizeof(int)));
    GA_HIP(pool_malloc(&trank.p, ((size_t)trials + 1) * sizeof(int)));
    GA_HIP(pool_malloc(&ttiles.p, scan_scratch_ints((unsigned)trials + 1) * sizeof(int)));
    gnc_tuple_kernel<<<blocks256((int64_t)trials + 1), 256, 0, st>>>(trials, seed1, C, list.as<int2>(), p.spts, p.tpts, prm.tuple_thresh, pass.as<int>());
    GA_HIP(exclusive_scan_int(st, pass.as<int>(), (unsigned)trials + 1, ttiles.as<int>(), trank.as<int>()));
    GA_HIP(hipGetLastError());
    int passed = 0;
    GA_HIP(read_back_sync(p.ctx, st, &passed, trank.as<int>() + trials, sizeof(int)));
    if (passed < 0 || passed > trials) return GLIM_AMD_ERR_STATE;
    const int kept = std::min(passed, (int)prm.max_num_tuples);
    info->num_tuples = kept;
    L = 3 * kept;
    GA_HIP(pool_malloc(&tuples.p, (size_t)std::max(L, 1) * sizeof(int2)));
    if (kept > 0)
      gnc_tuple_compact_kernel<<<blocks256(trials), 256, 0, st>>>(trials, seed1, C, kept, pass.as<int>(), trank.as<int>(), list.as<int2>(),
                                                                  tuples.as<int2>());
    final_list = tuples.as<int2>();
  }
  clock->mark(2, st);
  info->list_length = L;
  if (trace) {
    if ((int64_t)L > trace->list_capacity) return GLIM_AMD_ERR_INVALID;
    if (trace->list_length) *trace->list_length = L;
    if (trace->list_pairs && L > 0) GA_HIP(hipMemcpyAsync(trace->list_pairs, final_list, (size_t)L * sizeof(int2), hipMemcpyDeviceToHost, st));
  }
  // ---- 3. no estimate
  if (L < 3) {
    GA_HIP(hipGetLastError());
    GA_HIP(hipStreamSynchronize(st));
    in_flight.dismiss();
    for (int i = 3; i < 6; i++) clock->mark(i, st);
    return GLIM_AMD_OK;
  }
  // ---- 4, 5. frame, scale and loop: one launch
  DeviceTemp pairs, out, d_trace, d_weights;
  ransac_detail::RoundBuffers b;
  GA_TRY(b.alloc());
  GA_HIP(pool_malloc(&pairs.p, (size_t)L * 3 * sizeof(float2)));
  GA_HIP(pool_malloc(&out.p, sizeof(SolveOut)));
  if (trace && trace->iterations15) GA_HIP(pool_malloc(&d_trace.p, (size_t)prm.max_iterations * TRACE_STRIDE * sizeof(double)));
  if (trace && trace->weights) GA_HIP(pool_malloc(&d_weights.p, 2 * (size_t)L * sizeof(double)));
  gnc_gather_kernel<<<blocks256(L), 256, 0, st>>>(L, final_list, p.spts, p.tpts, pairs.as<float2>());
  gnc_solve_kernel<<<1, SOLVE_BLOCK, 0, st>>>(L, pairs.as<float2>(), prm.max_corr_dist, prm.div_factor, prm.max_iterations, prm.dof, out.as<SolveOut>(),
                                              d_trace.as<double>(), d_weights.as<double>(), b.poses.as<double>(), b.status.as<int>(),
                                              b.counts.as<int>());
  GA_HIP(hipGetLastError());
  clock->mark(3, st);
  // ---- 6. the occupancy table and the score of the last pose
  ransac_detail::Table table;
  GA_TRY(ransac_detail::build_table(p.ctx, st, p.tpts, p.n_tgt, 1.0 / prm.inlier_voxel_resolution, &table));
  clock->mark(4, st);
  ransac_detail::launch_score(p, prm.inlier_voxel_resolution, table, b, 1);
  GA_HIP(hipGetLastError());
  clock->mark(5, st);
  SolveOut h{};
  int hits = 0;
  GA_HIP(hipMemcpyAsync(&h, out.p, sizeof(SolveOut), hipMemcpyDeviceToHost, st));
  GA_HIP(hipMemcpyAsync(&hits, b.counts.p, sizeof(int), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  if (h.iterations_run < 0 || h.iterations_run > prm.max_iterations) return GLIM_AMD_ERR_STATE;
  if (trace) {
    if (trace->frame7) std::memcpy(trace->frame7, h.frame, sizeof(h.frame));
    if (trace->iterations15 && h.iterations_run > 0)
      GA_HIP(hipMemcpyAsync(trace->iterations15, d_trace.p, (size_t)h.iterations_run * TRACE_STRIDE * sizeof(double), hipMemcpyDeviceToHost, st));
    if (trace->weights && h.iterations_run > 0)  // the half the last COMPLETED iteration wrote
      GA_HIP(hipMemcpyAsync(trace->weights, d_weights.as<double>() + (size_t)((h.iterations_run - 1) & 1) * (size_t)L, (size_t)L * sizeof(double),
                            hipMemcpyDeviceToHost, st));
    GA_HIP(hipStreamSynchronize(st));
  }
  in_flight.dismiss();
  if (h.iterations_run == 0) return GLIM_AMD_OK;  // (the "no estimate" result stands)
  std::memcpy(result->T_target_source, h.T, sizeof(h.T));
  result->num_inliers = hits;
  result->inlier_rate = (double)hits / (double)p.n_src;
  result->iterations_run = h.iterations_run;
  result->best_iteration = h.iterations_run - 1;
  info->mu_final = h.mu_final;
  info->weight_sum = h.W;
  info->cost = h.cost;
  return GLIM_AMD_OK;
}

// the entries that take `nearest` from the host; us5: the five stage times of glim_amd_gnc_profile, over `iters` timed calls
int run_with_host_nearest(const glim_amd_cloud* target, const glim_amd_cloud* source, const int32_t* nearest, const glim_amd_gnc_params* params,
                          glim_amd_registration_result* result, glim_amd_gnc_info* info, const Trace* trace, int iters, float* us5) {
  if (!result) return GLIM_AMD_ERR_INVALID;
  GA_TRY(reg_detail::check_pair(target, source));
  GA_TRY(check_params(params));
  GA_TRY(reg_detail::check_nearest(nearest, source->n, target->n));
  glim_amd_gnc_info local;
  if (!info) info = &local;
  return reg_detail::with_host_nearest(target, source, nearest, [&](const Pair& p) -> int {
    if (!us5) return run(p, *params, result, info, trace, nullptr);
    StageClock clock;
    GA_TRY(clock.start());
    double sum[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = -1; i < iters; i++) {  // one warm-up call
      GA_TRY(run(p, *params, result, info, nullptr, &clock));
      GA_HIP(hipStreamSynchronize(p.st));
      for (int k = 0; k < 5 && i >= 0; k++) GA_HIP(clock.add_us(k, &sum[k]));
    }
    for (int k = 0; k < 5; k++) us5[k] = (float)(sum[k] / iters);
    return GLIM_AMD_OK;
  });
}

}  // namespace gnc_detail
}  // namespace glim_amd

extern "C" {

int glim_amd_gnc_default_params(glim_amd_gnc_params* params) {
  if (!params) return GLIM_AMD_ERR_INVALID;
  params->max_init_samples = 5000;
  params->tuple_check = 0;
  params->tuple_thresh = 0.9;
  params->max_num_tuples = 1000;
  params->div_factor = 1.4;
  params->max_iterations = 64;
  params->max_corr_dist = 0.0;
  params->inlier_voxel_resolution = 1.0;
  params->dof = 6;
  params->seed = 0;
  return GLIM_AMD_OK;
}

int glim_amd_gnc_align(const glim_amd_cloud* target, const glim_amd_cloud* source, const int32_t* nearest, const glim_amd_gnc_params* params,
                       glim_amd_registration_result* result, glim_amd_gnc_info* info) {
  return glim_amd::gnc_detail::run_with_host_nearest(target, source, nearest, params, result, info, nullptr, 0, nullptr);
}

int glim_amd_gnc_align_fpfh(const glim_amd_cloud* target, const glim_amd_cloud* source, const glim_amd_fpfh* target_fpfh,
                            const glim_amd_fpfh* source_fpfh, uint32_t match_flags, const glim_amd_gnc_params* params,
                            glim_amd_registration_result* result, glim_amd_gnc_info* info) {
  using namespace glim_amd;
  using namespace glim_amd::gnc_detail;
  if (!result) return GLIM_AMD_ERR_INVALID;
  GA_TRY(reg_detail::check_fpfh_pair(target, source, target_fpfh, source_fpfh, match_flags));
  GA_TRY(check_params(params));
  glim_amd_gnc_info local;
  if (!info) info = &local;
  if (source->n == 0 || target->n == 0) {
    *info = glim_amd_gnc_info{};
    reg_detail::identity_result(result, 0);
    return GLIM_AMD_OK;
  }
  return reg_detail::with_matched_nearest(target, source, target_fpfh, source_fpfh, match_flags,
                                          [&](const Pair& p) { return run(p, *params, result, info, nullptr, nullptr); });
}

int glim_amd_gnc_debug_trace(const glim_amd_cloud* target, const glim_amd_cloud* source, const int32_t* nearest, const glim_amd_gnc_params* params,
                             int64_t list_capacity, int32_t* list_pairs, int64_t* list_length, double* frame7, double* iterations15,
                             double* weights, glim_amd_registration_result* result, glim_amd_gnc_info* info) {
  if (!list_length || list_capacity < 0) return GLIM_AMD_ERR_INVALID;
  glim_amd::gnc_detail::Trace t;
  t.list_capacity = list_capacity;
  t.list_pairs = list_pairs;
  t.list_length = list_length;
  t.frame7 = frame7;
  t.iterations15 = iterations15;
  t.weights = weights;
  return glim_amd::gnc_detail::run_with_host_nearest(target, source, nearest, params, result, info, &t, 0, nullptr);
}

int glim_amd_gnc_profile(const glim_amd_cloud* target, const glim_amd_cloud* source, const int32_t* nearest, const glim_amd_gnc_params* params,
                         int iters, float* us_select, float* us_tuples, float* us_solve, float* us_table, float* us_score) {
  if (iters <= 0) return GLIM_AMD_ERR_INVALID;
  glim_amd_registration_result r;
  float us[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  const int rc = glim_amd::gnc_detail::run_with_host_nearest(target, source, nearest, params, &r, nullptr, nullptr, iters, us);
  if (rc != GLIM_AMD_OK) return rc;
  if (us_select) *us_select = us[0];
  if (us_tuples) *us_tuples = us[1];
  if (us_solve) *us_solve = us[2];
  if (us_table) *us_table = us[3];
  if (us_score) *us_score = us[4];
  return GLIM_AMD_OK;
}

}  // extern "C"
