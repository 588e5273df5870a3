// ransac.hip -- RANSAC global registration on gfx950: gtsam_points::estimate_pose_ransac as viewer/interactive/manual_loop_close_modal.cpp:431-443
// calls it, the consumer of fpfh.hip's descriptors and correspondences.  Semantics in include/glim_amd.h ("RANSAC"), layout in DESIGN.md 4.7a.
//
// The host scaffold of the entries is registration_host.hpp, shared with gnc.hip (it is that header which uses fpfh.hip's descriptor object and
// matcher, through fpfh.hpp); the generator is sample_hash.hpp, shared with preprocess.hip; ransac_table.hpp declares what gnc.hip uses of this
// file: the occupancy table, the round buffers and the scoring launch.
//
// table      occupancy set of the target: 64-bit keys only, open addressing, power-of-two slots, load <= 0.5, insert = one 64-bit integer
//            compare-and-swap per probe.  Built twice: into a table sized by the POINTS (the number of voxels is not known yet), which also counts
//            the voxels, then re-hashed into a table sized by the VOXELS -- small enough for LDS in the usual case (<= 4 096 voxels: 8 192 slots).
// hypothesis one lane per hypothesis of a round: counter-based draw, status, ransac_pose.hpp's solver, 12-double pose out.
// score      the hot path.  A block owns 2 048 source points (4 per lane, in registers) and a run of the round's hypotheses; the pose and the
//            status of a hypothesis are read through a uniform address (scalar loads), the table is copied into LDS once per block when it fits,
//            hits are counted per wavefront by ballot + popcount, ONE integer atomic per (wavefront, hypothesis).
// fold       one block per round: (first stop, best count, best index) of the round merged into the running state, with the two poses.
// Integer counts and integer atomics only: the result does not depend on the round size, the grid or the context.
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "device_math.hpp"
#include "internal.hpp"
#include "ransac_pose.hpp"
#include "ransac_table.hpp"
#include "registration_host.hpp"
#include "sample_hash.hpp"
#include "scope_sync.hpp"

namespace glim_amd {
namespace ransac_detail {

using reg_detail::Pair;

constexpr int ROUND = 1024;          // hypotheses per round: the early stop is looked at once per round
constexpr int SC_BLOCK = 512;        // lanes of a scoring block (8 wavefronts)
constexpr int SC_PPL = 4;            // source points per lane
constexpr int SC_TILE = SC_BLOCK * SC_PPL;
constexpr int LDS_SLOTS_MAX = 8192;  // 64 KiB of keys: two blocks (16 wavefronts) per compute unit of 160 KiB; <= 4 096 slots: four blocks, the wave limit
constexpr int MIN_SLOTS = 64;

// the debug cut of the LDS form (glim_amd_debug_ransac_max_lds_slots): per thread, tests and the timing tool only
thread_local int g_lds_slots_max = LDS_SLOTS_MAX;

__device__ __forceinline__ u32 slot_of(u64 key, u32 mask) { return (u32)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask; }

// key of the voxel of (x, y, z) * inv_res, EMPTY_KEY outside [-2^20, 2^20) on any axis or when a product is NaN
__device__ __forceinline__ u64 voxel_key_or_empty(double x, double y, double z, double inv_res) {
  const double tx = dmul(x, inv_res), ty = dmul(y, inv_res), tz = dmul(z, inv_res);
  const bool in = tx >= -1048576.0 && tx < 1048576.0 && ty >= -1048576.0 && ty < 1048576.0 && tz >= -1048576.0 && tz < 1048576.0;
  return in ? pack_key(fast_floor_d(tx), fast_floor_d(ty), fast_floor_d(tz)) : EMPTY_KEY;
}

// returns true when THIS call claimed a free slot.  The table never fills (load <= 0.5), and `slot` stays masked: every access is inside it.
__device__ __forceinline__ bool table_insert(u64* __restrict__ table, u32 mask, u64 key) {
  u32 slot = slot_of(key, mask);
  for (;;) {
    const u64 old = atomicCAS(&table[slot], EMPTY_KEY, key);
    if (old == EMPTY_KEY) return true;
    if (old == key) return false;
    slot = (slot + 1u) & mask;
  }
}

__global__ __launch_bounds__(256) void rs_fill_kernel(u32 slots, u64* __restrict__ table, int* __restrict__ voxels) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i < slots) table[i] = EMPTY_KEY;
  if (i == 0 && voxels) *voxels = 0;
}

__global__ __launch_bounds__(256) void rs_insert_kernel(int n, const float4* __restrict__ pts, double inv_res, u64* __restrict__ table, u32 mask,
                                                        int* __restrict__ voxels) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  const u64 key = voxel_key_or_empty((double)p.x, (double)p.y, (double)p.z, inv_res);
  if (key == EMPTY_KEY) return;
  if (table_insert(table, mask, key)) atomicAdd(voxels, 1);
}

__global__ __launch_bounds__(256) void rs_rehash_kernel(u32 from_slots, const u64* __restrict__ from, u64* __restrict__ table, u32 mask) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= from_slots) return;
  const u64 key = from[i];
  if (key != EMPTY_KEY) (void)table_insert(table, mask, key);
}

// hypothesis base + j, j = lane: samples (3 source indices), status, pose; the round's count of j is cleared here
__global__ __launch_bounds__(256) void rs_hypothesis_kernel(int count, int base, u64 seed, int n_src, const float4* __restrict__ spts,
                                                            const float4* __restrict__ tpts, const int* __restrict__ nearest, double poly_error_thresh,
                                                            int dof, int* __restrict__ samples, int* __restrict__ status, double* __restrict__ poses,
                                                            int* __restrict__ counts) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= count) return;
  const u64 it = (u64)(base + j);
  int s[3], t[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    s[k] = (int)(sample_hash(seed, 3ull * it + (u64)k) % (u64)n_src);
    t[k] = nearest[s[k]];
    samples[3 * j + k] = s[k];
  }
  int st = ransac_pose::OK;
  double T[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  if (t[0] < 0 || t[1] < 0 || t[2] < 0) {
    st = ransac_pose::NO_MATCH;
  } else if (s[0] == s[1] || s[1] == s[2] || s[0] == s[2] || t[0] == t[1] || t[1] == t[2] || t[0] == t[2]) {
    st = ransac_pose::REPEATED;
  } else {
    double ps[9], pt[9];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float4 a = spts[s[k]], b = tpts[t[k]];
      ps[3 * k] = (double)a.x, ps[3 * k + 1] = (double)a.y, ps[3 * k + 2] = (double)a.z;
      pt[3 * k] = (double)b.x, pt[3 * k + 1] = (double)b.y, pt[3 * k + 2] = (double)b.z;
    }
    st = ransac_pose::solve_pose(ps, pt, poly_error_thresh, dof, T);
  }
  status[j] = st;
  counts[j] = 0;
#pragma unroll
  for (int k = 0; k < 12; k++) poses[12 * j + k] = T[k];
}

// block (x, y): source points [2048 x, 2048 x + 2048) against hypotheses [y * hyps_per_block, (y + 1) * hyps_per_block) of the round
template <bool IN_LDS>
__global__ __launch_bounds__(SC_BLOCK) void rs_score_kernel(int n, const float4* __restrict__ pts, const u64* __restrict__ table, u32 mask,
                                                            double inv_res, int count, int hyps_per_block, const double* __restrict__ poses,
                                                            const int* __restrict__ status, int* __restrict__ counts) {
  extern __shared__ u64 s_table[];
  if (IN_LDS) {
    for (u32 i = threadIdx.x; i <= mask; i += SC_BLOCK) s_table[i] = table[i];
    __syncthreads();
  }
  // a lane's points; a point that does not exist, or has a non-finite coordinate, is all NaN and fails the range test under every pose
  double px[SC_PPL], py[SC_PPL], pz[SC_PPL];
#pragma unroll
  for (int k = 0; k < SC_PPL; k++) {
    const int i = blockIdx.x * SC_TILE + k * SC_BLOCK + (int)threadIdx.x;
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool ok = i < n;
    if (ok) p = pts[i];
    ok = ok && isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    px[k] = ok ? (double)p.x : nan;
    py[k] = ok ? (double)p.y : nan;
    pz[k] = ok ? (double)p.z : nan;
  }
  const int h0 = blockIdx.y * hyps_per_block, h1 = min(count, h0 + hyps_per_block);
  for (int h = h0; h < h1; h++) {
    if (status[h] != 0) continue;  // (uniform: the whole block skips it)
    const double* __restrict__ T = poses + 12 * h;
    int hits = 0;
#pragma unroll
    for (int k = 0; k < SC_PPL; k++) {
      double qx, qy, qz;
      transform_point_d(T, px[k], py[k], pz[k], qx, qy, qz);
      const u64 key = voxel_key_or_empty(qx, qy, qz, inv_res);
      bool hit = false;
      if (key != EMPTY_KEY) {
        u32 slot = slot_of(key, mask);
        for (;;) {
          const u64 c = IN_LDS ? s_table[slot] : table[slot];
          if (c == key) {
            hit = true;
            break;
          }
          if (c == EMPTY_KEY) break;
          slot = (slot + 1u) & mask;
        }
      }
      hits += __popcll(__ballot(hit));
    }
    if ((threadIdx.x & 63) == 0 && hits > 0) atomicAdd(&counts[h], hits);
  }
}

struct FoldState {
  int stop_it, stop_count, best_it, best_count;  // -1 / 0 / -1 / -1 before the first ok hypothesis
  double stop_pose[12], best_pose[12];
};

__global__ void rs_init_state_kernel(FoldState* __restrict__ state) {
  if (threadIdx.x == 0) {
    state->stop_it = -1;
    state->stop_count = 0;
    state->best_it = -1;
    state->best_count = -1;
  }
}

// merges round [base, base + count) into the state: the smallest ok index whose count reaches stop_threshold (kept once found), and the ok index with
// the largest count, the smaller index among equals (a strict > against the earlier rounds keeps theirs)
__global__ __launch_bounds__(256) void rs_fold_kernel(int count, int base, double stop_threshold, const int* __restrict__ status,
                                                      const int* __restrict__ counts, const double* __restrict__ poses, FoldState* __restrict__ state) {
  __shared__ int s_stop[256], s_best[256], s_cnt[256];
  int stop = 0x7fffffff, best = 0x7fffffff, cnt = -1;
  for (int j = threadIdx.x; j < count; j += 256) {  // a lane's indices ascend
    if (status[j] != 0) continue;
    const int c = counts[j];
    if (stop == 0x7fffffff && (double)c >= stop_threshold) stop = j;
    if (c > cnt) {
      cnt = c;
      best = j;
    }
  }
  s_stop[threadIdx.x] = stop;
  s_best[threadIdx.x] = best;
  s_cnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const int o = threadIdx.x + w;
      s_stop[threadIdx.x] = min(s_stop[threadIdx.x], s_stop[o]);
      if (s_cnt[o] > s_cnt[threadIdx.x] || (s_cnt[o] == s_cnt[threadIdx.x] && s_best[o] < s_best[threadIdx.x])) {
        s_cnt[threadIdx.x] = s_cnt[o];
        s_best[threadIdx.x] = s_best[o];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (state->stop_it < 0 && s_stop[0] != 0x7fffffff) {
      state->stop_it = base + s_stop[0];
      state->stop_count = counts[s_stop[0]];
      for (int k = 0; k < 12; k++) state->stop_pose[k] = poses[12 * s_stop[0] + k];
    }
    if (s_cnt[0] > state->best_count) {  // (s_cnt[0] >= 0 exactly when the round holds an ok hypothesis)
      state->best_it = base + s_best[0];
      state->best_count = s_cnt[0];
      for (int k = 0; k < 12; k++) state->best_pose[k] = poses[12 * s_best[0] + k];
    }
  }
}

inline u32 pow2_at_least(uint64_t v) {
  u32 s = MIN_SLOTS;
  while ((uint64_t)s < v) s <<= 1;
  return s;
}

// occupancy set of `n` target points at 1 / inv_res; synchronises `st` once (the voxel count)
int build_table(glim_amd_ctx* ctx, hipStream_t st, const float4* pts, int n, double inv_res, Table* out) {
  int voxels = 0;
  DeviceTemp wide, d_voxels;
  SyncOnExit in_flight(st);
  u32 wide_slots = 0;
  if (n > 0) {
    wide_slots = pow2_at_least(2ull * (uint64_t)n);
    GA_HIP(pool_malloc(&wide.p, (size_t)wide_slots * sizeof(u64)));
    GA_HIP(pool_malloc(&d_voxels.p, sizeof(int)));
    rs_fill_kernel<<<(wide_slots + 255u) / 256u, 256, 0, st>>>(wide_slots, wide.as<u64>(), d_voxels.as<int>());
    rs_insert_kernel<<<(n + 255) / 256, 256, 0, st>>>(n, pts, inv_res, wide.as<u64>(), wide_slots - 1u, d_voxels.as<int>());
    GA_HIP(hipGetLastError());
    GA_HIP(read_back_sync(ctx, st, &voxels, d_voxels.p, sizeof(int)));
    if (voxels < 0 || voxels > n) return GLIM_AMD_ERR_STATE;
  }
  out->slots = pow2_at_least(2ull * (uint64_t)voxels);
  out->in_lds = (int)out->slots <= std::min(g_lds_slots_max, LDS_SLOTS_MAX) ? 1 : 0;
  GA_HIP(pool_malloc(&out->keys.p, (size_t)out->slots * sizeof(u64)));
  rs_fill_kernel<<<(out->slots + 255u) / 256u, 256, 0, st>>>(out->slots, out->keys.as<u64>(), nullptr);
  if (voxels > 0) rs_rehash_kernel<<<(wide_slots + 255u) / 256u, 256, 0, st>>>(wide_slots, wide.as<u64>(), out->keys.as<u64>(), out->slots - 1u);
  GA_HIP(hipGetLastError());
  GA_HIP(hipStreamSynchronize(st));  // `wide` goes back to the pool with this scope
  in_flight.dismiss();
  return GLIM_AMD_OK;
}

int RoundBuffers::alloc() {
  GA_HIP(pool_malloc(&samples.p, (size_t)ROUND * 3 * sizeof(int)));
  GA_HIP(pool_malloc(&status.p, (size_t)ROUND * sizeof(int)));
  GA_HIP(pool_malloc(&poses.p, (size_t)ROUND * 12 * sizeof(double)));
  GA_HIP(pool_malloc(&counts.p, (size_t)ROUND * sizeof(int)));
  GA_HIP(pool_malloc(&state.p, sizeof(FoldState)));
  return GLIM_AMD_OK;
}

inline void launch_hypotheses(const Pair& p, const glim_amd_ransac_params& prm, const RoundBuffers& b, int base, int count) {
  rs_hypothesis_kernel<<<(count + 255) / 256, 256, 0, p.st>>>(count, base, (u64)prm.seed, p.n_src, p.spts, p.tpts, p.d_nearest, prm.poly_error_thresh,
                                                               prm.dof, b.samples.as<int>(), b.status.as<int>(), b.poses.as<double>(),
                                                               b.counts.as<int>());
}
// the first `count` hypotheses of `b` against the table of voxels of edge `resolution` (ransac_table.hpp)
void launch_score(const Pair& p, double resolution, const Table& t, const RoundBuffers& b, int count) {
  const int tiles = (p.n_src + SC_TILE - 1) / SC_TILE;
  const int want = 4 * std::max(p.ctx->num_cus, 1);
  const int hpb = std::min(count, std::max(16, (int)(((int64_t)count * tiles + want - 1) / want)));
  const dim3 grid((unsigned)tiles, (unsigned)((count + hpb - 1) / hpb));
  const double inv_res = 1.0 / resolution;
  if (t.in_lds) {
    static const hipError_t lds_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&rs_score_kernel<true>),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, LDS_SLOTS_MAX * (int)sizeof(u64));
    (void)lds_ok;  // (a refusal shows as the launch error the caller checks)
    rs_score_kernel<true><<<grid, SC_BLOCK, (size_t)t.slots * sizeof(u64), p.st>>>(p.n_src, p.spts, t.keys.as<u64>(), t.slots - 1u, inv_res, count, hpb,
                                                                                   b.poses.as<double>(), b.status.as<int>(), b.counts.as<int>());
  } else {
    rs_score_kernel<false><<<grid, SC_BLOCK, 0, p.st>>>(p.n_src, p.spts, t.keys.as<u64>(), t.slots - 1u, inv_res, count, hpb, b.poses.as<double>(),
                                                        b.status.as<int>(), b.counts.as<int>());
  }
}
inline void launch_fold(const Pair& p, const glim_amd_ransac_params& prm, const RoundBuffers& b, int base, int count) {
  rs_fold_kernel<<<1, 256, 0, p.st>>>(count, base, prm.early_stop_inlier_rate * (double)p.n_src, b.status.as<int>(), b.counts.as<int>(),
                                      b.poses.as<double>(), b.state.as<FoldState>());
}

int check_params(const glim_amd_ransac_params* p) {
  if (!p) return GLIM_AMD_ERR_INVALID;
  if (p->dof != 4 && p->dof != 6) return GLIM_AMD_ERR_INVALID;
  if (p->max_iterations <= 0) return GLIM_AMD_ERR_INVALID;
  if (!std::isfinite(p->inlier_voxel_resolution) || !(p->inlier_voxel_resolution > 0.0)) return GLIM_AMD_ERR_INVALID;
  if (std::isnan(p->early_stop_inlier_rate) || std::isnan(p->poly_error_thresh)) return GLIM_AMD_ERR_INVALID;
  return GLIM_AMD_OK;
}

// the rounds; caller holds ctx->mu, the device is set, p.d_nearest is on the device, p.n_src >= 3, p.n_tgt >= 1
int run_rounds(const Pair& p, const glim_amd_ransac_params& prm, glim_amd_registration_result* result) {
  Table table;
  GA_TRY(build_table(p.ctx, p.st, p.tpts, p.n_tgt, 1.0 / prm.inlier_voxel_resolution, &table));
  RoundBuffers b;
  SyncOnExit in_flight(p.st);
  GA_TRY(b.alloc());
  rs_init_state_kernel<<<1, 64, 0, p.st>>>(b.state.as<FoldState>());
  FoldState h{};
  h.stop_it = h.best_it = -1;
  for (int base = 0; base < prm.max_iterations; base += ROUND) {
    const int count = std::min(ROUND, prm.max_iterations - base);
    launch_hypotheses(p, prm, b, base, count);
    launch_score(p, prm.inlier_voxel_resolution, table, b, count);
    launch_fold(p, prm, b, base, count);
    GA_HIP(hipGetLastError());
    GA_HIP(read_back_sync(p.ctx, p.st, &h, b.state.p, sizeof(FoldState)));
    if (h.stop_it >= 0) break;
  }
  in_flight.dismiss();  // (every round ended with a synchronise)
  if (h.stop_it < 0 && h.best_it < 0) {
    reg_detail::identity_result(result, prm.max_iterations);
    return GLIM_AMD_OK;
  }
  const bool stopped = h.stop_it >= 0;
  std::memcpy(result->T_target_source, stopped ? h.stop_pose : h.best_pose, 12 * sizeof(double));
  result->num_inliers = stopped ? h.stop_count : h.best_count;
  result->inlier_rate = (double)result->num_inliers / (double)p.n_src;
  result->best_iteration = stopped ? h.stop_it : h.best_it;
  result->iterations_run = stopped ? h.stop_it + 1 : prm.max_iterations;
  return GLIM_AMD_OK;
}

}  // namespace ransac_detail
}  // namespace glim_amd

extern "C" {

int glim_amd_ransac_default_params(glim_amd_ransac_params* params) {
  if (!params) return GLIM_AMD_ERR_INVALID;
  params->max_iterations = 5000;
  params->early_stop_inlier_rate = 0.9;
  params->poly_error_thresh = 0.5;
  params->inlier_voxel_resolution = 1.0;
  params->dof = 6;
  params->seed = 0;
  return GLIM_AMD_OK;
}

int glim_amd_ransac_align(const glim_amd_cloud* target, const glim_amd_cloud* source, const int32_t* nearest, const glim_amd_ransac_params* params,
                          glim_amd_registration_result* result) {
  using namespace glim_amd;
  using namespace glim_amd::ransac_detail;
  if (!result) return GLIM_AMD_ERR_INVALID;
  GA_TRY(reg_detail::check_pair(target, source));
  GA_TRY(check_params(params));
  GA_TRY(reg_detail::check_nearest(nearest, source->n, target->n));
  if (source->n < 3 || target->n == 0) {
    reg_detail::identity_result(result, params->max_iterations);
    return GLIM_AMD_OK;
  }
  return reg_detail::with_host_nearest(target, source, nearest, [&](const Pair& p) { return run_rounds(p, *params, result); });
}

int glim_amd_ransac_align_fpfh(const glim_amd_cloud* target, const glim_amd_cloud* source, const glim_amd_fpfh* target_fpfh,
                               const glim_amd_fpfh* source_fpfh, uint32_t match_flags, const glim_amd_ransac_params* params,
                               glim_amd_registration_result* result) {
  using namespace glim_amd;
  using namespace glim_amd::ransac_detail;
  if (!result) return GLIM_AMD_ERR_INVALID;
  GA_TRY(reg_detail::check_fpfh_pair(target, source, target_fpfh, source_fpfh, match_flags));
  GA_TRY(check_params(params));
  if (source->n < 3 || target->n == 0) {
    reg_detail::identity_result(result, params->max_iterations);
    return GLIM_AMD_OK;
  }
  return reg_detail::with_matched_nearest(target, source, target_fpfh, source_fpfh, match_flags,
                                          [&](const Pair& p) { return run_rounds(p, *params, result); });
}

int glim_amd_debug_ransac_max_lds_slots(int32_t slots) {
  using namespace glim_amd::ransac_detail;
  if (slots < 0) return GLIM_AMD_ERR_INVALID;
  g_lds_slots_max = std::min((int)slots, LDS_SLOTS_MAX);
  return GLIM_AMD_OK;
}

int glim_amd_ransac_debug_hypotheses(const glim_amd_cloud* target, const glim_amd_cloud* source, const int32_t* nearest,
                                     const glim_amd_ransac_params* params, int32_t first, int32_t count, int32_t* samples, int32_t* status,
                                     double* poses12, int32_t* inliers, int32_t* table_slots, int32_t* table_in_lds) {
  using namespace glim_amd;
  using namespace glim_amd::ransac_detail;
  GA_TRY(reg_detail::check_pair(target, source));
  GA_TRY(check_params(params));
  GA_TRY(reg_detail::check_nearest(nearest, source->n, target->n));
  if (first < 0 || count < 0 || (int64_t)first + count > (int64_t)0x7fffffff) return GLIM_AMD_ERR_INVALID;
  if (source->n == 0) return GLIM_AMD_ERR_INVALID;  // there is nothing to draw from
  return reg_detail::with_host_nearest(target, source, nearest, [&](const Pair& p) -> int {
    hipStream_t st = p.st;
    Table table;
    GA_TRY(build_table(p.ctx, st, p.tpts, p.n_tgt, 1.0 / params->inlier_voxel_resolution, &table));
    if (table_slots) *table_slots = (int32_t)table.slots;
    if (table_in_lds) *table_in_lds = table.in_lds;
    RoundBuffers b;
    SyncOnExit in_flight(st);
    GA_TRY(b.alloc());
    for (int done = 0; done < count; done += ROUND) {
      const int c = std::min(ROUND, (int)count - done);
      launch_hypotheses(p, *params, b, first + done, c);
      launch_score(p, params->inlier_voxel_resolution, table, b, c);
      GA_HIP(hipGetLastError());
      if (samples) GA_HIP(hipMemcpyAsync(samples + 3 * (size_t)done, b.samples.p, (size_t)c * 3 * sizeof(int), hipMemcpyDeviceToHost, st));
      if (status) GA_HIP(hipMemcpyAsync(status + done, b.status.p, (size_t)c * sizeof(int), hipMemcpyDeviceToHost, st));
      if (poses12) GA_HIP(hipMemcpyAsync(poses12 + 12 * (size_t)done, b.poses.p, (size_t)c * 12 * sizeof(double), hipMemcpyDeviceToHost, st));
      if (inliers) GA_HIP(hipMemcpyAsync(inliers + done, b.counts.p, (size_t)c * sizeof(int), hipMemcpyDeviceToHost, st));
      GA_HIP(hipStreamSynchronize(st));
    }
    in_flight.dismiss();
    return GLIM_AMD_OK;
  });
}

int glim_amd_ransac_profile(const glim_amd_cloud* target, const glim_amd_cloud* source, const int32_t* nearest, const glim_amd_ransac_params* params,
                            int iters, float* us_hypothesis, float* us_score, float* us_fold, int32_t* table_slots, int32_t* table_in_lds) {
  using namespace glim_amd;
  using namespace glim_amd::ransac_detail;
  GA_TRY(reg_detail::check_pair(target, source));
  GA_TRY(check_params(params));
  GA_TRY(reg_detail::check_nearest(nearest, source->n, target->n));
  if (iters <= 0 || source->n == 0) return GLIM_AMD_ERR_INVALID;
  return reg_detail::with_host_nearest(target, source, nearest, [&](const Pair& p) -> int {
    hipStream_t st = p.st;
    Table table;
    GA_TRY(build_table(p.ctx, st, p.tpts, p.n_tgt, 1.0 / params->inlier_voxel_resolution, &table));
    if (table_slots) *table_slots = (int32_t)table.slots;
    if (table_in_lds) *table_in_lds = table.in_lds;
    RoundBuffers b;
    SyncOnExit in_flight(st);
    GA_TRY(b.alloc());
    const int count = std::min(ROUND, (int)params->max_iterations);
    reg_detail::StageClock<4> clock;  // (its events go on every path, a failing start() included)
    GA_TRY(clock.start());
    double sum[3] = {0.0, 0.0, 0.0};
    int rc = GLIM_AMD_OK;
    for (int i = -2; i < iters && rc == GLIM_AMD_OK; i++) {  // two warm-up rounds
      rs_init_state_kernel<<<1, 64, 0, st>>>(b.state.as<FoldState>());
      clock.mark(0, st);
      launch_hypotheses(p, *params, b, 0, count);
      clock.mark(1, st);
      launch_score(p, params->inlier_voxel_resolution, table, b, count);
      clock.mark(2, st);
      launch_fold(p, *params, b, 0, count);
      clock.mark(3, st);
      if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = GLIM_AMD_ERR_HIP;
      for (int k = 0; k < 3 && rc == GLIM_AMD_OK && i >= 0; k++)
        if (clock.add_us(k, &sum[k]) != hipSuccess) rc = GLIM_AMD_ERR_HIP;
    }
    in_flight.dismiss();
    if (rc != GLIM_AMD_OK) return rc;
    if (us_hypothesis) *us_hypothesis = (float)(sum[0] / iters);
    if (us_score) *us_score = (float)(sum[1] / iters);
    if (us_fold) *us_fold = (float)(sum[2] / iters);
    return GLIM_AMD_OK;
  });
}

}  // extern "C"
