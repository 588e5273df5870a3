// overlap.hip -- the overlap query on gfx950 (kernel K6): the fraction of a source cloud's points that fall into an occupied voxel of ANY of a
// list of (voxel map, pose) targets.
//
// Replaces gtsam_points::overlap_gpu as called from src/glim/odometry/odometry_estimation_gpu.cpp:224-231, :248.
// Voxel coordinates are formed as in the factor kernels (vgicp.hip): q = R p + t in FP64 with a fixed fma order, exact 64-bit key compare
// (device_math.hpp transform_point_d, voxel_key, find_slot).
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "device_math.hpp"
#include "internal.hpp"

using namespace glim_amd;

// FP contraction as WRITTEN, as in vgicp.hip, where this code was compiled before it became a unit of its own
#pragma clang fp contract(on)

namespace {

constexpr int BLOCK = 256;

struct OverlapTarget {
  const VoxelBucket* buckets;
  unsigned int num_buckets;
  int pad;
  double inv_res;
  double T[12];
};
// One overlap query = one source cloud against a list of (map, delta) targets (odometry_estimation_gpu.cpp:224-231, :248).
struct OverlapQuery {
  const float4* pts;
  int n;
  int first_target, num_targets;
  int first_block, num_blocks;  // blocks [first_block, first_block + num_blocks) of the launch walk this query's points
  int lanes_shift;              // 2^lanes_shift consecutive lanes share a point and split its targets (overlap_kernel)
};
constexpr int OVERLAP_INLINE_TARGETS = 16;
struct OverlapInline {  // single-query call: everything in the kernel arguments, nothing to upload
  OverlapQuery q;
  OverlapTarget t[OVERLAP_INLINE_TARGETS];
};

// K6: a point counts once if ANY (map_j, delta_j) contains it.  One launch answers any number of queries; completion without a stream
// synchronise or a read-back copy: every block adds (1 << 32 | its hits) to its query's 64-bit counter with ONE returning atomic, the block
// that sees all the others' arrivals writes the query's total into host-mapped memory, resets the counter for the next call and -- when it
// also completes the last query -- publishes the call's sequence number, on which the host spins.
template <bool INLINE>
__global__ __launch_bounds__(BLOCK) void overlap_kernel(const OverlapInline in, const OverlapQuery* __restrict__ queries, const OverlapTarget* __restrict__ targets,
                                                         const int* __restrict__ block_query, int num_queries, unsigned long long* __restrict__ counters,
                                                         unsigned int* __restrict__ queries_done, unsigned int* __restrict__ h_hits,
                                                         unsigned int* __restrict__ h_flag, unsigned int seq) {
  __shared__ int s_tmp[16];
  const int qi = INLINE ? 0 : block_query[blockIdx.x];
  const OverlapQuery q = INLINE ? in.q : queries[qi];
  const OverlapTarget* tg = INLINE ? in.t : targets + q.first_target;
  // A point's targets are looked up by G = 2^lanes_shift CONSECUTIVE LANES at once (G = 16 for the odometry's 15-keyframe query) instead of one
  // lane walking them one after the other: a lookup is a dependent chain of memory latencies (key line, perhaps a spill), and fifteen of them in
  // sequence made the 15-target call of a 10 000-pt frame a 30 us kernel -- latency, not work.  Lane l of a group takes targets l, l + G, ...; the
  // group's verdict is a slice of the wavefront's ballot; the group's first lane counts the point.  Same count: "any target contains the point".
  int mine = 0;
  const int chunk = (int)blockIdx.x - q.first_block;
  const int shift = q.lanes_shift, G = 1 << shift, sub_lane = (int)threadIdx.x & (G - 1);
  const int lane = (int)threadIdx.x & 63, group_base = lane & ~(G - 1);
  const unsigned long long group_mask = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << group_base;
  const long long items = (long long)q.n << shift;  // (point, lane-of-group) pairs
  const int rounds = (q.num_targets + G - 1) >> shift;
  for (long long base = (long long)chunk * BLOCK; base < items; base += (long long)q.num_blocks * BLOCK) {  // (block-uniform trip count: ballots stay whole)
    const long long idx = base + (long long)threadIdx.x;
    const bool live = idx < items;
    const int i = live ? (int)(idx >> shift) : 0;
    const float4 p4 = q.pts[i];
    bool group_hit = false;
    for (int r = 0; r < rounds; r++) {
      const int t = (r << shift) + sub_lane;
      bool hit = false;
      if (live && !group_hit && t < q.num_targets) {
        double qx, qy, qz;
        transform_point_d(tg[t].T, (double)p4.x, (double)p4.y, (double)p4.z, qx, qy, qz);
        hit = find_slot(tg[t].buckets, tg[t].num_buckets, voxel_key(qx, qy, qz, tg[t].inv_res)) >= 0;
      }
      group_hit = group_hit || (__ballot(hit) & group_mask) != 0ull;
    }
    if (live && group_hit && sub_lane == 0) mine++;
  }
  const int block_hits = block_reduce_i<2>(mine, s_tmp);
  if (threadIdx.x == 0) {
    const unsigned long long prev = atomicAdd(counters + qi, (1ull << 32) | (unsigned long long)(unsigned int)block_hits);
    if ((int)(prev >> 32) == q.num_blocks - 1) {
      counters[qi] = 0ull;  // every block of this query has arrived: nobody touches the counter again in this launch
      h_hits[qi] = (unsigned int)prev + (unsigned int)block_hits;
      __threadfence_system();
      const unsigned int done = INLINE ? 0u : atomicAdd(queries_done, 1u);
      if (INLINE || (int)done == num_queries - 1) {
        if (!INLINE) *queries_done = 0u;
        __hip_atomic_store(h_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

int overlap_scratch(glim_amd_ctx* ctx, hipStream_t st) {
  if (ctx->ov_counters) return GLIM_AMD_OK;
  const size_t cbytes = (size_t)glim_amd_ctx::OV_MAX_QUERIES * sizeof(unsigned long long) + 64;
  GA_HIP(pool_malloc(&ctx->ov_counters, cbytes));
  GA_HIP(hipMemsetAsync(ctx->ov_counters, 0, cbytes, st));
  if (ctx->ov_host) return GLIM_AMD_OK;  // (the counters alone are re-made after a failed call: overlap_discard_counters)
  GA_HIP(pinned_malloc(&ctx->ov_host, (size_t)(1 + glim_amd_ctx::OV_MAX_QUERIES) * sizeof(unsigned int)));
  memset(ctx->ov_host, 0, (size_t)(1 + glim_amd_ctx::OV_MAX_QUERIES) * sizeof(unsigned int));
  if (!host_device_view(ctx->ov_host, &ctx->ov_host_dev)) return GLIM_AMD_ERR_HIP;
  return GLIM_AMD_OK;
}

// After a failed overlap launch / wait the arrival counters may be left non-zero, which would poison the next call's counts: wait for whatever
// did get enqueued and drop the block -- overlap_scratch hands the next call a freshly zeroed one.
void overlap_discard_counters(glim_amd_ctx* ctx, hipStream_t st) {
  (void)hipStreamSynchronize(st);
  (void)hipGetLastError();
  if (ctx->ov_counters) (void)pool_free(ctx->ov_counters);
  ctx->ov_counters = nullptr;
}

void fill_overlap_target(OverlapTarget& o, const glim_amd_voxelmap* m, const double* T12) {
  o.buckets = m->buckets;
  o.num_buckets = m->num_buckets;
  o.pad = 0;
  o.inv_res = m->inv_resolution;
  memcpy(o.T, T12, 12 * sizeof(double));
}

// blocks a query's points are spread over: one atomic per block ends the query, so few fat blocks (at most one per CU)
// lanes that share a point: the smallest power of two >= the number of targets, at most 16 (more targets take further rounds)
int overlap_lanes_shift(int num_targets) {
  int s = 0;
  while ((1 << s) < num_targets && s < 4) s++;
  return s;
}
int overlap_blocks(const glim_amd_ctx* ctx, int64_t n, int lanes_shift) {
  // two (point, lane) items per thread, at most two blocks per CU: one returning atomic per block ends the query
  const int64_t items = n << lanes_shift;
  return (int)std::max<int64_t>(1, std::min<int64_t>((items + 2 * BLOCK - 1) / (2 * BLOCK), 2 * std::max(1, ctx->num_cus)));
}

}  // namespace

extern "C" {

// One launch, no allocation, no copy, no stream synchronise: descriptors in the kernel arguments (single query, <= 16 targets) or read by the
// kernel from a pinned staging block (batches), results and the completion word in host-mapped memory.
int glim_amd_overlap_batch(glim_amd_ctx* ctx, int32_t num_queries, const int32_t* num_targets, const glim_amd_voxelmap* const* targets,
                           const double* T, const glim_amd_cloud* const* sources, double* overlaps) {
  if (!ctx || num_queries <= 0 || !num_targets || !targets || !T || !sources || !overlaps) return GLIM_AMD_ERR_INVALID;
  if (num_queries > glim_amd_ctx::OV_MAX_QUERIES) return GLIM_AMD_ERR_UNSUPPORTED;
  int64_t total_targets = 0;
  for (int q = 0; q < num_queries; q++) {
    if (num_targets[q] <= 0 || !sources[q] || sources[q]->ctx->device != ctx->device) return GLIM_AMD_ERR_INVALID;
    for (int t = 0; t < num_targets[q]; t++) {
      const glim_amd_voxelmap* m = targets[total_targets + t];
      if (!m || m->ctx->device != ctx->device) return GLIM_AMD_ERR_INVALID;
      if (!m->buckets) return GLIM_AMD_ERR_STATE;
    }
    total_targets += num_targets[q];
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  for (int64_t t = 0; t < total_targets; t++) GA_TRY(voxelmap_wait_ready(targets[t], st));  // (maps whose build the host has not seen complete)
  GA_TRY(overlap_scratch(ctx, st));
  // queries with an empty source are answered here (0.0) and take no part in the launch
  std::vector<int> live;
  for (int q = 0; q < num_queries; q++) {
    overlaps[q] = 0.0;
    if (sources[q]->n > 0) live.push_back(q);
  }
  if (live.empty()) return GLIM_AMD_OK;
  const unsigned int seq = ++ctx->ov_seq;
  std::vector<int64_t> first_target((size_t)num_queries);
  {
    int64_t acc = 0;
    for (int q = 0; q < num_queries; q++) {
      first_target[(size_t)q] = acc;
      acc += num_targets[q];
    }
  }
  const OverlapInline none{};
  if (live.size() == 1 && num_targets[live[0]] <= OVERLAP_INLINE_TARGETS) {
    const int q = live[0];
    OverlapInline in{};
    in.q.pts = sources[q]->pts;
    in.q.n = (int)sources[q]->n;
    in.q.first_target = 0;
    in.q.num_targets = num_targets[q];
    in.q.first_block = 0;
    in.q.lanes_shift = overlap_lanes_shift(num_targets[q]);
    in.q.num_blocks = overlap_blocks(ctx, sources[q]->n, in.q.lanes_shift);
    for (int t = 0; t < num_targets[q]; t++) fill_overlap_target(in.t[t], targets[first_target[(size_t)q] + t], T + 12 * (first_target[(size_t)q] + t));
    overlap_kernel<true><<<in.q.num_blocks, BLOCK, 0, st>>>(in, nullptr, nullptr, nullptr, 1, ctx->ov_counters, nullptr, ctx->ov_host_dev + 1, ctx->ov_host_dev, seq);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && !spin_until(ctx->ov_host, seq)) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
      set_hip_error(e, "overlap");
      overlap_discard_counters(ctx, st);
      return GLIM_AMD_ERR_HIP;
    }
    overlaps[q] = (double)ctx->ov_host[1] / (double)sources[q]->n;
    return GLIM_AMD_OK;
  }
  // batch: queries, targets and the block -> query table in one pinned block the kernel reads directly
  int total_blocks = 0;
  std::vector<OverlapQuery> hq(live.size());
  int64_t live_targets = 0;
  long long walking_blocks = 0;
  for (const int q : live) walking_blocks += overlap_blocks(ctx, sources[q]->n, 0);
  const bool batch_fills_device = walking_blocks >= (long long)std::max(1, ctx->num_cus);
  for (size_t i = 0; i < live.size(); i++) {
    const int q = live[i];
    hq[i].pts = sources[q]->pts;
    hq[i].n = (int)sources[q]->n;
    hq[i].first_target = (int)live_targets;
    hq[i].num_targets = num_targets[q];
    hq[i].first_block = total_blocks;
    // Spreading a point's targets over lanes trades work for latency: every target is looked up, where one lane walking them stops at the first
    // hit (keyframes overlap: two or three lookups per point on average).  A batch that fills the chip by itself (the 43-query keyframe elimination
    // loop: 860 blocks) is bound by that work, not by one query's latency -- 55-59 us walking, 92 us spread -- so only batches too small to fill
    // the device spread.
    hq[i].lanes_shift = batch_fills_device ? 0 : overlap_lanes_shift(num_targets[q]);
    hq[i].num_blocks = overlap_blocks(ctx, sources[q]->n, hq[i].lanes_shift);
    total_blocks += hq[i].num_blocks;
    live_targets += num_targets[q];
  }
  const size_t qbytes = hq.size() * sizeof(OverlapQuery), tbytes = (size_t)live_targets * sizeof(OverlapTarget), bbytes = (size_t)total_blocks * sizeof(int);
  char* stage = nullptr;
  GA_HIP(pinned_malloc(&stage, qbytes + tbytes + bbytes));
  char* stage_dev = nullptr;
  if (!host_device_view(stage, &stage_dev)) {
    (void)pinned_free(stage);
    return GLIM_AMD_ERR_HIP;
  }
  memcpy(stage, hq.data(), qbytes);
  OverlapTarget* ht = reinterpret_cast<OverlapTarget*>(stage + qbytes);
  int* hb = reinterpret_cast<int*>(stage + qbytes + tbytes);
  for (size_t i = 0; i < live.size(); i++) {
    const int q = live[i];
    for (int t = 0; t < num_targets[q]; t++)
      fill_overlap_target(ht[hq[i].first_target + t], targets[first_target[(size_t)q] + t], T + 12 * (first_target[(size_t)q] + t));
    for (int b = 0; b < hq[i].num_blocks; b++) hb[hq[i].first_block + b] = (int)i;
  }
  unsigned int* queries_done = reinterpret_cast<unsigned int*>(ctx->ov_counters + glim_amd_ctx::OV_MAX_QUERIES);
  overlap_kernel<false><<<total_blocks, BLOCK, 0, st>>>(none, reinterpret_cast<const OverlapQuery*>(stage_dev), reinterpret_cast<const OverlapTarget*>(stage_dev + qbytes),
                                                        reinterpret_cast<const int*>(stage_dev + qbytes + tbytes), (int)live.size(), ctx->ov_counters, queries_done,
                                                        ctx->ov_host_dev + 1, ctx->ov_host_dev, seq);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && !spin_until(ctx->ov_host, seq)) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    set_hip_error(e, "overlap_batch");
    overlap_discard_counters(ctx, st);  // (waits for the stream: the kernel reads `stage` directly)
    (void)pinned_free(stage);
    return GLIM_AMD_ERR_HIP;
  }
  (void)pinned_free(stage);
  for (size_t i = 0; i < live.size(); i++) overlaps[live[i]] = (double)ctx->ov_host[1 + i] / (double)sources[live[i]]->n;
  return GLIM_AMD_OK;
}

int glim_amd_overlap_profile(glim_amd_ctx* ctx, int32_t num_queries, const int32_t* num_targets, const glim_amd_voxelmap* const* targets, const double* T,
                             const glim_amd_cloud* const* sources, int iters, float* us_per_call) {
  if (!ctx || num_queries <= 0 || iters <= 0 || !us_per_call) return GLIM_AMD_ERR_INVALID;
  std::vector<double> ov((size_t)num_queries);
  for (int i = 0; i < 5; i++) GA_TRY(glim_amd_overlap_batch(ctx, num_queries, num_targets, targets, T, sources, ov.data()));
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < iters; i++) GA_TRY(glim_amd_overlap_batch(ctx, num_queries, num_targets, targets, T, sources, ov.data()));
  const auto t1 = std::chrono::steady_clock::now();
  *us_per_call = (float)(std::chrono::duration<double, std::micro>(t1 - t0).count() / iters);
  return GLIM_AMD_OK;
}

int glim_amd_overlap(glim_amd_ctx* ctx, int32_t num_targets, const glim_amd_voxelmap* const* targets, const double* T,
                     const glim_amd_cloud* source, double* overlap) {
  if (!source || !overlap) return GLIM_AMD_ERR_INVALID;
  return glim_amd_overlap_batch(ctx, 1, &num_targets, targets, T, &source, overlap);
}

}  // extern "C"
