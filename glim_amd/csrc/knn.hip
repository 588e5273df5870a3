// knn.hip -- kernel group K2: exact k-nearest-neighbour search on the device.
// Replaces CloudPreprocessor::find_neighbors (src/glim/preprocess/cloud_preprocessor.cpp:190-221, a nanoflann kd-tree):
// for every point the k nearest points among ALL points including itself, ascending
// squared distance; ties are ordered by ascending index (the oracle's rule; the reference leaves exact ties to the kd-tree).
//
// Distances are evaluated in FP64 as (dx*dx + dy*dy) + dz*dz on the FP32-representable inputs -- the same expression, in
// the same order and without fma contraction, as oracle/vgicp_oracle.c:sqdist3 -- so neighbour lists are bit-identical.
//
// Two implementations, same result:
//   * curve-ordered chunks (knn_curve; every cloud above 2 048 points): Hilbert sort, 64-point chunks with boxes, a wavefront per one or two
//     queries whose lanes are the candidates of the chunk it scans (knn_qgroup.hip); adapts to the local density by construction.
//     0.23 ms for a 131 072-point LiDAR scan, 0.44 ms for a 307 104-point depth frame on MI355X.
//   * exhaustive (diag knn_path=brute): LDS-tiled scan of every point.  Answers clouds up to 2 048 points and clouds of astronomic extent, and
//     is the on-device cross-check of the other one: independent in method, milliseconds at test sizes.
//
// Measured and retired (git log has the code).  Three more implementations answered before the query-group kernel and were kept beside it as
// cross-checks until nothing called them:
//   * a hashed uniform grid (knn_path=grid): counting sort into cells, ring walk per query with an exactness bound and coarser retry levels.
//     0.85 / 1.11 ms at the two sizes above, 0.5 ... 5.5 ms on 10 000 ... 32 768-point clouds of uneven density
//     (profiles/r03/probe/knn_small_clouds.txt).  What bounded it: a wavefront lasts as long as its slowest lane, and the cells next to the
//     sensor hold 4000 candidates (p99) against a mean of 278; more lanes per query, a directly addressed grid and finer start levels were
//     all slower, four loads in flight and skipping cells beyond the k-th best were what helped (1.3 -> 0.86 ms).
//   * a 64-query chunk kernel (knn_kernel=wave64, knn_chunks.hip) with a per-lane threshold selection (knn_select) and a pair-lane kernel over
//     32-point half chunks (knn_kernel=pair, knn_pairs.hip): a query per LANE, candidate chunks streamed through LDS.  Both tail-bound -- the
//     launch lasts as long as its slowest wavefront, twice the mean at 131 072 points -- and a 10 000-point cloud fills 313 of 1 024 SIMDs
//     (profiles/r02/probe/knn_select_groupbox_ab.txt, knn_chunk_variants_ab.txt; profiles/r03/probe/knn_heavy_split_*.txt).
//   The query-group kernel against the faster of them, per call on one box: 10 000 points 0.294 -> 0.112 ms, 32 768 0.381 -> 0.167,
//   65 536 0.267 -> 0.169, 131 072 0.305 -> 0.233, 307 104 0.551 -> 0.437 ms (profiles/r04/probe/knn_qgroup.txt).
#include <algorithm>
#include <chrono>
#include <cstdio>

#include "knn_common.hpp"

using namespace glim_amd;

// measurement hook (glim_amd_cloud_profile_neighbors): when set, the calling thread's next kNN records these events around its query-group kernel
static thread_local hipEvent_t g_knn_probe_events[2] = {nullptr, nullptr};


namespace {

constexpr int TILE = 1024;

// ---- exhaustive scan.  `queries` (optional): list of point indices to answer; otherwise every point. ----
template <int K>
__global__ __launch_bounds__(256) void knn_bruteforce_kernel(int n, const float4* __restrict__ pts, int k, int32_t* __restrict__ out,
                                                             const int* __restrict__ queries, int num_queries) {
  __shared__ double s_x[TILE], s_y[TILE], s_z[TILE];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = t < num_queries;
  const int i = live ? (queries ? queries[t] : t) : 0;
  double qx = 0, qy = 0, qz = 0;
  if (live) {
    const float4 p = pts[i];
    qx = p.x; qy = p.y; qz = p.z;
  }
  TopK<K> best;
  best.init(i);
  for (int t0 = 0; t0 < n; t0 += TILE) {
    const int tn = min(TILE, n - t0);
    __syncthreads();
    for (int j = threadIdx.x; j < tn; j += blockDim.x) {
      const float4 p = pts[t0 + j];
      s_x[j] = p.x; s_y[j] = p.y; s_z[j] = p.z;
    }
    __syncthreads();
    if (live)
      for (int j = 0; j < tn; j++) best.push(sqdist(qx, qy, qz, s_x[j], s_y[j], s_z[j]), t0 + j);
  }
  if (live) {
    const int valid = min(n, K);
#pragma unroll
    for (int j = 0; j < K; j++)
      if (j < k) out[(size_t)i * k + j] = (j < valid) ? best.idx[j] : 0;  // fewer than k points: the reference's result vector stays 0 there (:193, :200)
  }
}

// bounding box by ordered-int atomics: bb[0..2] = min, bb[3..5] = max (as order-preserving ints)
__device__ __forceinline__ int ordered(float f) {
  const int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__global__ __launch_bounds__(256) void bbox_kernel(int n, const float4* __restrict__ pts, int* __restrict__ bb) {
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 p = pts[i];
    const int v[3] = {ordered(p.x), ordered(p.y), ordered(p.z)};
    for (int a = 0; a < 3; a++) {
      lo[a] = min(lo[a], v[a]);
      hi[a] = max(hi[a], v[a]);
    }
  }
  // one set of atomics per BLOCK (same-address atomics serialise in L2)
  __shared__ int s_tmp[16];
  for (int a = 0; a < 3; a++) {
    lo[a] = block_reduce_i<0>(lo[a], s_tmp);
    hi[a] = block_reduce_i<1>(hi[a], s_tmp);
  }
  if (threadIdx.x == 0)
    for (int a = 0; a < 3; a++) {
      atomicMin(&bb[a], lo[a]);
      atomicMax(&bb[3 + a], hi[a]);
    }
}
__host__ __device__ inline float unordered(int i) {
  const int j = i >= 0 ? i : i ^ 0x7fffffff;
  float f;
  memcpy(&f, &j, sizeof(f));
  return f;
}

template <int K>
void launch_brute(hipStream_t st, int n, const float4* pts, int k, int32_t* out, const int* queries, int nq) {
  if (nq > 0) knn_bruteforce_kernel<K><<<(nq + 255) / 256, 256, 0, st>>>(n, pts, k, out, queries, nq);
}

// =================================================================================================================
// Curve-ordered chunks: no grid, no rings.
//   1. the points are sorted along a Hilbert curve through the bounding box (stable radix sort, sort.hip);
//   2. every 64 consecutive points form a chunk with an axis-aligned box;
//   3. a wavefront answers one or two consecutive queries (knn_qgroup.hip): it scans candidate chunks, one coalesced load each -- first the
//      queries' own chunk and its two curve neighbours, which already contain most true neighbours, then every other chunk whose box can
//      still hold a point closer than some query's current k-th best.  A chunk is skipped only when the gap between the query and the
//      chunk's box is strictly larger than that query's k-th best distance, so nothing that could enter (or tie into) a top-k list is missed:
//      the result is exact for any point distribution, with the same (distance, index) order as the exhaustive kernel.
// Work per query adapts to the local density by construction (a chunk is 64 points wherever they are).
// =================================================================================================================
__device__ __forceinline__ unsigned long long spread3(unsigned int v) {  // 21 bits -> every third bit
  unsigned long long x = v & 0x1fffffu;
  x = (x | (x << 32)) & 0x1f00000000ffffull;
  x = (x | (x << 16)) & 0x1f0000ff0000ffull;
  x = (x | (x << 8)) & 0x100f00f00f00f00full;
  x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
  x = (x | (x << 2)) & 0x1249249249249249ull;
  return x;
}

// stats[1] counts points with a non-finite coordinate (an error).  The bounding box (bbox_kernel's ordered ints) is read
// HERE, not by the host: one synchronise per kNN call instead of two.  stats[2] is the guard word of the query-group kernel: 1 = the box is not
// finite, 2 = the cloud spans 1e18 m or more (the FP32 chunk test needs finite FP32 squared distances: the exhaustive FP64 kernel answers).
__global__ __launch_bounds__(256) void curve_key_kernel(int n, const float4* __restrict__ pts, const int* __restrict__ bb, unsigned int qmax, int bits,
                                                        unsigned long long* __restrict__ keys, int* __restrict__ stats) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float lox = unordered(bb[0]), loy = unordered(bb[1]), loz = unordered(bb[2]);
  const float ext = fmaxf(fmaxf(unordered(bb[3]) - lox, unordered(bb[4]) - loy), unordered(bb[5]) - loz);
  const bool finite_box = ext >= 0.f && isfinite(ext) && isfinite(lox) && isfinite(loy) && isfinite(loz);
  if (i == 0 && !(finite_box && ext < 1e18f)) stats[2] = finite_box ? 2 : 1;
  if (i >= n) return;
  const float scale = (finite_box && ext > 0.f) ? (float)qmax / ext : 0.f;
  const float4 p = pts[i];
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) {
    atomicAdd(&stats[1], 1);
    keys[i] = ~0ull;
    return;
  }
  const unsigned int x = min(qmax, (unsigned int)fmaxf(0.f, (p.x - lox) * scale));
  const unsigned int y = min(qmax, (unsigned int)fmaxf(0.f, (p.y - loy) * scale));
  const unsigned int z = min(qmax, (unsigned int)fmaxf(0.f, (p.z - loz) * scale));
  // Hilbert index (Skilling's axes-to-transpose): consecutive points of a Hilbert curve are always in adjacent cells, so 64
  // consecutive points form a compact chunk.  A Morton curve jumps at octant boundaries: it gave chunks 28 m across whose lanes
  // wanted different candidate sets (one wavefront 985 us against a mean of 170 us); the order only affects speed, never results.
  unsigned int X[3] = {x, y, z};
  const unsigned int M = 1u << (bits - 1);
  for (unsigned int Q = M; Q > 1u; Q >>= 1) {
    const unsigned int P = Q - 1u;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      if (X[a] & Q) {
        X[0] ^= P;
      } else {
        const unsigned int t = (X[0] ^ X[a]) & P;
        X[0] ^= t;
        X[a] ^= t;
      }
    }
  }
  X[1] ^= X[0];
  X[2] ^= X[1];
  unsigned int t = 0u;
  for (unsigned int Q = M; Q > 1u; Q >>= 1)
    if (X[2] & Q) t ^= Q - 1u;
  X[0] ^= t;
  X[1] ^= t;
  X[2] ^= t;
  keys[i] = spread3(X[2]) | (spread3(X[1]) << 1) | (spread3(X[0]) << 2);
}

// one wavefront per chunk: points in curve order (xyz + original index, index -1 and +inf coordinates past the end) and the chunk boxes
__global__ __launch_bounds__(256) void curve_gather_kernel(int n, int C, const float4* __restrict__ pts, const unsigned int* __restrict__ order,
                                                           float4* __restrict__ sorted, float* __restrict__ box /* [C][6] */,
                                                           float* __restrict__ box32 /* [2 C][6] or null */, unsigned int* __restrict__ rank) {
  const int c = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (c >= C) return;
  const int s = c * CHUNK + lane;
  const float inf = __int_as_float(0x7f800000);
  float4 q = make_float4(inf, inf, inf, __int_as_float(-1));
  if (s < n) {
    const unsigned int i = order[s];
    const float4 p = pts[i];
    q = make_float4(p.x, p.y, p.z, __int_as_float((int)i));
    if (rank) rank[i] = (unsigned int)s;
  }
  sorted[s] = q;
  float lo[3] = {q.x, q.y, q.z}, hi[3] = {s < n ? q.x : -inf, s < n ? q.y : -inf, s < n ? q.z : -inf};
  // xor offsets <= 16 stay inside a 32-lane half: the boxes of the two 32-point half chunks (box32[2 c + half], for a caller that wants
  // them; knn_curve passes null) fall out of the same butterfly, one step before the chunk's own box
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, 64));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, 64));
    }
  if (box32 && (lane & 31) == 0) {
    const int h = 2 * c + (lane >> 5);
#pragma unroll
    for (int a = 0; a < 3; a++) {
      box32[6 * h + a] = lo[a];
      box32[6 * h + 3 + a] = hi[a];
    }
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = fminf(lo[a], __shfl_xor(lo[a], 32, 64));
    hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], 32, 64));
  }
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      box[6 * c + a] = lo[a];
      box[6 * c + 3 + a] = hi[a];
    }
  }
}

// bounding-box accumulator (init_bbox_kernel's values) and the four status words of a kNN call, in one launch
__global__ void knn_scratch_init_kernel(int* __restrict__ bb, int* __restrict__ stats) {
  if (threadIdx.x < 6) bb[threadIdx.x] = threadIdx.x < 3 ? 0x7fffffff : (int)0x80000000;
  if (threadIdx.x < 4) stats[threadIdx.x] = 0;
}

int knn_curve(glim_amd_ctx* ctx, hipStream_t st, int n, const float4* pts, int k, int32_t* out, unsigned int* rank) {
  DeviceTemp bb, ka, kb, va, vb, hist, sorted, box, stats, dbg;  // (all returned to the pool after the synchronise at the end)
  SyncOnExit in_flight(st);  // an early return after the first launch waits for the stream before the scratch above goes back to the pool
  const int C = (n + CHUNK - 1) / CHUNK;
  GA_HIP(pool_malloc(&bb.p, 6 * sizeof(int)));
  GA_HIP(pool_malloc(&ka.p, (size_t)n * sizeof(unsigned long long)));
  GA_HIP(pool_malloc(&kb.p, (size_t)n * sizeof(unsigned long long)));
  GA_HIP(pool_malloc(&va.p, (size_t)n * sizeof(unsigned int)));
  GA_HIP(pool_malloc(&vb.p, (size_t)n * sizeof(unsigned int)));
  GA_HIP(pool_malloc(&hist.p, radix_sort_scratch_bytes(n)));
  GA_HIP(pool_malloc(&sorted.p, (size_t)C * CHUNK * sizeof(float4)));
  GA_HIP(pool_malloc(&box.p, ((size_t)C + (size_t)(C + CHUNK - 1) / CHUNK) * 6 * sizeof(float)));  // chunk boxes, then the boxes of the groups of 64 chunks
  GA_HIP(pool_malloc(&stats.p, 4 * sizeof(int)));
  knn_scratch_init_kernel<<<1, 64, 0, st>>>(bb.as<int>(), stats.as<int>());
  bbox_kernel<<<std::max(1, std::min((n + 2047) / 2048, 128)), 256, 0, st>>>(n, pts, bb.as<int>());
  const int bits = n < 32768 ? 8 : 13;  // per axis: 24-bit keys / 3 sort passes for small clouds, 39 bits / 5 passes otherwise; the order only affects speed
  const unsigned int qmax = (1u << bits) - 1u;
  curve_key_kernel<<<(n + 255) / 256, 256, 0, st>>>(n, pts, bb.as<int>(), qmax, bits, ka.as<unsigned long long>(), stats.as<int>());
  unsigned long long* ks = nullptr;
  unsigned int* order = nullptr;
  GA_HIP(radix_sort_pairs(st, n, 3 * bits, ka.as<unsigned long long>(), va.as<unsigned int>(), kb.as<unsigned long long>(), vb.as<unsigned int>(), true,
                          hist.as<int>(), &ks, &order));
  constexpr int DBG_INTS = 8;  // diag knn_debug: the query-group kernel's 5 counters over the launch, padded
  if (k > 0 && ctx->diag.knn_debug[0]) {
    GA_HIP(pool_malloc(&dbg.p, DBG_INTS * sizeof(int)));
    GA_HIP(hipMemsetAsync(dbg.p, 0, DBG_INTS * sizeof(int), st));
  }
  curve_gather_kernel<<<(C * CHUNK + 255) / 256, 256, 0, st>>>(n, C, pts, order, sorted.as<float4>(), box.as<float>(), nullptr, rank);
  // A wavefront answers 1 (clouds below 49 152 points) or 2 consecutive queries -- n or n / 2 short independent work items, so there is no
  // tail and small clouds fill the chip.  Four queries per wavefront share more of the walk but need 82 registers (5 wavefronts per SIMD
  // instead of 8): 0.252 / 0.466 ms at 131 072 / 307 104 points against 0.233 / 0.437 (profiles/r04/probe/knn_qgroup.txt).
  // The kernel's FP32 chunk test needs finite FP32 squared distances (3 ext^2 < FLT_MAX): it stands down on the guard word, and a cloud that
  // spans more than 1e18 m is answered by the exhaustive FP64 kernel below.
  if (k > 0) {  // k == 0: ordering only
    if (g_knn_probe_events[0]) (void)hipEventRecord(g_knn_probe_events[0], st);  // (glim_amd_cloud_profile_neighbors: HIP events around the dominant kernel)
    knn_launch_qgroup(st, n, C, sorted.as<float4>(), box.as<float>(), k, out, stats.as<int>() + 2, n < 49152 ? 1 : 2, dbg.as<int>());
    if (g_knn_probe_events[1]) (void)hipEventRecord(g_knn_probe_events[1], st);
  }
  GA_HIP(hipGetLastError());
  if (dbg.p) {
    int hd[DBG_INTS];
    GA_HIP(hipStreamSynchronize(st));  // (the context's streams do not synchronise with the null stream the copy below runs on)
    GA_HIP(hipMemcpy(hd, dbg.p, sizeof(hd), hipMemcpyDeviceToHost));
    if (FILE* f = fopen(ctx->diag.knn_debug, "wb")) {
      fwrite(hd, sizeof(int), DBG_INTS, f);
      fclose(f);
    }
  }
  int h_stats[4];
  GA_HIP(read_back_sync(ctx, st, h_stats, stats.p, sizeof(h_stats)));
  in_flight.dismiss();  // synchronised
  if (h_stats[1] != 0 || h_stats[2] == 1) return GLIM_AMD_ERR_RANGE;
  if (h_stats[2] == 2 && k > 0) {  // astronomic extent: the query-group kernel stood down
    DISPATCH_K(launch_brute, st, n, pts, k, out, (const int*)nullptr, n);
    GA_HIP(hipGetLastError());
    GA_HIP(hipStreamSynchronize(st));
  }
  return GLIM_AMD_OK;
}

}  // namespace

namespace glim_amd {

// Hilbert rank of every point of a cloud that has none yet (clouds whose neighbours came from the host or from the exhaustive kernel).
// Caller holds held->mu (the cloud's owner may be another context: its mutex is NOT held, so nothing of c->ctx is touched here).  Clouds with non-finite points simply stay in arrival order, and so do clouds below 32 768 points: sorting a cloud
// ONLY for its rank costs 70 us at 10 000 points, which GLIM's odometry would pay for every frame (the frame arrives with CPU covariances,
// so no kNN runs here whose by-product the rank would be) to gain 0.5 us per 34-factor linearisation
// (`bench.py --workload odometry_frame`, create_frame_us.factor_streams_on_first_use: 115 -> 44 us).
int cloud_curve_rank(glim_amd_cloud* c, glim_amd_ctx* held, hipStream_t st) {
  if (c->curve_rank || c->n < 32768 || c->n > (int64_t)(1 << 28) || !held->diag.curve_order) return GLIM_AMD_OK;
  GA_HIP(pool_malloc(&c->curve_rank, (size_t)c->n * sizeof(unsigned int)));
  const int rc = knn_curve(held, st, (int)c->n, c->pts, 0, nullptr, c->curve_rank);
  if (rc != GLIM_AMD_OK) {
    (void)pool_free(c->curve_rank);
    c->curve_rank = nullptr;
  }
  return rc == GLIM_AMD_ERR_RANGE ? GLIM_AMD_OK : rc;
}

}  // namespace glim_amd

extern "C" {

// Timing aid (bench.py rooflines of the kNN-led workloads): `iters` find_neighbors calls; wall milliseconds per call and the HIP-event duration of
// the query-group kernel inside it (0 when another kernel answered: clouds <= 2 048 points, forced paths).
int glim_amd_cloud_profile_neighbors(glim_amd_cloud* c, int k, int iters, float* ms_per_call, float* ms_qgroup_kernel) {
  if (!c || iters <= 0) return GLIM_AMD_ERR_INVALID;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  GA_HIP(hipSetDevice(c->ctx->device));
  GA_HIP(hipEventCreate(&e0));
  GA_HIP(hipEventCreate(&e1));
  int rc = glim_amd_cloud_find_neighbors(c, k, nullptr);  // warm-up (allocations, first-use paths)
  double kernel_ms = 0.0;
  int timed = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < iters && rc == GLIM_AMD_OK; i++) {
    g_knn_probe_events[0] = e0;
    g_knn_probe_events[1] = e1;
    rc = glim_amd_cloud_find_neighbors(c, k, nullptr);
    g_knn_probe_events[0] = g_knn_probe_events[1] = nullptr;
    float ms = 0.f;
    if (rc == GLIM_AMD_OK && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) {
      kernel_ms += ms;
      timed++;
    }
    (void)hipGetLastError();
  }
  const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc != GLIM_AMD_OK) return rc;
  if (ms_per_call) *ms_per_call = (float)(wall_ms / iters);
  if (ms_qgroup_kernel) *ms_qgroup_kernel = timed ? (float)(kernel_ms / timed) : 0.f;
  return GLIM_AMD_OK;
}

int glim_amd_cloud_find_neighbors(glim_amd_cloud* c, int k, int32_t* neighbors_out) {
  if (!c || k <= 0) return GLIM_AMD_ERR_INVALID;
  if (k > 32) return GLIM_AMD_ERR_UNSUPPORTED;
  glim_amd_ctx* ctx = c->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  if (c->neighbors) {
    (void)pool_free(c->neighbors);
    c->neighbors = nullptr;
  }
  c->k = k;
  GA_HIP(pool_malloc(&c->neighbors, (size_t)(c->n > 0 ? c->n : 1) * k * sizeof(int32_t)));
  if (c->n == 0) return GLIM_AMD_OK;
  if (c->n > (int64_t)(1 << 28)) return GLIM_AMD_ERR_INVALID;
  const int n = (int)c->n;
  hipStream_t st = ctx->stream();
  const Diag& diag = ctx->diag;
  const bool brute = n <= 2048 || n <= 2 * k || diag.knn_path == KNN_PATH_BRUTE;
  if (brute) {
    DISPATCH_K(launch_brute, st, n, c->pts, k, c->neighbors, (const int*)nullptr, n);
    GA_HIP(hipGetLastError());
  } else {
    // the Hilbert rank of every point is kept: estimate_covariances writes the factor's plane-form stream in that order
    if (!c->curve_rank && diag.curve_order) GA_HIP(pool_malloc(&c->curve_rank, (size_t)n * sizeof(unsigned int)));
    GA_TRY(knn_curve(ctx, st, n, c->pts, k, c->neighbors, c->curve_rank));
  }
  if (neighbors_out) GA_HIP(hipMemcpyAsync(neighbors_out, c->neighbors, (size_t)n * k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  return GLIM_AMD_OK;
}

}  // extern "C"
