// ivox.hip -- the device iVox: gtsam_points::IncrementalVoxelMap<FlatContainer> (gtsam_points::iVox), the incremental target model of GLIM's
// LiDAR-only continuous-time odometry (odometry_estimation_ct.cpp:56-63 creates it, :229-235 inserts every finished frame).  The container and
// its insert; the map object itself and its description as a target are ivox_map.hpp's, and the factors over the map are gicp.hip's.
//
// Semantics (upstream recall; include/glim_amd.h states them in full): a voxel is floor(p / leaf) of the STORED (FP32) point; insert takes the
// points in input order, a new voxel is appended in first-seen order, a cell drops a point when it is full or when a point already in it is
// closer than min_dist_in_cell (strict, FP64 (dx^2 + dy^2) + dz^2), every touched voxel's lru becomes the insert counter, and every
// lru_clear_cycle inserts the voxels with lru + lru_horizon < counter are removed, survivors keeping their order.
//
// Layout: an open-addressing table (key -> slot, linear probing, load <= 1/2) and per-slot arrays in structure-of-arrays form -- key, count,
// lru, and `cap` = max_num_points_in_cell entries of points (float4: xyz + the entry's own position slot * cap + place as int bits, which is
// what the factor kernels report as correspondence) and covariances (float4 + float2, the clouds' form).  Slot order IS upstream's voxel order.
//
// Parallel insert that equals the sequential one: key every point (pose applied in FP64, rounded to FP32, R C R^T in FP32), stable radix sort of
// (key, input index) (sort.hip), run heads look their voxel up; the new voxels are ranked by the input index of their first point (scan.hpp),
// which is their first-seen order, and claim slots behind the existing ones; then ONE WAVEFRONT PER RUN: lane l holds the cell's l-th stored
// point, the run's candidates are walked in input order, the rejection test is one distance per lane and a wave-wide ballot, an accepted
// point is written by the lane that owns the next place, and the wavefront leaves when the cell is full.  No atomics touch point data (the
// table claim is a compare-and-swap on distinct keys, the point total an integer sum): the map does not depend on scheduling.
// Eviction compacts the surviving slots in order into fresh arrays and rebuilds the table.  Every call returns with the stream idle.
#include <algorithm>
#include <cmath>
#include <vector>

#include "device_math.hpp"
#include "internal.hpp"
#include "ivox_map.hpp"
#include "scan.hpp"
#include "scope_sync.hpp"

using namespace glim_amd;

namespace {

struct IvoxPose {
  double T[12];
};

// stored point, covariance and voxel key of every input point
__global__ __launch_bounds__(256) void ivox_key_kernel(int n, const float4* __restrict__ pts, const float4* __restrict__ cA, const float2* __restrict__ cB,
                                                       int has_T, const IvoxPose P, double inv_leaf, float4* __restrict__ opts, float4* __restrict__ oA,
                                                       float2* __restrict__ oB, u64* __restrict__ key) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float4 p = pts[i];
  float4 a = cA[i];
  float2 b = cB[i];
  if (has_T) {
    const double* T = P.T;
    const double x = p.x, y = p.y, z = p.z;
    p.x = (float)dadd(dadd(dadd(dmul(T[0], x), dmul(T[1], y)), dmul(T[2], z)), T[3]);
    p.y = (float)dadd(dadd(dadd(dmul(T[4], x), dmul(T[5], y)), dmul(T[6], z)), T[7]);
    p.z = (float)dadd(dadd(dadd(dmul(T[8], x), dmul(T[9], y)), dmul(T[10], z)), T[11]);
    const float R[9] = {(float)T[0], (float)T[1], (float)T[2], (float)T[4], (float)T[5], (float)T[6], (float)T[8], (float)T[9], (float)T[10]};
    const float Cm[9] = {a.x, a.y, a.z, a.y, a.w, b.x, a.z, b.x, b.y};
    float W[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int k = 0; k < 3; k++) W[3 * r + k] = R[3 * r] * Cm[k] + R[3 * r + 1] * Cm[3 + k] + R[3 * r + 2] * Cm[6 + k];
    float M[6];
    const int mr[6] = {0, 0, 0, 1, 1, 2}, mc[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
    for (int u = 0; u < 6; u++) M[u] = W[3 * mr[u]] * R[3 * mc[u]] + W[3 * mr[u] + 1] * R[3 * mc[u] + 1] + W[3 * mr[u] + 2] * R[3 * mc[u] + 2];
    a = make_float4(M[0], M[1], M[2], M[3]);
    b = make_float2(M[4], M[5]);
  }
  p.w = 1.0f;
  opts[i] = p;
  oA[i] = a;
  oB[i] = b;
  const double t[3] = {(double)p.x * inv_leaf, (double)p.y * inv_leaf, (double)p.z * inv_leaf};
  bool valid = true;
#pragma unroll
  for (int q = 0; q < 3; q++) valid = valid && (t[q] >= -1048576.0 && t[q] < 1048576.0);  // false for NaN / inf: the point is skipped
  u64 k = EMPTY_KEY;
  if (valid) {
    const u64 c0 = (u64)(fast_floor_d(t[0]) + KEY_OFFSET), c1 = (u64)(fast_floor_d(t[1]) + KEY_OFFSET), c2 = (u64)(fast_floor_d(t[2]) + KEY_OFFSET);
    k = c0 | (c1 << 21) | (c2 << 42);
  }
  key[i] = k;
}

// run heads of the sorted order: the voxel's slot, or -1 and a mark at the input index of the run's first point (a new voxel); -2 elsewhere
__global__ __launch_bounds__(256) void ivox_head_kernel(int n, const u64* __restrict__ ks, const u32* __restrict__ order, const u64* __restrict__ tkeys,
                                                        const int* __restrict__ tslots, u32 mask, int* __restrict__ run_slot, int* __restrict__ newflag) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const u64 k = ks[j];
  if (k == EMPTY_KEY || (j > 0 && ks[j - 1] == k)) {
    run_slot[j] = -2;
    return;
  }
  u32 s = cell_hash(k) & mask;
  for (;;) {
    const u64 kk = tkeys[s];
    if (kk == k) {
      run_slot[j] = tslots[s];
      return;
    }
    if (kk == EMPTY_KEY) break;
    s = (s + 1) & mask;
  }
  run_slot[j] = -1;
  newflag[order[j]] = 1;
}

__device__ __forceinline__ void ivox_table_put(u64* __restrict__ tkeys, int* __restrict__ tslots, u32 mask, u64 k, int slot) {
  u32 s = cell_hash(k) & mask;
  for (;;) {
    if (atomicCAS(&tkeys[s], EMPTY_KEY, k) == EMPTY_KEY) break;  // keys put in one launch are distinct and not in the table yet
    s = (s + 1) & mask;
  }
  tslots[s] = slot;
}

// new voxels take the slots behind the existing ones, in the order of their first point's input index
__global__ __launch_bounds__(256) void ivox_claim_kernel(int n, const u64* __restrict__ ks, const u32* __restrict__ order, const int* __restrict__ rank,
                                                         int first_slot, int counter, u64* __restrict__ tkeys, int* __restrict__ tslots, u32 mask,
                                                         u64* __restrict__ skey, int* __restrict__ scount, int* __restrict__ slru, int* __restrict__ run_slot) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n || run_slot[j] != -1) return;
  const int slot = first_slot + rank[order[j]];
  const u64 k = ks[j];
  skey[slot] = k;
  scount[slot] = 0;
  slru[slot] = counter;
  ivox_table_put(tkeys, tslots, mask, k, slot);
  run_slot[j] = slot;
}

// one wavefront per sorted position; only a run head stays: FlatContainer::add over the run's candidates in input order
__global__ __launch_bounds__(256) void ivox_run_kernel(int n, const u64* __restrict__ ks, const u32* __restrict__ order, const int* __restrict__ run_slot,
                                                       const float4* __restrict__ tp, const float4* __restrict__ tA, const float2* __restrict__ tB, int cap,
                                                       double min_sq, int counter, int* __restrict__ scount, int* __restrict__ slru, float4* __restrict__ pts,
                                                       float4* __restrict__ covA, float2* __restrict__ covB, int* __restrict__ added) {
  const int j = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (j >= n) return;
  const int slot = run_slot[j];
  if (slot < 0) return;
  const int lane = threadIdx.x & 63;
  const int first = slot * cap;
  const int cnt0 = scount[slot];
  int cnt = cnt0;
  double mx = 0.0, my = 0.0, mz = 0.0;
  if (lane < cnt) {
    const float4 m = pts[first + lane];
    mx = m.x;
    my = m.y;
    mz = m.z;
  }
  const u64 k = ks[j];
  for (int jj = j; jj < n && cnt < cap; jj++) {
    if (jj > j && ks[jj] != k) break;
    const u32 i = order[jj];
    const float4 p = tp[i];
    const bool close = lane < cnt && sqdist_nc((double)p.x, (double)p.y, (double)p.z, mx, my, mz) < min_sq;
    if (__ballot(close) != 0ull) continue;
    if (lane == cnt) {
      mx = p.x;
      my = p.y;
      mz = p.z;
      pts[first + cnt] = make_float4(p.x, p.y, p.z, __int_as_float(first + cnt));
      covA[first + cnt] = tA[i];
      covB[first + cnt] = tB[i];
    }
    cnt++;
  }
  if (lane == 0) {
    scount[slot] = cnt;
    slru[slot] = counter;
    if (cnt > cnt0) atomicAdd(added, cnt - cnt0);
  }
}

__global__ __launch_bounds__(256) void ivox_table_build_kernel(int v, const u64* __restrict__ skey, u64* __restrict__ tkeys, int* __restrict__ tslots, u32 mask) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s < v) ivox_table_put(tkeys, tslots, mask, skey[s], s);
}

// the LRU sweep: keep[s] = !(lru + horizon < counter), one entry past the end stays 0 so that the scan's last value is the survivor count
__global__ __launch_bounds__(256) void ivox_lru_flag_kernel(int v, const int* __restrict__ slru, int horizon, int counter, int* __restrict__ keep) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s <= v) keep[s] = (s < v && !((long long)slru[s] + horizon < (long long)counter)) ? 1 : 0;
}

// one wavefront per old slot: a survivor moves to its rank among the survivors (order kept); its points learn their new positions
__global__ __launch_bounds__(256) void ivox_compact_kernel(int v, const int* __restrict__ keep, const int* __restrict__ rank, int cap, const u64* __restrict__ skey,
                                                           const int* __restrict__ scount, const int* __restrict__ slru, const float4* __restrict__ pts,
                                                           const float4* __restrict__ covA, const float2* __restrict__ covB, u64* __restrict__ nkey,
                                                           int* __restrict__ ncount, int* __restrict__ nlru, float4* __restrict__ npts, float4* __restrict__ nA,
                                                           float2* __restrict__ nB, int* __restrict__ kept_points) {
  const int s = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (s >= v || !keep[s]) return;
  const int lane = threadIdx.x & 63;
  const int d = rank[s], cnt = scount[s];
  if (lane == 0) {
    nkey[d] = skey[s];
    ncount[d] = cnt;
    nlru[d] = slru[s];
    atomicAdd(kept_points, cnt);
  }
  if (lane < cnt) {
    const float4 p = pts[s * cap + lane];
    npts[d * cap + lane] = make_float4(p.x, p.y, p.z, __int_as_float(d * cap + lane));
    nA[d * cap + lane] = covA[s * cap + lane];
    nB[d * cap + lane] = covB[s * cap + lane];
  }
}

struct IvoxSlots {
  u64* skey = nullptr;
  int* scount = nullptr;
  int* slru = nullptr;
  float4* pts = nullptr;
  float4* covA = nullptr;
  float2* covB = nullptr;
  void release() {
    void* all[] = {skey, scount, slru, pts, covA, covB};
    for (void* p : all)
      if (p) (void)pool_free(p);
    *this = IvoxSlots();
  }
};

int ivox_slots_alloc(IvoxSlots* s, int slots, int cap) {
  const size_t ns = (size_t)slots, np = ns * (size_t)cap;
  GA_HIP(pool_malloc(&s->skey, ns * sizeof(u64)));
  GA_HIP(pool_malloc(&s->scount, ns * sizeof(int)));
  GA_HIP(pool_malloc(&s->slru, ns * sizeof(int)));
  GA_HIP(pool_malloc(&s->pts, np * sizeof(float4)));
  GA_HIP(pool_malloc(&s->covA, np * sizeof(float4)));
  GA_HIP(pool_malloc(&s->covB, np * sizeof(float2)));
  return GLIM_AMD_OK;
}
IvoxSlots ivox_slots_of(const glim_amd_ivox* m) {
  IvoxSlots s;
  s.skey = m->skey; s.scount = m->scount; s.slru = m->slru; s.pts = m->pts; s.covA = m->covA; s.covB = m->covB;
  return s;
}
void ivox_slots_adopt(glim_amd_ivox* m, const IvoxSlots& s) {
  m->skey = s.skey; m->scount = s.scount; m->slru = s.slru; m->pts = s.pts; m->covA = s.covA; m->covB = s.covB;
}

// table of at least 2 * need entries holding the first `v` slots; the stream is idle on return when it was rebuilt
int ivox_table_ensure(glim_amd_ivox* m, int need, int v, bool rebuild, hipStream_t st) {
  unsigned int want = m->tsize;
  if ((unsigned long long)need * 2 > want) {
    want = next_pow2((unsigned long long)std::max(need, 16) * 4);
    rebuild = true;
  }
  if (!rebuild) return GLIM_AMD_OK;
  if (want != m->tsize) {
    GA_HIP(hipStreamSynchronize(st));
    if (m->tkeys) (void)pool_free(m->tkeys);
    if (m->tslots) (void)pool_free(m->tslots);
    m->tkeys = nullptr;
    m->tslots = nullptr;
    m->tsize = 0;
    GA_HIP(pool_malloc(&m->tkeys, (size_t)want * sizeof(u64)));
    GA_HIP(pool_malloc(&m->tslots, (size_t)want * sizeof(int)));
    m->tsize = want;
  }
  GA_HIP(hipMemsetAsync(m->tkeys, 0xff, (size_t)m->tsize * sizeof(u64), st));
  if (v > 0) ivox_table_build_kernel<<<grid_for(v), 256, 0, st>>>(v, m->skey, m->tkeys, m->tslots, m->tsize - 1);
  GA_HIP(hipGetLastError());
  return GLIM_AMD_OK;
}

// slot arrays for at least `need` slots: growth copies the live slots over (positions, hence correspondences, keep their meaning)
int ivox_slots_ensure(glim_amd_ivox* m, int need, hipStream_t st) {
  if (need <= m->slot_cap) return GLIM_AMD_OK;
  const long long want = std::max<long long>(std::max<long long>(need, 2ll * m->slot_cap), std::max(m->init_slots, 1));
  if (want * m->cap > 0x7fffffffll) return GLIM_AMD_ERR_NOMEM;  // positions are 32-bit
  IvoxSlots fresh;
  const int rc = ivox_slots_alloc(&fresh, (int)want, m->cap);
  if (rc != GLIM_AMD_OK) {
    fresh.release();
    return rc;
  }
  const size_t v = (size_t)m->num_slots, vp = v * (size_t)m->cap;
  hipError_t e = hipSuccess;
  if (v > 0) {
    e = hipMemcpyAsync(fresh.skey, m->skey, v * sizeof(u64), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(fresh.scount, m->scount, v * sizeof(int), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(fresh.slru, m->slru, v * sizeof(int), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(fresh.pts, m->pts, vp * sizeof(float4), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(fresh.covA, m->covA, vp * sizeof(float4), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(fresh.covB, m->covB, vp * sizeof(float2), hipMemcpyDeviceToDevice, st);
  }
  const hipError_t e2 = hipStreamSynchronize(st);  // the old arrays go back to the pool only when nothing reads them
  if (e != hipSuccess || e2 != hipSuccess) {
    fresh.release();
    set_hip_error(e != hipSuccess ? e : e2, "ivox grow");
    return GLIM_AMD_ERR_HIP;
  }
  IvoxSlots old = ivox_slots_of(m);
  old.release();
  ivox_slots_adopt(m, fresh);
  m->slot_cap = (int)want;
  return GLIM_AMD_OK;
}

// the eviction of insert()'s clear cycle; caller holds ctx->mu
int ivox_sweep(glim_amd_ivox* m, hipStream_t st) {
  const int v = m->num_slots;
  if (v == 0) return GLIM_AMD_OK;
  glim_amd_ctx* ctx = m->ctx;
  DeviceTemp keep, rank, tiles, counters;
  SyncOnExit in_flight(st);
  GA_HIP(pool_malloc(&keep.p, ((size_t)v + 1) * sizeof(int)));
  GA_HIP(pool_malloc(&rank.p, ((size_t)v + 1) * sizeof(int)));
  GA_HIP(pool_malloc(&tiles.p, scan_scratch_ints((unsigned int)v + 1) * sizeof(int)));
  GA_HIP(pool_malloc(&counters.p, sizeof(int)));
  ivox_lru_flag_kernel<<<grid_for(v + 1), 256, 0, st>>>(v, m->slru, m->lru_horizon, m->lru_counter, keep.as<int>());
  GA_HIP(exclusive_scan_int(st, keep.as<int>(), (unsigned int)v + 1, tiles.as<int>(), rank.as<int>()));
  int kept = 0;
  GA_HIP(read_back_sync(ctx, st, &kept, rank.as<int>() + v, sizeof(int)));
  if (kept == v) {
    in_flight.dismiss();
    return GLIM_AMD_OK;
  }
  IvoxSlots fresh;
  const int rc = ivox_slots_alloc(&fresh, m->slot_cap, m->cap);
  if (rc != GLIM_AMD_OK) {
    fresh.release();
    return rc;
  }
  hipError_t e = hipMemsetAsync(counters.p, 0, sizeof(int), st);
  ivox_compact_kernel<<<(v + 3) / 4, 256, 0, st>>>(v, keep.as<int>(), rank.as<int>(), m->cap, m->skey, m->scount, m->slru, m->pts, m->covA, m->covB, fresh.skey,
                                                   fresh.scount, fresh.slru, fresh.pts, fresh.covA, fresh.covB, counters.as<int>());
  if (e == hipSuccess) e = hipGetLastError();
  int kept_points = 0;
  if (e == hipSuccess) e = read_back_sync(ctx, st, &kept_points, counters.p, sizeof(int));
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    fresh.release();
    set_hip_error(e, "ivox sweep");
    return GLIM_AMD_ERR_HIP;
  }
  IvoxSlots old = ivox_slots_of(m);
  old.release();
  ivox_slots_adopt(m, fresh);
  m->num_slots = kept;
  m->num_points = kept_points;
  GA_TRY(ivox_table_ensure(m, kept, kept, true, st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  return GLIM_AMD_OK;
}

}  // namespace

extern "C" {

int glim_amd_ivox_destroy(glim_amd_ivox* m) {
  if (!m) return GLIM_AMD_OK;
  if (m->live_factors.load() > 0) return GLIM_AMD_ERR_STATE;
  if (m->ctx) {
    (void)hipSetDevice(m->ctx->device);
    std::lock_guard<std::mutex> lock(m->ctx->mu);
    IvoxSlots s = ivox_slots_of(m);
    s.release();
    if (m->tkeys) (void)pool_free(m->tkeys);
    if (m->tslots) (void)pool_free(m->tslots);
  }
  delete m;
  return GLIM_AMD_OK;
}

int glim_amd_ivox_create(glim_amd_ctx* ctx, double leaf_size, glim_amd_ivox** out) {
  if (!ctx || !out || !(leaf_size > 0.0) || !std::isfinite(leaf_size)) return GLIM_AMD_ERR_INVALID;
  glim_amd_ivox* m = new glim_amd_ivox();
  m->ctx = ctx;
  m->leaf = leaf_size;
  m->inv_leaf = 1.0 / leaf_size;
  *out = m;
  return GLIM_AMD_OK;
}

int glim_amd_ivox_set_insertion(glim_amd_ivox* m, double min_dist_in_cell, int32_t max_points_in_cell) {
  if (!m || !(min_dist_in_cell >= 0.0) || max_points_in_cell < 1 || max_points_in_cell > 64) return GLIM_AMD_ERR_INVALID;
  std::lock_guard<std::mutex> lock(m->ctx->mu);
  if (m->num_slots > 0 || m->slot_cap > 0) return GLIM_AMD_ERR_STATE;  // the slot arrays are laid out for one cell size
  m->min_dist = min_dist_in_cell;
  m->cap = max_points_in_cell;
  return GLIM_AMD_OK;
}

int glim_amd_ivox_set_lru(glim_amd_ivox* m, int32_t horizon, int32_t clear_cycle) {
  if (!m || horizon < 0 || clear_cycle < 1) return GLIM_AMD_ERR_INVALID;
  std::lock_guard<std::mutex> lock(m->ctx->mu);
  m->lru_horizon = horizon;
  m->lru_clear_cycle = clear_cycle;
  return GLIM_AMD_OK;
}

int glim_amd_ivox_set_neighbor_voxel_mode(glim_amd_ivox* m, int32_t mode) {
  if (!m || (mode != 1 && mode != 7 && mode != 19 && mode != 27)) return GLIM_AMD_ERR_INVALID;
  std::lock_guard<std::mutex> lock(m->ctx->mu);
  m->mode = mode;
  m->generation++;  // kept correspondences were found with the old mode
  return GLIM_AMD_OK;
}

int glim_amd_ivox_insert(glim_amd_ivox* m, const glim_amd_cloud* cloud, const double* T_world_cloud12) {
  if (!m || !cloud) return GLIM_AMD_ERR_INVALID;
  if (cloud->ctx->device != m->ctx->device) return GLIM_AMD_ERR_INVALID;
  if (cloud->n > (int64_t)(1 << 28)) return GLIM_AMD_ERR_INVALID;
  if (!cloud->has_covs) return GLIM_AMD_ERR_STATE;
  glim_amd_ctx* ctx = m->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  const int n = (int)cloud->n;
  m->generation++;
  if (n > 0) {
    const size_t nn = (size_t)n;
    DeviceTemp tp, tA, tB, ka, kb, va, vb, hist, run_slot, newflag, rank, tiles, counters;
    SyncOnExit in_flight(st);
    GA_HIP(pool_malloc(&tp.p, nn * sizeof(float4)));
    GA_HIP(pool_malloc(&tA.p, nn * sizeof(float4)));
    GA_HIP(pool_malloc(&tB.p, nn * sizeof(float2)));
    GA_HIP(pool_malloc(&ka.p, nn * sizeof(u64)));
    GA_HIP(pool_malloc(&kb.p, nn * sizeof(u64)));
    GA_HIP(pool_malloc(&va.p, nn * sizeof(u32)));
    GA_HIP(pool_malloc(&vb.p, nn * sizeof(u32)));
    GA_HIP(pool_malloc(&hist.p, radix_sort_scratch_bytes(n)));
    GA_HIP(pool_malloc(&run_slot.p, nn * sizeof(int)));
    GA_HIP(pool_malloc(&newflag.p, (nn + 1) * sizeof(int)));
    GA_HIP(pool_malloc(&rank.p, (nn + 1) * sizeof(int)));
    GA_HIP(pool_malloc(&tiles.p, scan_scratch_ints((unsigned int)n + 1) * sizeof(int)));
    GA_HIP(pool_malloc(&counters.p, sizeof(int)));
    GA_TRY(ivox_table_ensure(m, std::max(m->num_slots, 1), m->num_slots, false, st));
    IvoxPose P{};
    if (T_world_cloud12) memcpy(P.T, T_world_cloud12, sizeof(P.T));
    ivox_key_kernel<<<grid_for(n), 256, 0, st>>>(n, cloud->pts, cloud->covA, cloud->covB, T_world_cloud12 ? 1 : 0, P, m->inv_leaf, tp.as<float4>(),
                                                 tA.as<float4>(), tB.as<float2>(), ka.as<u64>());
    u64* ks = nullptr;
    u32* vs = nullptr;
    GA_HIP(radix_sort_pairs(st, n, 64, ka.as<u64>(), va.as<u32>(), kb.as<u64>(), vb.as<u32>(), true, hist.as<int>(), &ks, &vs));
    GA_HIP(hipMemsetAsync(newflag.p, 0, (nn + 1) * sizeof(int), st));
    GA_HIP(hipMemsetAsync(counters.p, 0, sizeof(int), st));
    ivox_head_kernel<<<grid_for(n), 256, 0, st>>>(n, ks, vs, m->tkeys, m->tslots, m->tsize - 1, run_slot.as<int>(), newflag.as<int>());
    GA_HIP(exclusive_scan_int(st, newflag.as<int>(), (unsigned int)n + 1, tiles.as<int>(), rank.as<int>()));
    int fresh = 0;
    GA_HIP(read_back_sync(ctx, st, &fresh, rank.as<int>() + n, sizeof(int)));
    if (fresh < 0 || fresh > n) return GLIM_AMD_ERR_HIP;
    const int v0 = m->num_slots, v1 = v0 + fresh;
    GA_TRY(ivox_slots_ensure(m, std::max(v1, 1), st));
    GA_TRY(ivox_table_ensure(m, v1, v0, false, st));
    if (fresh > 0)
      ivox_claim_kernel<<<grid_for(n), 256, 0, st>>>(n, ks, vs, rank.as<int>(), v0, m->lru_counter, m->tkeys, m->tslots, m->tsize - 1, m->skey, m->scount,
                                                     m->slru, run_slot.as<int>());
    ivox_run_kernel<<<(n + 3) / 4, 256, 0, st>>>(n, ks, vs, run_slot.as<int>(), tp.as<float4>(), tA.as<float4>(), tB.as<float2>(), m->cap,
                                                 m->min_dist * m->min_dist, m->lru_counter, m->scount, m->slru, m->pts, m->covA, m->covB, counters.as<int>());
    GA_HIP(hipGetLastError());
    int added = 0;
    GA_HIP(read_back_sync(ctx, st, &added, counters.p, sizeof(int)));
    in_flight.dismiss();
    m->num_slots = v1;
    m->num_points += added;
  }
  if (++m->lru_counter % m->lru_clear_cycle == 0) GA_TRY(ivox_sweep(m, st));
  return GLIM_AMD_OK;
}

int glim_amd_ivox_info(const glim_amd_ivox* m, int32_t* num_voxels, int64_t* num_points, int32_t* lru_counter, double* leaf_size) {
  if (!m) return GLIM_AMD_ERR_INVALID;
  std::lock_guard<std::mutex> lock(m->ctx->mu);
  if (num_voxels) *num_voxels = m->num_slots;
  if (num_points) *num_points = m->num_points;
  if (lru_counter) *lru_counter = m->lru_counter;
  if (leaf_size) *leaf_size = m->leaf;
  return GLIM_AMD_OK;
}

int glim_amd_ivox_download(const glim_amd_ivox* m, int32_t* coords, int32_t* counts, float* points, float* covs) {
  if (!m) return GLIM_AMD_ERR_INVALID;
  glim_amd_ctx* ctx = m->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  const size_t v = (size_t)m->num_slots, cap = (size_t)m->cap;
  if (v == 0) return GLIM_AMD_OK;
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  std::vector<u64> k(v);
  std::vector<int> c(v);
  std::vector<float4> p, a;
  std::vector<float2> b;
  GA_HIP(hipMemcpyAsync(k.data(), m->skey, v * sizeof(u64), hipMemcpyDeviceToHost, st));
  GA_HIP(hipMemcpyAsync(c.data(), m->scount, v * sizeof(int), hipMemcpyDeviceToHost, st));
  if (points) {
    p.resize(v * cap);
    GA_HIP(hipMemcpyAsync(p.data(), m->pts, v * cap * sizeof(float4), hipMemcpyDeviceToHost, st));
  }
  if (covs) {
    a.resize(v * cap);
    b.resize(v * cap);
    GA_HIP(hipMemcpyAsync(a.data(), m->covA, v * cap * sizeof(float4), hipMemcpyDeviceToHost, st));
    GA_HIP(hipMemcpyAsync(b.data(), m->covB, v * cap * sizeof(float2), hipMemcpyDeviceToHost, st));
  }
  GA_HIP(hipStreamSynchronize(st));
  for (size_t s = 0; s < v; s++) {
    if (coords)
      for (int q = 0; q < 3; q++) coords[3 * s + q] = (int32_t)((k[s] >> (21 * q)) & 0x1FFFFFull) - KEY_OFFSET;
    if (counts) counts[s] = c[s];
    for (size_t l = 0; l < cap; l++) {
      const size_t j = s * cap + l;
      const bool live = (int)l < c[s];  // places beyond the count were never written: they read as zero
      if (points) {
        points[3 * j] = live ? p[j].x : 0.f;
        points[3 * j + 1] = live ? p[j].y : 0.f;
        points[3 * j + 2] = live ? p[j].z : 0.f;
      }
      if (covs) {
        const float m9[9] = {a[j].x, a[j].y, a[j].z, a[j].y, a[j].w, b[j].x, a[j].z, b[j].x, b[j].y};
        for (int q = 0; q < 9; q++) covs[9 * j + q] = live ? m9[q] : 0.f;
      }
    }
  }
  return GLIM_AMD_OK;
}

int glim_amd_ivox_voxel_points(const glim_amd_ivox* m, double* points4) {
  if (!m || (!points4 && m->num_points > 0)) return GLIM_AMD_ERR_INVALID;
  glim_amd_ctx* ctx = m->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  const size_t v = (size_t)m->num_slots, cap = (size_t)m->cap;
  if (v == 0) return GLIM_AMD_OK;
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  std::vector<int> c(v);
  std::vector<float4> p(v * cap);
  GA_HIP(hipMemcpyAsync(c.data(), m->scount, v * sizeof(int), hipMemcpyDeviceToHost, st));
  GA_HIP(hipMemcpyAsync(p.data(), m->pts, v * cap * sizeof(float4), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  size_t o = 0;
  for (size_t s = 0; s < v; s++)
    for (int l = 0; l < c[s]; l++, o++) {
      const float4 q = p[s * cap + (size_t)l];
      points4[4 * o] = q.x;
      points4[4 * o + 1] = q.y;
      points4[4 * o + 2] = q.z;
      points4[4 * o + 3] = 1.0;
    }
  return GLIM_AMD_OK;
}

int glim_amd_debug_ivox_set_initial_capacity(glim_amd_ivox* m, int32_t slots) {
  if (!m || slots < 1) return GLIM_AMD_ERR_INVALID;
  std::lock_guard<std::mutex> lock(m->ctx->mu);
  if (m->slot_cap > 0) return GLIM_AMD_ERR_STATE;
  m->init_slots = slots;
  return GLIM_AMD_OK;
}

int glim_amd_debug_ivox_capacity(const glim_amd_ivox* m, int32_t* slot_capacity, int32_t* table_size) {
  if (!m) return GLIM_AMD_ERR_INVALID;
  std::lock_guard<std::mutex> lock(m->ctx->mu);
  if (slot_capacity) *slot_capacity = m->slot_cap;
  if (table_size) *table_size = (int32_t)m->tsize;
  return GLIM_AMD_OK;
}

}  // extern "C"
