// map_edit.hip -- device side of the reference's map editor (src/glim/viewer/editor/points_selector.cpp): point selection over many sub-maps
// with the editor's predicates, the statistical outliers in a radius, region growing, min-cut segmentation, and the removal of points from a device cloud.
// Semantics: include/glim_amd.h "Map editing"; the predicates themselves: map_edit.hpp.
//
// Passes (one lane per point, 256-thread blocks, FP64):
//   edit_flag_kernel      predicate of every point of every sub-map -> 0 / 1, then scan.hpp's exclusive prefix sum and edit_scatter_kernel:
//                         the stable compaction of plane_ba.hip
//   edit_world_kernel     world point, squared distance to the centre (and world normal) of every selected pair, in pair order
//   edit_seed_*           lexicographic minimum of (qq, candidate) in two stages
//   edit_cell_key_kernel  cell of a uniform grid per candidate -> sort.hip -> edit_cell_range_kernel (first / last position of every cell)
//   edit_round_kernel     one growth round: an unassigned candidate takes level rho iff a neighbour in its 27 cells has a level < rho and an edge to it
//   edit_mc_*             min-cut: the candidates' neighbour graph -- edge keys from the kNN -> sort.hip -> unique -> capacities, terminal
//                         capacities; the flow itself is min_cut.hip's
//   edit_keep_*           removal: keep flags, prefix sum, then cloud_gather.hpp's gather of every per-point array
#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>

#include "cloud_gather.hpp"
#include "internal.hpp"
#include "map_edit.hpp"
#include "min_cut.hpp"
#include "outlier_stat.hpp"
#include "scan.hpp"
#include "scope_sync.hpp"

namespace glim_amd {
namespace edit {

using u64 = unsigned long long;
using u32 = unsigned int;

struct SubDesc {
  const double4* p64;
  const float4* p32;
  const float4* nrm;
  int n;
  int off;  // index of the sub-map's first point in the concatenation
  double M[12];
};

constexpr int MAX_CLOUDS = 4096;
constexpr int RPL = GLIM_AMD_EDIT_ROUNDS_PER_LOOK;

__device__ __forceinline__ int find_sub(const SubDesc* __restrict__ d, int S, int i) {
  int lo = 0, hi = S - 1;  // last sub-map whose offset is <= i (empty sub-maps share an offset with their successor: take the last)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].off <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ void load_transformed(const SubDesc& d, int j, double* v) {
  double x, y, z;
  if (d.p64) {
    const double4 p = d.p64[j];
    x = p.x, y = p.y, z = p.z;
  } else {
    const float4 p = d.p32[j];
    x = (double)p.x, y = (double)p.y, z = (double)p.z;
  }
  transform(d.M, x, y, z, v);
}

static __global__ __launch_bounds__(256) void edit_flag_kernel(const SubDesc* __restrict__ descs, int S, int total, Predicate pred, int* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const SubDesc& d = descs[find_sub(descs, S, i)];
  double v[3];
  load_transformed(d, i - d.off, v);
  flags[i] = selected(pred, v) ? 1 : 0;
}

// pairs[2 pos] = (sub-map, point) of the pos-th selected point, for pos < capacity
static __global__ __launch_bounds__(256) void edit_scatter_kernel(const int* __restrict__ flags, const int* __restrict__ pos, int total,
                                                                  const SubDesc* __restrict__ descs, int S, int capacity, int* __restrict__ pairs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total || !flags[i]) return;
  const int p = pos[i];
  if (p >= capacity) return;
  const int s = find_sub(descs, S, i);
  pairs[2 * p] = s;
  pairs[2 * p + 1] = i - descs[s].off;
}

// W[i] = (world point, qq to the centre) of pair i; Nw[i] = the world normal; e4 / w4: the FP32 image of w - c and the FP64 point of a
// transient cloud.  Each output may be null.
static __global__ __launch_bounds__(256) void edit_world_kernel(const int* __restrict__ pairs, int m, const SubDesc* __restrict__ descs, Predicate pred,
                                                                double4* __restrict__ W, double4* __restrict__ Nw, float4* __restrict__ e4,
                                                                double4* __restrict__ w4) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const SubDesc& d = descs[pairs[2 * i]];
  const int j = pairs[2 * i + 1];
  double v[3];
  load_transformed(d, j, v);
  if (W) W[i] = make_double4(v[0], v[1], v[2], center_qq(pred, v));
  if (Nw) {
    const float4 n = d.nrm[j];
    double r[3];
    rotate(d.M, (double)n.x, (double)n.y, (double)n.z, r);
    Nw[i] = make_double4(r[0], r[1], r[2], 0.0);
  }
  if (e4) e4[i] = make_float4((float)(v[0] - pred.center[0]), (float)(v[1] - pred.center[1]), (float)(v[2] - pred.center[2]), 1.0f);
  if (w4) w4[i] = make_double4(v[0], v[1], v[2], 1.0);
}

// ---- seed: the smallest (qq, candidate), a total order, so that any reduction shape gives the same answer ----
__device__ __forceinline__ void lex_min(double& q, int& i, double q2, int i2) {
  if (i2 >= 0 && (i < 0 || q2 < q || (q2 == q && i2 < i))) q = q2, i = i2;
}

__device__ __forceinline__ void block_lex_min(double& q, int& i, double* s_q, int* s_i) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double q2 = __shfl_down(q, off, 64);
    const int i2 = __shfl_down(i, off, 64);
    lex_min(q, i, q2, i2);
  }
  if ((threadIdx.x & 63) == 0) s_q[threadIdx.x >> 6] = q, s_i[threadIdx.x >> 6] = i;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < 4; w++) lex_min(q, i, s_q[w], s_i[w]);
}

static __global__ __launch_bounds__(256) void edit_seed_partial_kernel(const double4* __restrict__ W, int m, double* __restrict__ bq, int* __restrict__ bi) {
  __shared__ double s_q[4];
  __shared__ int s_i[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double q = 0.0;
  int idx = -1;
  if (i < m) q = W[i].w, idx = i;
  block_lex_min(q, idx, s_q, s_i);
  if (threadIdx.x == 0) bq[blockIdx.x] = q, bi[blockIdx.x] = idx;
}

// seed[0] = the seed candidate, seed_qq[0] = its qq
static __global__ __launch_bounds__(256) void edit_seed_final_kernel(const double* __restrict__ bq, const int* __restrict__ bi, int nblocks,
                                                                     int* __restrict__ seed, double* __restrict__ seed_qq) {
  __shared__ double s_q[4];
  __shared__ int s_i[4];
  double q = 0.0;
  int idx = -1;
  for (int b = threadIdx.x; b < nblocks; b += 256) lex_min(q, idx, bq[b], bi[b]);
  block_lex_min(q, idx, s_q, s_i);
  if (threadIdx.x == 0) seed[0] = idx, seed_qq[0] = q;
}

// ---- uniform grid over the candidates ----
struct Grid {
  double origin[3];
  double inv_h;
  int dim[3];
  int pad;
};

__device__ __forceinline__ int cell_coord(double w, double origin, double inv_h, int dim) {
  const double f = floor((w - origin) * inv_h);
  return (int)fmin(fmax(f, 0.0), (double)(dim - 1));  // clamping keeps neighbours within one cell of each other
}

static __global__ __launch_bounds__(256) void edit_cell_key_kernel(const double4* __restrict__ W, int m, Grid g, u64* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const double4 w = W[i];
  const int cx = cell_coord(w.x, g.origin[0], g.inv_h, g.dim[0]), cy = cell_coord(w.y, g.origin[1], g.inv_h, g.dim[1]),
            cz = cell_coord(w.z, g.origin[2], g.inv_h, g.dim[2]);
  keys[i] = (u64)(((long long)cz * g.dim[1] + cy) * g.dim[0] + cx);
}

// keys sorted: cell c holds the positions [cstart[c], cend[c]) (both zero for an empty cell: the arrays are cleared first)
static __global__ __launch_bounds__(256) void edit_cell_range_kernel(const u64* __restrict__ keys, int m, int* __restrict__ cstart, int* __restrict__ cend) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const u64 k = keys[j];
  if (j == 0 || keys[j - 1] != k) cstart[k] = j;
  if (j == m - 1 || keys[j + 1] != k) cend[k] = j + 1;
}

// candidates in cell order; level -1 everywhere but at the seed
static __global__ __launch_bounds__(256) void edit_reorder_kernel(const u32* __restrict__ vals, int m, const double4* __restrict__ W, const double4* __restrict__ Nw,
                                                                  const int* __restrict__ seed, double4* __restrict__ Ws, double4* __restrict__ Ns,
                                                                  int* __restrict__ lv) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const int i = (int)vals[j];
  Ws[j] = W[i];
  if (Ns) Ns[j] = Nw[i];
  lv[j] = i == seed[0] ? 0 : -1;
}

// One pull round.  Levels are read and written with plain 32-bit accesses: a level written in THIS round is rho, which the test `< rho`
// rejects like the -1 it replaced, so what a lane sees of its neighbours' stores does not matter.  prev: the counter of the round before
// (null: run anyway); a round after one that assigned nothing returns at once.  cnt: points this round assigned (a counter, not a result).
static __global__ __launch_bounds__(256) void edit_round_kernel(const double4* __restrict__ Ws, const double4* __restrict__ Ns, const u64* __restrict__ keys,
                                                                const int* __restrict__ cstart, const int* __restrict__ cend, int m, Grid g, double thr2,
                                                                double cos_angle, int rho, int* lv, const int* __restrict__ prev, int* __restrict__ cnt) {
  if (prev && *prev == 0) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  bool hit = false;
  if (j < m && lv[j] < 0) {
    const double4 a4 = Ws[j];
    const double a[3] = {a4.x, a4.y, a4.z};
    double na[3] = {0.0, 0.0, 0.0};
    if (Ns) {
      const double4 n4 = Ns[j];
      na[0] = n4.x, na[1] = n4.y, na[2] = n4.z;
    }
    const long long key = (long long)keys[j];
    const int cx = (int)(key % g.dim[0]), cy = (int)((key / g.dim[0]) % g.dim[1]), cz = (int)(key / ((long long)g.dim[0] * g.dim[1]));
    for (int dz = -1; dz <= 1 && !hit; dz++) {
      const int z = cz + dz;
      if (z < 0 || z >= g.dim[2]) continue;
      for (int dy = -1; dy <= 1 && !hit; dy++) {
        const int y = cy + dy;
        if (y < 0 || y >= g.dim[1]) continue;
        const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dim[0] - 1);
        const long long row = ((long long)z * g.dim[1] + y) * g.dim[0];
        for (int x = x0; x <= x1 && !hit; x++) {
          const int k1 = cend[row + x];
          for (int k = cstart[row + x]; k < k1; k++) {
            const int l = lv[k];
            if (l < 0 || l >= rho) continue;
            const double4 b4 = Ws[k];
            const double b[3] = {b4.x, b4.y, b4.z};
            bool e;
            if (Ns) {
              const double4 n4 = Ns[k];
              const double nb[3] = {n4.x, n4.y, n4.z};
              e = edge(a, b, thr2, na, nb, cos_angle);
            } else {
              e = edge(a, b, thr2, nullptr, nullptr, 0.0);
            }
            if (e) {
              hit = true;
              break;
            }
          }
        }
      }
    }
    if (hit) lv[j] = rho;
  }
  const u64 mask = __ballot(hit);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd(cnt, __popcll(mask));
}

// back to candidate order: level[i], and flags[i] = 1 iff candidate i belongs to the cluster
static __global__ __launch_bounds__(256) void edit_unsort_kernel(const u32* __restrict__ vals, const int* __restrict__ lv, int m, int* __restrict__ level,
                                                                 int* __restrict__ flags) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const int l = lv[j];
  level[vals[j]] = l;
  flags[vals[j]] = l >= 0 ? 1 : 0;
}

// out[pos] = the pos-th flagged candidate's pair (and level), for pos < capacity
static __global__ __launch_bounds__(256) void edit_pick_kernel(const int* __restrict__ flags, const int* __restrict__ pos, int m, const int* __restrict__ cand,
                                                               const int* __restrict__ level, int capacity, int* __restrict__ pairs, int* __restrict__ levels) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m || !flags[i]) return;
  const int p = pos[i];
  if (p >= capacity) return;
  pairs[2 * p] = cand[2 * i];
  pairs[2 * p + 1] = cand[2 * i + 1];
  if (levels) levels[p] = level[i];
}

// outliers: flags[i] = candidate i lies inside the inner radius and is no inlier; flags[m] = 0
static __global__ __launch_bounds__(256) void edit_outlier_flag_kernel(const double4* __restrict__ W, const int* __restrict__ inlier, int m, double r2,
                                                                       int* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > m) return;
  flags[i] = (i < m && W[i].w < r2 && !inlier[i]) ? 1 : 0;
}

// ---- min-cut: the candidates' neighbour graph ----
// keys[i K + t] = (min << 32 | max) of candidate i and its t-th neighbour; an entry equal to i itself gets the key (m << 32), past every edge
static __global__ __launch_bounds__(256) void edit_mc_key_kernel(const int* __restrict__ nb, int m, int K, u64* __restrict__ keys) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= m * K) return;
  const int i = p / K, j = nb[p];
  u64 key = (u64)(u32)m << 32;
  if (j != i && j >= 0 && j < m) key = ((u64)(u32)min(i, j) << 32) | (u64)(u32)max(i, j);
  keys[p] = key;
}
// keys sorted: flags[p] = the key is an edge and differs from its predecessor; flags[total] = 0
static __global__ __launch_bounds__(256) void edit_mc_unique_kernel(const u64* __restrict__ keys, int total, int m, int* __restrict__ flags) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p > total) return;
  flags[p] = (p < total && (keys[p] >> 32) < (u64)m && (p == 0 || keys[p - 1] != keys[p])) ? 1 : 0;
}
// the flagged keys in their order (ascending), with their capacities
static __global__ __launch_bounds__(256) void edit_mc_edge_kernel(const u64* __restrict__ keys, const int* __restrict__ flags, const int* __restrict__ pos,
                                                                  int total, const double4* __restrict__ P, const double4* __restrict__ Nw, double sigma_d,
                                                                  double sigma_a, int2* __restrict__ edges, int* __restrict__ cap) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= total || !flags[p]) return;
  const int i = (int)(keys[p] >> 32), j = (int)(keys[p] & 0xffffffffull);
  const double4 a4 = P[i], b4 = P[j];
  const double a[3] = {a4.x, a4.y, a4.z}, b[3] = {b4.x, b4.y, b4.z};
  int c;
  if (Nw) {
    const double4 n4 = Nw[i], o4 = Nw[j];
    const double na[3] = {n4.x, n4.y, n4.z}, nb[3] = {o4.x, o4.y, o4.z};
    c = min_cut_edge_capacity(a, b, sigma_d, na, nb, sigma_a);
  } else {
    c = min_cut_edge_capacity(a, b, sigma_d, nullptr, nullptr, 0.0);
  }
  edges[pos[p]] = make_int2(i, j);
  cap[pos[p]] = c;
}
// terminal capacities from the predicate's qq; counts[0] / counts[1] += foreground / background points (counters of integers: any order)
static __global__ __launch_bounds__(256) void edit_mc_terminal_kernel(const double4* __restrict__ W, int m, double fg2, double bg2, int fg_cap, int bg_cap,
                                                                      int* __restrict__ src, int* __restrict__ snk, int* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool fg = false, bg = false;
  if (i < m) {
    const double qq = W[i].w;
    fg = qq < fg2, bg = qq >= bg2;
    src[i] = fg ? fg_cap : 0;
    snk[i] = bg ? bg_cap : 0;
  }
  const u64 mf = __ballot(fg), mb = __ballot(bg);
  if ((threadIdx.x & 63) == 0) {
    if (mf) atomicAdd(counts, __popcll(mf));
    if (mb) atomicAdd(counts + 1, __popcll(mb));
  }
}

// ---- removal ----
static __global__ __launch_bounds__(256) void edit_keep_fill_kernel(int n, int* __restrict__ keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i <= n) keep[i] = i < n ? 1 : 0;
}
// duplicates store the same 0 twice
static __global__ __launch_bounds__(256) void edit_keep_mark_kernel(const int* __restrict__ idx, int cnt, int* keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < cnt) keep[idx[i]] = 0;
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static bool finite_n(const double* a, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(a[i])) return false;
  return true;
}
static inline int grid_for(int n) { return (n + 255) / 256; }

static int check_clouds(const glim_amd_cloud* const* clouds, int32_t S, const double* M12, int* total) {
  if (S < 0 || S > MAX_CLOUDS || (S > 0 && (!clouds || !M12))) return GLIM_AMD_ERR_INVALID;
  int64_t sum = 0;
  for (int s = 0; s < S; s++) {
    if (!clouds[s]) return GLIM_AMD_ERR_INVALID;
    if ((glim_amd_ctx*)clouds[s]->ctx != (glim_amd_ctx*)clouds[0]->ctx) return GLIM_AMD_ERR_INVALID;
    sum += clouds[s]->n;
  }
  if (sum > (int64_t)0x7fffffff - 257) return GLIM_AMD_ERR_INVALID;
  if (!finite_n(M12, 12 * (size_t)S)) return GLIM_AMD_ERR_INVALID;
  *total = (int)sum;
  return GLIM_AMD_OK;
}

static int make_predicate(int mode, const glim_amd_edit_window* w, double radius, Predicate* p) {
  *p = Predicate();
  p->mode = mode;
  if (mode == MODE_BOX || mode == MODE_SPHERE) return GLIM_AMD_OK;
  if (mode != MODE_WINDOW && mode != MODE_WINDOW_BALL) return GLIM_AMD_ERR_INVALID;
  if (!w || !finite_n(w->center, 3) || !std::isfinite(w->resolution) || !(w->resolution > 0.0) || w->window < 0) return GLIM_AMD_ERR_INVALID;
  window_bounds(w->center, w->resolution, w->window, p);
  if (mode == MODE_WINDOW_BALL) {
    if (!std::isfinite(radius) || !(radius > 0.0)) return GLIM_AMD_ERR_INVALID;
    p->r2 = radius * radius;
  }
  return GLIM_AMD_OK;
}

// the sub-map descriptors and the selection's flags / ranks / pairs on the device (caller holds ctx->mu, device set)
struct Selection {
  DeviceTemp descs, flags, pos, tiles, pairs;
  int S = 0, total = 0;
};

static int select_enqueue(hipStream_t st, const glim_amd_cloud* const* clouds, int32_t S, const double* M12, int total, const Predicate& pred, int capacity,
                          Selection* sel) {
  std::vector<SubDesc> h((size_t)S);
  int off = 0;
  for (int s = 0; s < S; s++) {
    SubDesc& d = h[(size_t)s];
    d.p64 = clouds[s]->pts64;
    d.p32 = clouds[s]->pts;
    d.nrm = clouds[s]->normals;
    d.n = (int)clouds[s]->n;
    d.off = off;
    off += d.n;
    for (int i = 0; i < 12; i++) d.M[i] = M12[12 * (size_t)s + i];
  }
  sel->S = S;
  sel->total = total;
  const unsigned int T = (unsigned int)total + 1u;
  GA_HIP(pool_malloc(&sel->descs.p, (size_t)S * sizeof(SubDesc)));
  GA_HIP(pool_malloc(&sel->flags.p, (size_t)T * sizeof(int)));
  GA_HIP(pool_malloc(&sel->pos.p, (size_t)T * sizeof(int)));
  GA_HIP(pool_malloc(&sel->tiles.p, scan_scratch_ints(T) * sizeof(int)));
  GA_HIP(pool_malloc(&sel->pairs.p, (size_t)std::max(capacity, 1) * 2 * sizeof(int)));
  GA_HIP(hipMemcpyAsync(sel->descs.p, h.data(), (size_t)S * sizeof(SubDesc), hipMemcpyHostToDevice, st));
  GA_HIP(hipStreamSynchronize(st));  // h leaves scope with this call
  GA_HIP(hipMemsetAsync(sel->flags.as<int>() + total, 0, sizeof(int), st));
  if (total > 0) edit_flag_kernel<<<grid_for(total), 256, 0, st>>>(sel->descs.as<SubDesc>(), S, total, pred, sel->flags.as<int>());
  GA_HIP(exclusive_scan_int(st, sel->flags.as<int>(), T, sel->tiles.as<int>(), sel->pos.as<int>()));
  if (total > 0 && capacity > 0)
    edit_scatter_kernel<<<grid_for(total), 256, 0, st>>>(sel->flags.as<int>(), sel->pos.as<int>(), total, sel->descs.as<SubDesc>(), S, capacity, sel->pairs.as<int>());
  GA_HIP(hipGetLastError());
  return GLIM_AMD_OK;
}

// flags (m + 1 entries, the last 0) -> the flagged candidates' pairs / levels on the host, and their count
static int pick_to_host(glim_amd_ctx* ctx, hipStream_t st, const int* flags, int m, const int* cand, const int* level, int64_t capacity, int32_t* pairs,
                        int32_t* levels, int64_t* count) {
  DeviceTemp pos, tiles, d_pairs, d_levels;
  const int cap = (int)std::min<int64_t>(capacity, m);
  GA_HIP(pool_malloc(&pos.p, (size_t)(m + 1) * sizeof(int)));
  GA_HIP(pool_malloc(&tiles.p, scan_scratch_ints((unsigned int)m + 1u) * sizeof(int)));
  GA_HIP(pool_malloc(&d_pairs.p, (size_t)std::max(cap, 1) * 2 * sizeof(int)));
  if (levels) GA_HIP(pool_malloc(&d_levels.p, (size_t)std::max(cap, 1) * sizeof(int)));
  SyncOnExit in_flight(st);
  GA_HIP(exclusive_scan_int(st, flags, (unsigned int)m + 1u, tiles.as<int>(), pos.as<int>()));
  if (cap > 0) edit_pick_kernel<<<grid_for(m), 256, 0, st>>>(flags, pos.as<int>(), m, cand, level, cap, d_pairs.as<int>(), d_levels.as<int>());
  GA_HIP(hipGetLastError());
  int n = 0;
  GA_HIP(read_back_sync(ctx, st, &n, pos.as<int>() + m, sizeof(int)));
  const int wr = std::min(n, cap);
  if (wr > 0) {
    GA_HIP(hipMemcpyAsync(pairs, d_pairs.p, (size_t)wr * 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    if (levels) GA_HIP(hipMemcpyAsync(levels, d_levels.p, (size_t)wr * sizeof(int), hipMemcpyDeviceToHost, st));
    GA_HIP(hipStreamSynchronize(st));
  }
  in_flight.dismiss();
  *count = n;
  return GLIM_AMD_OK;
}

static bool no_device() { return glim_amd_device_count() <= 0; }

// the grid of the growth rounds: cells of edge >= `reach` (a hair more, so that rounding cannot put two points closer than `reach` two cells
// apart) over the window's box, doubled until the table is no larger than a few cells per candidate
static Grid make_grid(const Predicate& pred, double resolution, double reach, int m, int64_t* cells) {
  Grid g;
  double h = reach * (1.0 + 1.0 / 1048576.0);
  const int64_t budget = std::max<int64_t>(32768, std::min<int64_t>(4 * (int64_t)m, (int64_t)1 << 24));
  for (;;) {
    int64_t c = 1;
    bool fits = true;
    for (int k = 0; k < 3; k++) {
      const double extent = (pred.hi[k] - pred.lo[k] + 1.0) * resolution;
      const double d = std::floor(extent / h) + 2.0;
      if (!(d < 1048576.0)) {
        fits = false;
        break;
      }
      g.dim[k] = (int)d;
      g.origin[k] = pred.lo[k] * resolution;
      c *= g.dim[k];
    }
    if (fits && c <= budget) {
      *cells = c;
      break;
    }
    h *= 2.0;
  }
  g.inv_h = 1.0 / h;
  g.pad = 0;
  return g;
}

// ---- min-cut ----
struct MinCutSetup {
  glim_amd_edit_min_cut_params prm;
  Predicate pred;
  int total = 0;
  int fg_cap = 0, bg_cap = 0;
};

// the checks of glim_amd_edit_min_cut, in the order of glim_amd_edit_region_grow
static int min_cut_setup(const glim_amd_cloud* const* clouds, int32_t S, const double* M12, const glim_amd_edit_window* window,
                         const glim_amd_edit_min_cut_params* params, MinCutSetup* s) {
  glim_amd_edit_min_cut_params prm = {0.25, 0.17453292519943295, 0.5, 5.0, 10.0, 0.0, 20, 0, 0, 0};
  if (params) prm = *params;
  const double reals[6] = {prm.distance_sigma, prm.angle_sigma, prm.foreground_mask_radius, prm.background_mask_radius, prm.foreground_weight, prm.background_weight};
  if (!finite_n(reals, 6) || !(prm.distance_sigma > 0.0) || !(prm.angle_sigma > 0.0) || !(prm.foreground_mask_radius > 0.0) ||
      !(prm.foreground_mask_radius < prm.background_mask_radius) || !(prm.foreground_weight > 0.0) || prm.background_weight < 0.0 || prm.k_neighbors < 1 ||
      prm.max_rounds < 0)
    return GLIM_AMD_ERR_INVALID;
  if (prm.background_weight == 0.0) prm.background_weight = prm.foreground_weight;
  if (!capacity_fits(prm.foreground_weight) || !capacity_fits(prm.background_weight)) return GLIM_AMD_ERR_INVALID;
  if (prm.k_neighbors > 31) return GLIM_AMD_ERR_UNSUPPORTED;
  GA_TRY(make_predicate(MODE_WINDOW_BALL, window, prm.background_mask_radius + 1.0, &s->pred));
  GA_TRY(check_clouds(clouds, S, M12, &s->total));
  if (prm.use_normals)
    for (int c = 0; c < S; c++)
      if (clouds[c]->n > 0 && (!clouds[c]->has_normals || !clouds[c]->normals)) return GLIM_AMD_ERR_STATE;
  s->prm = prm;
  s->fg_cap = quantize_capacity(prm.foreground_weight);
  s->bg_cap = quantize_capacity(prm.background_weight);
  return GLIM_AMD_OK;
}

// the candidates and their graph on the device; the transient cloud is destroyed with the structure, outside every lock scope
struct MinCutGraph {
  CloudGuard tc;
  Selection sel;
  DeviceTemp W, Nw, edges, cap, src, snk;
  int m = 0, E = 0, num_fg = 0, num_bg = 0;
  int status = GLIM_AMD_EDIT_EMPTY;
};

// Takes the context's mutex itself, twice around the neighbour search (which takes it too).  Leaves status EMPTY / FEW_POINTS / NO_SEED with
// the counts known so far, or OK with every array built.
static int min_cut_graph(const glim_amd_cloud* const* clouds, int32_t S, const double* M12, const MinCutSetup& s, MinCutGraph* g) {
  glim_amd_ctx* ctx = clouds[0]->ctx;
  const int K = s.prm.k_neighbors + 1;
  const bool normals = s.prm.use_normals != 0;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    GA_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream();
    SyncOnExit in_flight(st);
    GA_TRY(select_enqueue(st, clouds, S, M12, s.total, s.pred, s.total, &g->sel));
    int m = 0;
    GA_HIP(read_back_sync(ctx, st, &m, g->sel.pos.as<int>() + s.total, sizeof(int)));
    if (m < 0 || m > s.total) return GLIM_AMD_ERR_HIP;
    g->m = m;
    if (m < K) {
      in_flight.dismiss();
      g->status = m == 0 ? GLIM_AMD_EDIT_EMPTY : GLIM_AMD_EDIT_FEW_POINTS;
      return GLIM_AMD_OK;
    }
    if ((int64_t)m * K > (int64_t)0x7fffffff - 257) return GLIM_AMD_ERR_INVALID;
    g->tc.c = new glim_amd_cloud();
    g->tc.c->ctx = ctx;
    g->tc.c->n = m;
    GA_HIP(pool_malloc(&g->tc.c->pts, (size_t)m * sizeof(float4)));
    GA_HIP(pool_malloc(&g->tc.c->pts64, (size_t)m * sizeof(double4)));
    GA_HIP(pool_malloc(&g->W.p, (size_t)m * sizeof(double4)));
    if (normals) GA_HIP(pool_malloc(&g->Nw.p, (size_t)m * sizeof(double4)));
    edit_world_kernel<<<grid_for(m), 256, 0, st>>>(g->sel.pairs.as<int>(), m, g->sel.descs.as<SubDesc>(), s.pred, g->W.as<double4>(), g->Nw.as<double4>(),
                                                   g->tc.c->pts, g->tc.c->pts64);
    GA_HIP(hipGetLastError());
    GA_HIP(hipStreamSynchronize(st));
    in_flight.dismiss();
  }
  GA_TRY(glim_amd_cloud_find_neighbors(g->tc.c, K, nullptr));  // takes the context's mutex itself
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  const int m = g->m, total = m * K;
  // sized by the candidate count: the keys, and the terminal arrays
  DeviceTemp ka, kb, va, vb, sort_scratch, flags, pos, tiles, counts;
  GA_HIP(pool_malloc(&ka.p, (size_t)total * sizeof(u64)));
  GA_HIP(pool_malloc(&kb.p, (size_t)total * sizeof(u64)));
  GA_HIP(pool_malloc(&va.p, (size_t)total * sizeof(u32)));
  GA_HIP(pool_malloc(&vb.p, (size_t)total * sizeof(u32)));
  GA_HIP(pool_malloc(&sort_scratch.p, radix_sort_scratch_bytes(total)));
  GA_HIP(pool_malloc(&flags.p, ((size_t)total + 1) * sizeof(int)));
  GA_HIP(pool_malloc(&pos.p, ((size_t)total + 1) * sizeof(int)));
  GA_HIP(pool_malloc(&tiles.p, scan_scratch_ints((unsigned int)total + 1u) * sizeof(int)));
  GA_HIP(pool_malloc(&counts.p, 2 * sizeof(int)));
  GA_HIP(pool_malloc(&g->src.p, (size_t)m * sizeof(int)));
  GA_HIP(pool_malloc(&g->snk.p, (size_t)m * sizeof(int)));
  SyncOnExit in_flight(st);
  GA_HIP(hipMemsetAsync(counts.p, 0, 2 * sizeof(int), st));
  edit_mc_terminal_kernel<<<grid_for(m), 256, 0, st>>>(g->W.as<double4>(), m, s.prm.foreground_mask_radius * s.prm.foreground_mask_radius,
                                                       s.prm.background_mask_radius * s.prm.background_mask_radius, s.fg_cap, s.bg_cap, g->src.as<int>(),
                                                       g->snk.as<int>(), counts.as<int>());
  edit_mc_key_kernel<<<grid_for(total), 256, 0, st>>>(g->tc.c->neighbors, m, K, ka.as<u64>());
  GA_HIP(hipGetLastError());
  int bits = 33;
  while (((int64_t)1 << (bits - 32)) <= (int64_t)m) bits++;
  u64* keys = nullptr;
  u32* vals = nullptr;
  GA_HIP(radix_sort_pairs(st, total, bits, ka.as<u64>(), va.as<u32>(), kb.as<u64>(), vb.as<u32>(), true, sort_scratch.as<int>(), &keys, &vals));
  edit_mc_unique_kernel<<<grid_for(total + 1), 256, 0, st>>>(keys, total, m, flags.as<int>());
  GA_HIP(hipGetLastError());
  GA_HIP(exclusive_scan_int(st, flags.as<int>(), (unsigned int)total + 1u, tiles.as<int>(), pos.as<int>()));
  int E = 0, h_counts[2] = {0, 0};
  GA_HIP(read_back_sync(ctx, st, &E, pos.as<int>() + total, sizeof(int)));
  GA_HIP(read_back_sync(ctx, st, h_counts, counts.p, sizeof(h_counts)));
  if (E < 0 || E > total) return GLIM_AMD_ERR_HIP;
  g->E = E, g->num_fg = h_counts[0], g->num_bg = h_counts[1];
  // sized by the edge count
  GA_HIP(pool_malloc(&g->edges.p, (size_t)std::max(E, 1) * sizeof(int2)));
  GA_HIP(pool_malloc(&g->cap.p, (size_t)std::max(E, 1) * sizeof(int)));
  edit_mc_edge_kernel<<<grid_for(total), 256, 0, st>>>(keys, flags.as<int>(), pos.as<int>(), total, g->tc.c->pts64, g->Nw.as<double4>(), s.prm.distance_sigma,
                                                       s.prm.angle_sigma, g->edges.as<int2>(), g->cap.as<int>());
  GA_HIP(hipGetLastError());
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  g->status = g->num_fg == 0 ? GLIM_AMD_EDIT_NO_SEED : GLIM_AMD_EDIT_OK;
  return GLIM_AMD_OK;
}

static void min_cut_counts(const MinCutGraph& g, glim_amd_edit_min_cut_result* out) {
  out->num_candidates = g.m;
  out->num_edges = g.E;
  out->num_foreground = g.num_fg;
  out->num_background = g.num_bg;
  out->status = g.status;
}

}  // namespace edit
}  // namespace glim_amd

extern "C" {

int glim_amd_edit_select(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* matrices12, int32_t mode,
                         const glim_amd_edit_window* window, double radius, int64_t capacity, int32_t* pairs, int64_t* count) {
  using namespace glim_amd;
  using namespace glim_amd::edit;
  if (no_device()) return GLIM_AMD_ERR_NO_DEVICE;
  if (capacity < 0 || !count || (capacity > 0 && !pairs)) return GLIM_AMD_ERR_INVALID;
  Predicate pred;
  GA_TRY(make_predicate(mode, window, radius, &pred));
  int total = 0;
  GA_TRY(check_clouds(clouds, num_clouds, matrices12, &total));
  *count = 0;
  if (num_clouds == 0) return GLIM_AMD_OK;
  glim_amd_ctx* ctx = clouds[0]->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  Selection sel;
  SyncOnExit in_flight(st);
  const int cap = (int)std::min<int64_t>(capacity, total);
  GA_TRY(select_enqueue(st, clouds, num_clouds, matrices12, total, pred, cap, &sel));
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

int glim_amd_edit_select_outliers(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12,
                                  const glim_amd_edit_window* window, double radius, const glim_amd_edit_outlier_params* params, int64_t capacity,
                                  int32_t* pairs, int64_t* count, int32_t* status) {
  using namespace glim_amd;
  using namespace glim_amd::edit;
  if (no_device()) return GLIM_AMD_ERR_NO_DEVICE;
  if (capacity < 0 || !count || (capacity > 0 && !pairs)) return GLIM_AMD_ERR_INVALID;
  glim_amd_edit_outlier_params prm = {1.0, 2.0, 10, 0};
  if (params) prm = *params;
  if (!std::isfinite(prm.radius_offset) || prm.radius_offset < 0.0 || !std::isfinite(prm.stddev_thresh) || prm.num_neighbors < 1) return GLIM_AMD_ERR_INVALID;
  if (prm.num_neighbors > 32) return GLIM_AMD_ERR_UNSUPPORTED;
  if (!std::isfinite(radius) || !(radius > 0.0)) return GLIM_AMD_ERR_INVALID;
  Predicate pred;
  GA_TRY(make_predicate(MODE_WINDOW_BALL, window, radius + prm.radius_offset, &pred));
  int total = 0;
  GA_TRY(check_clouds(clouds, num_clouds, T_world_submap12, &total));
  *count = 0;
  if (status) *status = GLIM_AMD_EDIT_FEW_POINTS;
  if (num_clouds == 0) return GLIM_AMD_OK;
  const int k = prm.num_neighbors;
  glim_amd_ctx* ctx = clouds[0]->ctx;
  CloudGuard tc;  // the candidates' world points: destroyed after the lock scopes below
  Selection sel;
  DeviceTemp W;
  int m = 0;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    GA_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream();
    SyncOnExit in_flight(st);
    GA_TRY(select_enqueue(st, clouds, num_clouds, T_world_submap12, total, pred, total, &sel));
    GA_HIP(read_back_sync(ctx, st, &m, sel.pos.as<int>() + total, sizeof(int)));
    if (m < k || m > total) {  // :730-733
      in_flight.dismiss();
      return m > total ? GLIM_AMD_ERR_HIP : GLIM_AMD_OK;
    }
    tc.c = new glim_amd_cloud();
    tc.c->ctx = ctx;
    tc.c->n = m;
    GA_HIP(pool_malloc(&tc.c->pts, (size_t)m * sizeof(float4)));
    GA_HIP(pool_malloc(&tc.c->pts64, (size_t)m * sizeof(double4)));
    GA_HIP(pool_malloc(&W.p, (size_t)m * sizeof(double4)));
    edit_world_kernel<<<grid_for(m), 256, 0, st>>>(sel.pairs.as<int>(), m, sel.descs.as<SubDesc>(), pred, W.as<double4>(), nullptr, tc.c->pts, tc.c->pts64);
    GA_HIP(hipGetLastError());
    GA_HIP(hipStreamSynchronize(st));
    in_flight.dismiss();
  }
  GA_TRY(glim_amd_cloud_find_neighbors(tc.c, k, nullptr));  // takes the context's mutex itself
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    GA_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream();
    OutlierScratch stat;
    DeviceTemp inlier, flags;
    GA_HIP(pool_malloc(&inlier.p, (size_t)(m + 1) * sizeof(int)));
    GA_HIP(pool_malloc(&flags.p, (size_t)(m + 1) * sizeof(int)));
    SyncOnExit in_flight(st);
    GA_HIP(outlier_inlier_flags(st, m, tc.c->pts64, tc.c->neighbors, k, prm.stddev_thresh, &stat, inlier.as<int>()));
    edit_outlier_flag_kernel<<<grid_for(m + 1), 256, 0, st>>>(W.as<double4>(), inlier.as<int>(), m, radius * radius, flags.as<int>());
    GA_HIP(hipGetLastError());
    GA_TRY(pick_to_host(ctx, st, flags.as<int>(), m, sel.pairs.as<int>(), nullptr, capacity, pairs, nullptr, count));
    in_flight.dismiss();
  }
  if (status) *status = GLIM_AMD_EDIT_OK;
  return GLIM_AMD_OK;
}

int glim_amd_edit_region_grow(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12,
                              const glim_amd_edit_window* window, const glim_amd_edit_region_growing_params* params, int64_t capacity,
                              int32_t* pairs, int32_t* levels, glim_amd_edit_region_result* out) {
  using namespace glim_amd;
  using namespace glim_amd::edit;
  if (no_device()) return GLIM_AMD_ERR_NO_DEVICE;
  if (capacity < 0 || !out || (capacity > 0 && !pairs)) return GLIM_AMD_ERR_INVALID;
  glim_amd_edit_region_growing_params prm = {0.5, 0.984807753012208, 0.5, 0, 0};
  if (params) prm = *params;
  if (!std::isfinite(prm.distance_threshold) || !(prm.distance_threshold > 0.0) || !std::isfinite(prm.dilation_radius) || prm.dilation_radius < 0.0 ||
      std::isnan(prm.cos_angle_threshold) || prm.max_hops < 0)
    return GLIM_AMD_ERR_INVALID;
  Predicate pred;
  GA_TRY(make_predicate(MODE_WINDOW, window, 0.0, &pred));
  int total = 0;
  GA_TRY(check_clouds(clouds, num_clouds, T_world_submap12, &total));
  const bool normals = prm.use_normals != 0;
  if (normals)
    for (int s = 0; s < num_clouds; s++)
      if (clouds[s]->n > 0 && (!clouds[s]->has_normals || !clouds[s]->normals)) return GLIM_AMD_ERR_STATE;
  *out = glim_amd_edit_region_result();
  out->seed[0] = out->seed[1] = -1;
  out->status = GLIM_AMD_EDIT_EMPTY;
  if (num_clouds == 0) return GLIM_AMD_OK;
  glim_amd_ctx* ctx = clouds[0]->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  Selection sel;
  DeviceTemp W, Nw, Ws, Ns, bq, bi, seed, seed_qq, ka, kb, va, vb, sort_scratch, cstart, cend, lv, cnt, level, flags;
  SyncOnExit in_flight(st);
  GA_TRY(select_enqueue(st, clouds, num_clouds, T_world_submap12, total, pred, total, &sel));
  int m = 0;
  GA_HIP(read_back_sync(ctx, st, &m, sel.pos.as<int>() + total, sizeof(int)));
  if (m > total) return GLIM_AMD_ERR_HIP;
  out->num_candidates = m;
  if (m == 0) {
    in_flight.dismiss();
    return GLIM_AMD_OK;
  }
  // every buffer below is sized by the candidate count
  const size_t mm = (size_t)m;
  const int mb = grid_for(m);
  GA_HIP(pool_malloc(&W.p, mm * sizeof(double4)));
  GA_HIP(pool_malloc(&Ws.p, mm * sizeof(double4)));
  if (normals) {
    GA_HIP(pool_malloc(&Nw.p, mm * sizeof(double4)));
    GA_HIP(pool_malloc(&Ns.p, mm * sizeof(double4)));
  }
  GA_HIP(pool_malloc(&bq.p, (size_t)mb * sizeof(double)));
  GA_HIP(pool_malloc(&bi.p, (size_t)mb * sizeof(int)));
  GA_HIP(pool_malloc(&seed.p, sizeof(int)));
  GA_HIP(pool_malloc(&seed_qq.p, sizeof(double)));
  edit_world_kernel<<<mb, 256, 0, st>>>(sel.pairs.as<int>(), m, sel.descs.as<SubDesc>(), pred, W.as<double4>(), Nw.as<double4>(), nullptr, nullptr);
  edit_seed_partial_kernel<<<mb, 256, 0, st>>>(W.as<double4>(), m, bq.as<double>(), bi.as<int>());
  edit_seed_final_kernel<<<1, 256, 0, st>>>(bq.as<double>(), bi.as<int>(), mb, seed.as<int>(), seed_qq.as<double>());
  GA_HIP(hipGetLastError());
  // the grid, and the candidates in cell order
  int64_t cells = 0;
  const Grid g = make_grid(pred, window->resolution, std::max(prm.distance_threshold, prm.dilation_radius), m, &cells);
  int bits = 1;
  while (((int64_t)1 << bits) < cells) bits++;
  GA_HIP(pool_malloc(&ka.p, mm * sizeof(u64)));
  GA_HIP(pool_malloc(&kb.p, mm * sizeof(u64)));
  GA_HIP(pool_malloc(&va.p, mm * sizeof(u32)));
  GA_HIP(pool_malloc(&vb.p, mm * sizeof(u32)));
  GA_HIP(pool_malloc(&sort_scratch.p, radix_sort_scratch_bytes(m)));
  GA_HIP(pool_malloc(&cstart.p, (size_t)cells * sizeof(int)));
  GA_HIP(pool_malloc(&cend.p, (size_t)cells * sizeof(int)));
  GA_HIP(pool_malloc(&lv.p, mm * sizeof(int)));
  GA_HIP(pool_malloc(&cnt.p, (size_t)(RPL + 1) * sizeof(int)));
  GA_HIP(pool_malloc(&level.p, mm * sizeof(int)));
  GA_HIP(pool_malloc(&flags.p, (mm + 1) * sizeof(int)));
  edit_cell_key_kernel<<<mb, 256, 0, st>>>(W.as<double4>(), m, g, ka.as<u64>());
  GA_HIP(hipGetLastError());
  u64* keys = nullptr;
  u32* vals = nullptr;
  GA_HIP(radix_sort_pairs(st, m, bits, ka.as<u64>(), va.as<u32>(), kb.as<u64>(), vb.as<u32>(), true, sort_scratch.as<int>(), &keys, &vals));
  GA_HIP(hipMemsetAsync(cstart.p, 0, (size_t)cells * sizeof(int), st));
  GA_HIP(hipMemsetAsync(cend.p, 0, (size_t)cells * sizeof(int), st));
  edit_cell_range_kernel<<<mb, 256, 0, st>>>(keys, m, cstart.as<int>(), cend.as<int>());
  edit_reorder_kernel<<<mb, 256, 0, st>>>(vals, m, W.as<double4>(), Nw.as<double4>(), seed.as<int>(), Ws.as<double4>(), Ns.as<double4>(), lv.as<int>());
  GA_HIP(hipGetLastError());
  // growth: chunks of RPL rounds, one look at the chunk's counters between them
  const double thr2 = prm.distance_threshold * prm.distance_threshold;
  const int limit = prm.max_hops > 0 ? prm.max_hops : INT_MAX;
  int enqueued = 0, last = 0;
  bool done = false;
  while (!done && enqueued < limit) {
    const int chunk = std::min(RPL, limit - enqueued);
    GA_HIP(hipMemsetAsync(cnt.p, 1, sizeof(int), st));  // "the round before the chunk assigned something"
    GA_HIP(hipMemsetAsync(cnt.as<int>() + 1, 0, (size_t)RPL * sizeof(int), st));
    for (int i = 1; i <= chunk; i++)
      edit_round_kernel<<<mb, 256, 0, st>>>(Ws.as<double4>(), Ns.as<double4>(), keys, cstart.as<int>(), cend.as<int>(), m, g, thr2, prm.cos_angle_threshold,
                                            enqueued + i, lv.as<int>(), cnt.as<int>() + i - 1, cnt.as<int>() + i);
    GA_HIP(hipGetLastError());
    int h_cnt[RPL + 1];
    GA_HIP(read_back_sync(ctx, st, h_cnt, cnt.p, sizeof(h_cnt)));
    for (int i = 1; i <= chunk && !done; i++) {
      if (h_cnt[i] > 0) last = enqueued + i;
      else done = true;
    }
    enqueued += chunk;
  }
  if (prm.dilation_radius > 0.0) {
    edit_round_kernel<<<mb, 256, 0, st>>>(Ws.as<double4>(), nullptr, keys, cstart.as<int>(), cend.as<int>(), m, g, prm.dilation_radius * prm.dilation_radius, 0.0,
                                          last + 1, lv.as<int>(), nullptr, cnt.as<int>());
    GA_HIP(hipGetLastError());
  }
  GA_HIP(hipMemsetAsync(flags.as<int>() + m, 0, sizeof(int), st));
  edit_unsort_kernel<<<mb, 256, 0, st>>>(vals, lv.as<int>(), m, level.as<int>(), flags.as<int>());
  GA_HIP(hipGetLastError());
  GA_TRY(pick_to_host(ctx, st, flags.as<int>(), m, sel.pairs.as<int>(), level.as<int>(), capacity, pairs, levels, &out->count));
  int h_seed = -1;
  GA_HIP(read_back_sync(ctx, st, &h_seed, seed.p, sizeof(int)));
  GA_HIP(read_back_sync(ctx, st, &out->seed_qq, seed_qq.p, sizeof(double)));
  if (h_seed < 0 || h_seed >= m) return GLIM_AMD_ERR_HIP;
  GA_HIP(read_back_sync(ctx, st, out->seed, sel.pairs.as<int>() + 2 * (size_t)h_seed, 2 * sizeof(int)));
  in_flight.dismiss();
  out->rounds = last;
  out->status = GLIM_AMD_EDIT_OK;
  return GLIM_AMD_OK;
}

int glim_amd_edit_min_cut(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12, const glim_amd_edit_window* window,
                          const glim_amd_edit_min_cut_params* params, int64_t capacity, int32_t* pairs, glim_amd_edit_min_cut_result* out) {
  using namespace glim_amd;
  using namespace glim_amd::edit;
  if (no_device()) return GLIM_AMD_ERR_NO_DEVICE;
  if (capacity < 0 || !out || (capacity > 0 && !pairs)) return GLIM_AMD_ERR_INVALID;
  MinCutSetup setup;
  GA_TRY(min_cut_setup(clouds, num_clouds, T_world_submap12, window, params, &setup));
  *out = glim_amd_edit_min_cut_result();
  out->status = GLIM_AMD_EDIT_EMPTY;
  if (num_clouds == 0) return GLIM_AMD_OK;
  MinCutGraph g;  // its transient cloud is destroyed after the lock scope below
  GA_TRY(min_cut_graph(clouds, num_clouds, T_world_submap12, setup, &g));
  min_cut_counts(g, out);
  if (g.status != GLIM_AMD_EDIT_OK) return GLIM_AMD_OK;
  glim_amd_ctx* ctx = clouds[0]->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  DeviceTemp flags;
  GA_HIP(pool_malloc(&flags.p, ((size_t)g.m + 1) * sizeof(int)));
  SyncOnExit in_flight(st);
  MaxFlowResult r;
  GA_TRY(max_flow_source_side(ctx, st, g.m, g.E, g.edges.as<int2>(), g.cap.as<int>(), g.src.as<int>(), g.snk.as<int>(), setup.prm.max_rounds, flags.as<int>(), &r));
  out->flow = r.flow, out->rounds = r.rounds, out->looks = r.looks, out->status = r.status;
  if (r.status == GLIM_AMD_EDIT_OK) GA_TRY(pick_to_host(ctx, st, flags.as<int>(), g.m, g.sel.pairs.as<int>(), nullptr, capacity, pairs, nullptr, &out->count));
  in_flight.dismiss();
  return GLIM_AMD_OK;
}

int glim_amd_diag_edit_min_cut_graph(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12,
                                     const glim_amd_edit_window* window, const glim_amd_edit_min_cut_params* params, int64_t pair_capacity, int32_t* pairs,
                                     int32_t* source_cap, int32_t* sink_cap, int64_t edge_capacity, int32_t* edges, int32_t* edge_cap,
                                     glim_amd_edit_min_cut_result* out) {
  using namespace glim_amd;
  using namespace glim_amd::edit;
  if (no_device()) return GLIM_AMD_ERR_NO_DEVICE;
  if (pair_capacity < 0 || edge_capacity < 0 || !out || (pair_capacity > 0 && (!pairs || !source_cap || !sink_cap)) ||
      (edge_capacity > 0 && (!edges || !edge_cap)))
    return GLIM_AMD_ERR_INVALID;
  MinCutSetup setup;
  GA_TRY(min_cut_setup(clouds, num_clouds, T_world_submap12, window, params, &setup));
  *out = glim_amd_edit_min_cut_result();
  out->status = GLIM_AMD_EDIT_EMPTY;
  if (num_clouds == 0) return GLIM_AMD_OK;
  MinCutGraph g;
  GA_TRY(min_cut_graph(clouds, num_clouds, T_world_submap12, setup, &g));
  min_cut_counts(g, out);
  glim_amd_ctx* ctx = clouds[0]->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  const size_t np = (size_t)std::min<int64_t>(pair_capacity, g.m);
  if (np > 0) GA_HIP(hipMemcpyAsync(pairs, g.sel.pairs.p, np * 2 * sizeof(int), hipMemcpyDeviceToHost, st));
  if (g.src.p) {  // the graph was built (status OK or NO_SEED)
    const size_t ne = (size_t)std::min<int64_t>(edge_capacity, g.E);
    if (np > 0) {
      GA_HIP(hipMemcpyAsync(source_cap, g.src.p, np * sizeof(int), hipMemcpyDeviceToHost, st));
      GA_HIP(hipMemcpyAsync(sink_cap, g.snk.p, np * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    if (ne > 0) {
      GA_HIP(hipMemcpyAsync(edges, g.edges.p, ne * sizeof(int2), hipMemcpyDeviceToHost, st));
      GA_HIP(hipMemcpyAsync(edge_cap, g.cap.p, ne * sizeof(int), hipMemcpyDeviceToHost, st));
    }
  }
  GA_HIP(hipStreamSynchronize(st));
  return GLIM_AMD_OK;
}

int glim_amd_edit_remove_points(const glim_amd_cloud* cloud, int64_t n, const int32_t* indices, glim_amd_cloud** out) {
  using namespace glim_amd;
  using namespace glim_amd::edit;
  if (no_device()) return GLIM_AMD_ERR_NO_DEVICE;
  if (!cloud || !out || n < 0 || (n > 0 && !indices) || n > (int64_t)0x7fffffff - 257) return GLIM_AMD_ERR_INVALID;
  *out = nullptr;
  const int size = (int)cloud->n;
  std::vector<char> removed((size_t)size, 0);
  for (int64_t i = 0; i < n; i++) {
    if (indices[i] < 0 || indices[i] >= size) return GLIM_AMD_ERR_INVALID;
    removed[(size_t)indices[i]] = 1;
  }
  glim_amd_ctx* ctx = cloud->ctx;
  CloudGuard result;  // destroyed after the lock
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  DeviceTemp idx, keep, pos, tiles;
  GA_HIP(pool_malloc(&idx.p, (size_t)std::max<int64_t>(n, 1) * sizeof(int)));
  GA_HIP(pool_malloc(&keep.p, (size_t)(size + 1) * sizeof(int)));
  GA_HIP(pool_malloc(&pos.p, (size_t)(size + 1) * sizeof(int)));
  GA_HIP(pool_malloc(&tiles.p, scan_scratch_ints((unsigned int)size + 1u) * sizeof(int)));
  SyncOnExit in_flight(st);
  if (n > 0) GA_HIP(hipMemcpyAsync(idx.p, indices, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
  edit_keep_fill_kernel<<<grid_for(size + 1), 256, 0, st>>>(size, keep.as<int>());
  if (n > 0) edit_keep_mark_kernel<<<grid_for((int)n), 256, 0, st>>>(idx.as<int>(), (int)n, keep.as<int>());
  GA_HIP(hipGetLastError());
  GA_HIP(exclusive_scan_int(st, keep.as<int>(), (unsigned int)size + 1u, tiles.as<int>(), pos.as<int>()));
  int kept = 0;
  GA_HIP(read_back_sync(ctx, st, &kept, pos.as<int>() + size, sizeof(int)));  // also: the index array has been read
  if (kept < 0 || kept > size) return GLIM_AMD_ERR_HIP;
  GA_TRY(alloc_cloud_like(cloud, kept, &result));
  glim_amd_cloud* c = result.c;
  if (kept > 0) GA_HIP(cloud_gather(st, size, keep.as<int>(), pos.as<int>(), nullptr, gather_args(cloud, c)));
  if (cloud->h_times.size() == (size_t)size) {
    c->h_times.reserve((size_t)kept);
    for (int i = 0; i < size; i++)
      if (!removed[(size_t)i]) c->h_times.push_back(cloud->h_times[(size_t)i]);
  }
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  *out = c;
  result.c = nullptr;
  return GLIM_AMD_OK;
}

// parity / debug only: scan.hpp's exclusive prefix sum of a host array on the device
int glim_amd_debug_exclusive_scan(glim_amd_ctx* ctx, int64_t n, const int32_t* in, int32_t* out) {
  using namespace glim_amd;
  if (!ctx || n < 0 || n > (int64_t)(1 << 28) || (n > 0 && (!in || !out))) return GLIM_AMD_ERR_INVALID;
  if (n == 0) return GLIM_AMD_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  const unsigned int T = (unsigned int)n;
  DeviceTemp d_in, d_out, tiles;
  GA_HIP(pool_malloc(&d_in.p, (size_t)T * sizeof(int)));
  GA_HIP(pool_malloc(&d_out.p, (size_t)T * sizeof(int)));
  GA_HIP(pool_malloc(&tiles.p, scan_scratch_ints(T) * sizeof(int)));
  SyncOnExit in_flight(st);
  GA_HIP(hipMemcpyAsync(d_in.p, in, (size_t)T * sizeof(int), hipMemcpyHostToDevice, st));
  GA_HIP(exclusive_scan_int(st, d_in.as<int>(), T, tiles.as<int>(), d_out.as<int>()));
  GA_HIP(hipMemcpyAsync(out, d_out.p, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  return GLIM_AMD_OK;
}

}  // extern "C"
