// gicp_factor.hpp -- what the translation units of the GICP family share (gicp.hip: the search index, the rigid and the continuous-time factor;
// ivox.hip: the device iVox; gicp_align.hip, ct_align.hip: the loops): the search index object and the factor kernels' arguments, the two searches
// (IndexSearch, IvoxSearch), the per-point algebra, the block epilogue and the ordered sum that make a record bit-reproducible, and the host's
// description of a target (GicpTarget).  Each of them is defined here, once.  Like knn_common.hpp the shared part is in an unnamed namespace:
// device functions are forced inline, the __constant__ tables are static (one copy per unit), the host helpers are a few lines each, and
// nothing of it is called across units -- a unit that runs a factor kernel instantiates it itself.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <mutex>

#include "device_math.hpp"
#include "internal.hpp"

struct glim_amd_nn_index {
  CtxRef ctx;
  const glim_amd_cloud* cloud = nullptr;  // not owned; must outlive the index
  int n = 0;
  double h = 0.0;                         // cell edge
  unsigned int mask = 0;                  // table size - 1 (power of two)
  unsigned long long* keys = nullptr;     // cell key per table slot (EMPTY_KEY when free)
  int2* runs = nullptr;                   // [begin, end) of the cell's run in the sorted order
  float4* sorted = nullptr;               // xyz + original index (int bits), cell order
  float4* covA = nullptr;                 // target covariances in the same order
  float2* covB = nullptr;
};

namespace {

using namespace glim_amd;

using u64 = unsigned long long;
using u32 = unsigned int;
constexpr int BLOCK = 256;
constexpr int NACC = 28;
constexpr int GICP_MAX_RING = 64;
// the walk counts a cell edge as this fraction of h, so that rounding in the cell assignment never makes a distance bound optimistic
constexpr double GICP_EDGE_SHRINK = 0.999999;
static __constant__ int c_acc_of_upper_g[21] = {0, 1, 2, 6, 7, 8, 3, 4, 9, 10, 11, 5, 12, 13, 14, 15, 16, 17, 18, 19, 20};

__device__ __forceinline__ u32 cell_hash(u64 key) {
  u64 z = key * 0x9E3779B97F4A7C15ull;
  z ^= z >> 29;
  return (u32)(z * 0xBF58476D1CE4E5B9ull >> 32);
}

// ---- the factor ----
struct GicpArgs {
  const float4* sorted;
  const float4* tA;
  const float2* tB;
  const u64* keys;
  const int2* runs;
  u32 mask;
  int nt;
  double h, inv_h;
  const float4* pts;   // source xyz1
  const float4* covA;  // source covariances
  const float2* covB;
  int n;
  int ppt;             // points per thread (chunk = 256 * ppt consecutive points per block)
  double T[12];
  double max_sq;       // max_correspondence_distance^2
  int max_ring;        // rings after which the scanned cube covers the correspondence radius
};

__device__ __forceinline__ double sqdist_nc(double qx, double qy, double qz, double x, double y, double z) {
  const double dx = qx - x, dy = qy - y, dz = qz - z;
  return dadd(dadd(dmul(dx, dx), dmul(dy, dy)), dmul(dz, dz));
}

// exact nearest target point of q within sqrt(max_sq): position in the sorted order, or -1
__device__ __forceinline__ int nearest(const GicpArgs& a, double qx, double qy, double qz, double& best_d) {
  const double tx = qx * a.inv_h, ty = qy * a.inv_h, tz = qz * a.inv_h;
  if (!(tx >= -1048576.0 && tx < 1048576.0 && ty >= -1048576.0 && ty < 1048576.0 && tz >= -1048576.0 && tz < 1048576.0)) return -1;
  const int cx = fast_floor_d(tx), cy = fast_floor_d(ty), cz = fast_floor_d(tz);
  double margin = fmin(fmin(tx - (double)cx, (double)(cx + 1) - tx), fmin(fmin(ty - (double)cy, (double)(cy + 1) - ty), fmin(tz - (double)cz, (double)(cz + 1) - tz)));
  margin = fmax(0.0, margin * a.h * GICP_EDGE_SHRINK);
  int best = -1, best_idx = 0x7fffffff;
  best_d = __longlong_as_double(0x7ff0000000000000ll);
  for (int ring = 0; ring <= a.max_ring; ring++) {
    if (ring >= 1) {
      const double reach = (double)(ring - 1) * a.h * GICP_EDGE_SHRINK + margin;  // every unscanned point is at least this far
      const double r2 = reach * reach;
      if (best_d < r2 || r2 > a.max_sq) break;  // proven nearest (strict: an unscanned tie could carry a smaller index) / beyond the radius
    }
    for (int dz = -ring; dz <= ring; dz++)
      for (int dy = -ring; dy <= ring; dy++) {
        const bool shell_yz = (abs(dz) == ring) || (abs(dy) == ring);
        for (int dx = -ring; dx <= ring; dx += (shell_yz || ring == 0) ? 1 : 2 * ring) {
          if (ring >= 1) {
            // prune: no point of this cell is closer than the gap between q and the cell's box (shrunk so that rounding in the cell
            // assignment cannot make it optimistic); strictly greater than the current best / the radius, so ties are still seen
            const double gx = dx > 0 ? (double)(cx + dx) - tx : (dx < 0 ? tx - (double)(cx + dx + 1) : 0.0);
            const double gy = dy > 0 ? (double)(cy + dy) - ty : (dy < 0 ? ty - (double)(cy + dy + 1) : 0.0);
            const double gz = dz > 0 ? (double)(cz + dz) - tz : (dz < 0 ? tz - (double)(cz + dz + 1) : 0.0);
            const double gap = a.h * GICP_EDGE_SHRINK;
            const double ex = fmax(0.0, gx) * gap, ey = fmax(0.0, gy) * gap, ez = fmax(0.0, gz) * gap;
            const double g2 = ex * ex + ey * ey + ez * ez;
            if (g2 > best_d || g2 > a.max_sq) continue;
          }
          const u32 ux = (u32)(cx + dx + KEY_OFFSET), uy = (u32)(cy + dy + KEY_OFFSET), uz = (u32)(cz + dz + KEY_OFFSET);
          if ((ux | uy | uz) >> KEY_BITS) continue;
          const u64 key = (u64)ux | ((u64)uy << 21) | ((u64)uz << 42);
          u32 s = cell_hash(key) & a.mask;
          int2 run = make_int2(0, 0);
          for (;;) {
            const u64 kk = a.keys[s];
            if (kk == key) {
              run = a.runs[s];
              break;
            }
            if (kk == EMPTY_KEY) break;
            s = (s + 1) & a.mask;
          }
          for (int j = run.x; j < run.y; j++) {
            const float4 c = a.sorted[j];
            const double d = sqdist_nc(qx, qy, qz, (double)c.x, (double)c.y, (double)c.z);
            const int idx = __float_as_int(c.w);
            if (d < best_d || (d == best_d && idx < best_idx)) {
              best_d = d;
              best = j;
              best_idx = idx;
            }
          }
        }
      }
  }
  return (best >= 0 && best_d <= a.max_sq) ? best : -1;
}

// the target kind of the factor kernels: where a transformed source point finds its correspondence.  IndexSearch is the exact search above.
struct IndexSearch {
  __device__ __forceinline__ int find(const GicpArgs& a, double qx, double qy, double qz, double& best_d) const { return nearest(a, qx, qy, qz, best_d); }
};

// Neighbour offsets of the incremental voxel map's search (gtsam_points::IncrementalVoxelMap::set_neighbor_voxel_mode): modes 1, 7 and 19 are
// prefixes of this list (centre; the six faces +x -x +y -y +z -z; the twelve edges); mode 27 is the full cube, z outermost and x innermost.
static __constant__ int c_ivox_offsets[19][3] = {{0, 0, 0},  {1, 0, 0},  {-1, 0, 0}, {0, 1, 0},  {0, -1, 0}, {0, 0, 1},  {0, 0, -1},
                                          {1, 1, 0},  {1, -1, 0}, {-1, 1, 0}, {-1, -1, 0}, {1, 0, 1},  {1, 0, -1}, {-1, 0, 1},
                                          {-1, 0, -1}, {0, 1, 1},  {0, 1, -1}, {0, -1, 1}, {0, -1, -1}};

// IvoxSearch: the target is a device iVox (ivox_map.hpp).  a.sorted / a.tA / a.tB are the map's point and covariance arrays, `cap` entries per
// slot; position = slot * cap + place in the cell, which is also what the point's w holds.  NOT an exact nearest-neighbour search: only the
// cells of the neighbour mode around q's own cell are visited (upstream's behaviour).  Smallest FP64 (dx^2 + dy^2) + dz^2; a later candidate
// replaces the best only when strictly smaller; valid iff d^2 <= max_correspondence_distance^2.
struct IvoxSearch {
  const u64* keys;    // open-addressing table: voxel key per entry (EMPTY_KEY when free)
  const int* slots;   // slot of the entry's voxel
  const int* counts;  // points per slot
  u32 mask;
  int cap;            // max_num_points_in_cell
  int nnb;            // 1 | 7 | 19 | 27
  double inv_leaf;
  __device__ __forceinline__ int find(const GicpArgs& a, double qx, double qy, double qz, double& best_d) const {
    best_d = __longlong_as_double(0x7ff0000000000000ll);
    const double tx = qx * inv_leaf, ty = qy * inv_leaf, tz = qz * inv_leaf;
    if (!(tx >= -1048576.0 && tx < 1048576.0 && ty >= -1048576.0 && ty < 1048576.0 && tz >= -1048576.0 && tz < 1048576.0)) return -1;
    const int cx = fast_floor_d(tx), cy = fast_floor_d(ty), cz = fast_floor_d(tz);
    int best = -1;
    for (int k = 0; k < nnb; k++) {
      int dx, dy, dz;
      if (nnb == 27) {
        dx = k % 3 - 1;
        dy = (k / 3) % 3 - 1;
        dz = k / 9 - 1;
      } else {
        dx = c_ivox_offsets[k][0];
        dy = c_ivox_offsets[k][1];
        dz = c_ivox_offsets[k][2];
      }
      const u32 ux = (u32)(cx + dx + KEY_OFFSET), uy = (u32)(cy + dy + KEY_OFFSET), uz = (u32)(cz + dz + KEY_OFFSET);
      if ((ux | uy | uz) >> KEY_BITS) continue;
      const u64 key = (u64)ux | ((u64)uy << 21) | ((u64)uz << 42);
      u32 s = cell_hash(key) & mask;
      int slot = -1;
      for (;;) {
        const u64 kk = keys[s];
        if (kk == key) {
          slot = slots[s];
          break;
        }
        if (kk == EMPTY_KEY) break;
        s = (s + 1) & mask;
      }
      if (slot < 0) continue;
      const int first = slot * cap, last = first + counts[slot];
      for (int j = first; j < last; j++) {
        const float4 c = a.sorted[j];
        const double d = sqdist_nc(qx, qy, qz, (double)c.x, (double)c.y, (double)c.z);
        if (d < best_d) {
          best_d = d;
          best = j;
        }
      }
    }
    return (best >= 0 && best_d <= a.max_sq) ? best : -1;
  }
};

// per-point GICP algebra in the source frame (gicp_kernel and ct_gicp_kernel): adds the point's terms to the 28 accumulators and returns the
// source-frame A = (R^T C_B R + C_A)^-1 (a00 a01 a02 a11 a12 a22)
template <bool LINEARIZE>
__device__ __forceinline__ void gicp_point(float (&acc)[NACC], float R00, float R01, float R02, float R10, float R11, float R12, float R20, float R21,
                                           float R22, const float4 p, const float4 b, const float4 tA, const float2 tB, const float4 ca, const float2 cb,
                                           double qx, double qy, double qz, float (&A)[6]) {
  // residual b_j - q: formed in FP64 (|r| <= the correspondence radius), then FP32
  const float rx = (float)((double)b.x - qx), ry = (float)((double)b.y - qy), rz = (float)((double)b.z - qz);
  // S = R^T C_B R + C_A (source frame, symmetric)
  const float b00 = tA.x, b01 = tA.y, b02 = tA.z, b11 = tA.w, b12 = tB.x, b22 = tB.y;
  const float w00 = b00 * R00 + b01 * R10 + b02 * R20, w01 = b00 * R01 + b01 * R11 + b02 * R21, w02 = b00 * R02 + b01 * R12 + b02 * R22;
  const float w10 = b01 * R00 + b11 * R10 + b12 * R20, w11 = b01 * R01 + b11 * R11 + b12 * R21, w12 = b01 * R02 + b11 * R12 + b12 * R22;
  const float w20 = b02 * R00 + b12 * R10 + b22 * R20, w21 = b02 * R01 + b12 * R11 + b22 * R21, w22 = b02 * R02 + b12 * R12 + b22 * R22;
  const float S00 = ca.x + R00 * w00 + R10 * w10 + R20 * w20;
  const float S01 = ca.y + R00 * w01 + R10 * w11 + R20 * w21;
  const float S02 = ca.z + R00 * w02 + R10 * w12 + R20 * w22;
  const float S11 = ca.w + R01 * w01 + R11 * w11 + R21 * w21;
  const float S12 = cb.x + R01 * w02 + R11 * w12 + R21 * w22;
  const float S22 = cb.y + R02 * w02 + R12 * w12 + R22 * w22;
  const float k00 = S11 * S22 - S12 * S12;
  const float k01 = S02 * S12 - S01 * S22;
  const float k02 = S01 * S12 - S02 * S11;
  const float det = S00 * k00 + S01 * k01 + S02 * k02;
  float idet = __builtin_amdgcn_rcpf(det);
  idet = fmaf(fmaf(-det, idet, 1.0f), idet, idet);
  const float A00 = k00 * idet, A01 = k01 * idet, A02 = k02 * idet;
  const float A11 = (S00 * S22 - S02 * S02) * idet;
  const float A12 = (S01 * S02 - S00 * S12) * idet;
  const float A22 = (S00 * S11 - S01 * S01) * idet;
  const float rsx = R00 * rx + R10 * ry + R20 * rz;
  const float rsy = R01 * rx + R11 * ry + R21 * rz;
  const float rsz = R02 * rx + R12 * ry + R22 * rz;
  const float ux = A00 * rsx + A01 * rsy + A02 * rsz;
  const float uy = A01 * rsx + A11 * rsy + A12 * rsz;
  const float uz = A02 * rsx + A12 * rsy + A22 * rsz;
  acc[27] += rsx * ux + rsy * uy + rsz * uz;
  if (LINEARIZE) {
    const float x = p.x, y = p.y, z = p.z;
    const float g00 = y * A02 - z * A01, g01 = y * A12 - z * A11, g02 = y * A22 - z * A12;
    const float g10 = z * A00 - x * A02, g11 = z * A01 - x * A12, g12 = z * A02 - x * A22;
    const float g20 = x * A01 - y * A00, g21 = x * A11 - y * A01, g22 = x * A12 - y * A02;
    acc[0] += y * g02 - z * g01;
    acc[1] += z * g00 - x * g02;
    acc[2] += x * g01 - y * g00;
    acc[3] += z * g10 - x * g12;
    acc[4] += x * g11 - y * g10;
    acc[5] += x * g21 - y * g20;
    acc[6] += g00; acc[7] += g01; acc[8] += g02;
    acc[9] += g10; acc[10] += g11; acc[11] += g12;
    acc[12] += g20; acc[13] += g21; acc[14] += g22;
    acc[15] += A00; acc[16] += A01; acc[17] += A02; acc[18] += A11; acc[19] += A12; acc[20] += A22;
    acc[21] += uy * z - uz * y;
    acc[22] += uz * x - ux * z;
    acc[23] += ux * y - uy * x;
    acc[24] += ux; acc[25] += uy; acc[26] += uz;
  }
  A[0] = A00; A[1] = A01; A[2] = A02; A[3] = A11; A[4] = A12; A[5] = A22;
}

// the FP32 rotation of a row-major 3 x 4 pose, entry by entry as gicp_point takes it
struct Rot32 {
  float r00, r01, r02, r10, r11, r12, r20, r21, r22;
  __device__ __forceinline__ explicit Rot32(const double* T)
      : r00((float)T[0]), r01((float)T[1]), r02((float)T[2]), r10((float)T[4]), r11((float)T[5]), r12((float)T[6]), r20((float)T[8]), r21((float)T[9]), r22((float)T[10]) {}
};

// The block epilogue of the factor kernels (BLOCK = 4 waves): the order of additions that makes a partial row bit-reproducible.  Every wave sums
// its lanes into lane 63 (DPP, step-major: device_math.hpp; the same six additions per value) and leaves the sums in s_red[wave]; (0 + 1) + (2 + 3).
template <int W>
__device__ __forceinline__ float sum_of_waves(const float (&s_red)[4][W], int j) {
  return (s_red[0][j] + s_red[1][j]) + (s_red[2][j] + s_red[3][j]);
}
// the 28 accumulators to columns 0..27 of the block's partial row, the inlier count to column 28, zero above
__device__ __forceinline__ void store_partial_row(float (&acc)[NACC], int inliers, float (&s_red)[4][PARTIAL_STRIDE], float* __restrict__ partials) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  wave_sums_to_lane63<NACC>(acc);
  if (lane == 63) {
#pragma unroll
    for (int j = 0; j < NACC; j++) s_red[wave][j] = acc[j];
  }
  const float v = wave_sum_to_lane63((float)inliers);
  if (lane == 63) s_red[wave][28] = v;
  __syncthreads();
  if (threadIdx.x < PARTIAL_STRIDE) {
    const int j = threadIdx.x;
    partials[(size_t)blockIdx.x * PARTIAL_STRIDE + j] = j <= 28 ? sum_of_waves(s_red, j) : 0.f;
  }
}

// One group's share of a fixed-order column sum (same order as vgicp.hip's finalize_factor): group g of 8 adds rows g, g + 8, g + 16, ... of
// column j in that order, with the (clamped) loads of INFLIGHT trips in flight at a time.  The caller then adds the 8 groups in order.
template <class T, int STRIDE, int INFLIGHT>
__device__ __forceinline__ double ordered_column_sum(const T* __restrict__ rows, int n, int j, int g) {
  double s = 0.0;
  for (int c = g; c < n; c += 8 * INFLIGHT) {
    T v[INFLIGHT];
#pragma unroll
    for (int u = 0; u < INFLIGHT; u++) v[u] = rows[(size_t)min(c + 8 * u, n - 1) * STRIDE + j];
#pragma unroll
    for (int u = 0; u < INFLIGHT; u++)
      if (c + 8 * u < n) s += (double)v[u];
  }
  return s;
}

// The two steps of the finaliser (a block of 256 threads; gicp.hip's gicp_finalize_kernel and the decide kernel of gicp_align.hip): the fixed-order FP64 sum of `nb`
// partial rows -- 8 groups of ordered_column_sum, then the groups in order -- into s_sum, and entry t of the linearising compact record from it.
__device__ __forceinline__ void sum_partial_rows(const float* __restrict__ partials, int nb, double (&s_part)[8][PARTIAL_STRIDE], double (&s_sum)[PARTIAL_STRIDE]) {
  const int j = threadIdx.x & 31, g = threadIdx.x >> 5;
  s_part[g][j] = ordered_column_sum<float, PARTIAL_STRIDE, 16>(partials, nb, j, g);
  __syncthreads();
  if (threadIdx.x < PARTIAL_STRIDE) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 8; k++) t += s_part[k][threadIdx.x];
    s_sum[threadIdx.x] = t;
  }
  __syncthreads();
}
__device__ __forceinline__ double compact_entry(const double (&s_sum)[PARTIAL_STRIDE], int t) {
  if (t == 0) return s_sum[28];
  if (t == 1) return s_sum[27];
  if (t < 23) return s_sum[c_acc_of_upper_g[t - 2]];
  return t < 26 ? s_sum[t - 2] : -s_sum[t - 2];
}

inline int grid_for(int n) { return (n + 255) / 256; }
unsigned int next_pow2(unsigned long long v) {
  unsigned long long p = 1;
  while (p < v) p <<= 1;
  return (unsigned int)p;
}

// the search is latency-bound: spread the points over >= 4 blocks per CU when there are enough of them
int points_per_thread(const glim_amd_ctx* ctx, int n) {
  const int target_blocks = std::max(1, ctx->num_cus * 4);
  return std::max(1, std::min(64, (n + BLOCK * target_blocks - 1) / (BLOCK * target_blocks)));
}

// ---- a target the factor kernels can search, as the host sees it ----
// Everything the two kinds differ in, as data: built by gicp_target() from a search index (below) or from a device iVox (ivox_map.hpp), read by
// gicp.hip's run_gicp and run_ct, which do not ask for the kind.  A map changes under insert, so the description holds the context's mutex from the moment
// it is taken: what it says stays true, and its arrays stay where they are, for as long as it lives.  That is also the lock of the evaluation.
struct GicpTarget {
  glim_amd_ctx* ctx = nullptr;  // null: no target was given
  std::unique_lock<std::mutex> held;
  GicpArgs args{};              // the target half filled (sorted .. inv_h), the source half zero
  bool ivox = false;            // the search object: `nn` when set, IndexSearch otherwise (with_search)
  IvoxSearch nn{};
  bool usable = true;           // the target has covariances
  const float4* normals = nullptr;  // the target cloud's normals in its original order, or null (an index only: the ICP factors)
  bool empty = true;            // nothing to find: every point is an outlier
  int ring_cap = 0;             // most rings the index's walk may take; 0: no walk (a map searches the cells of its neighbour mode)
  int64_t max_source = INT64_MAX;  // source points beyond which the kind's entry points refuse the call
  uint64_t generation = 0;      // moves when positions in the target change their meaning (never for an index)
  // rings after which the scanned cube covers the correspondence radius `d`: the first ring R whose reach R * h * GICP_EDGE_SHRINK, as
  // nearest() counts it, is no less than d -- by that same count every point beyond ring R is farther than d, so a further ring finds nothing.
  // The walk is bounded: a radius that needs more than ring_cap rings (d beyond ring_cap * h * GICP_EDGE_SHRINK, with h between hint / 3
  // and hint; so 21 x hint always fits) is refused rather than searched incompletely: -1
  int rings(double d) const {
    if (ring_cap == 0) return 0;
    const double r = std::ceil(d / (args.h * GICP_EDGE_SHRINK));
    return r <= (double)ring_cap ? (int)r : -1;
  }
};

// (lock = false: the caller already holds the context's mutex -- a batch of targets of one context, gicp_align.hip)
GicpTarget gicp_target(const glim_amd_nn_index* ix, bool lock = true) {
  GicpTarget t;
  if (!ix) return t;
  t.ctx = ix->ctx;
  if (lock) t.held = std::unique_lock<std::mutex>(t.ctx->mu);
  t.args.sorted = ix->sorted;
  t.args.tA = ix->covA;
  t.args.tB = ix->covB;
  t.args.keys = ix->keys;
  t.args.runs = ix->runs;
  t.args.mask = ix->mask;
  t.args.nt = ix->n;
  t.args.h = ix->h;
  t.args.inv_h = 1.0 / ix->h;
  t.usable = ix->covA != nullptr;
  t.normals = (ix->cloud && ix->cloud->has_normals) ? ix->cloud->normals : nullptr;
  t.empty = ix->n == 0;
  t.ring_cap = GICP_MAX_RING;
  return t;
}

// which per-point algebra a rigid evaluation runs: the GICP factor's (gicp_point), or one of the ICP factors' (icp_factor.hpp) over a search index
enum class Metric { GICP, ICP_POINT, ICP_PLANE };
inline Metric icp_metric(uint32_t flags) { return (flags & GLIM_AMD_ICP_POINT_TO_PLANE) ? Metric::ICP_PLANE : Metric::ICP_POINT; }
// what a metric needs of its clouds: GLIM_AMD_OK or GLIM_AMD_ERR_STATE
inline int metric_state(Metric m, const GicpTarget& t, const glim_amd_cloud* source) {
  if (m == Metric::GICP) return (source->has_covs && t.usable) ? GLIM_AMD_OK : GLIM_AMD_ERR_STATE;
  if (t.ivox) return GLIM_AMD_ERR_STATE;  // (no entry point reaches this: the ICP factors take a search index)
  return (m == Metric::ICP_PLANE && !t.normals) ? GLIM_AMD_ERR_STATE : GLIM_AMD_OK;
}

// the source half of the kernels' arguments
void set_source(GicpArgs* a, const glim_amd_cloud* source, int ppt, double max_dist) {
  a->pts = source->pts;
  a->covA = source->covA;
  a->covB = source->covB;
  a->n = (int)source->n;
  a->ppt = ppt;
  a->max_sq = max_dist * max_dist;
}

// the one place where the target's kind becomes the NN template argument of a factor kernel: launch(search object)
template <class Launch>
void with_search(const GicpTarget& t, Launch&& launch) {
  if (t.ivox) launch(t.nn);
  else launch(IndexSearch{});
}

}  // namespace
