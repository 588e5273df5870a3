// fpfh.hip -- FPFH descriptors of a device cloud and nearest-descriptor matching on gfx950: the two data-parallel stages of global registration
// (gtsam_points::estimate_fpfh and the KdTreeX<FPFH_DIM> queries of viewer/interactive/manual_loop_close_modal.cpp:376-463).  Semantics in
// include/glim_amd.h ("FPFH"), layout and measurements in DESIGN.md 4.7.  fpfh.hpp declares what the global-registration entries use of this
// file: the descriptor object and the matcher's device side.
//
// estimate:  cell grid of edge >= r over the cloud (cells dense inside the bounding box, one border cell all round; stable radix sort of sort.hip
//            on the cell index, exclusive scan of scan.hpp over the cell counts), so the neighbours of a point lie in the 27 cells around it = 9
//            contiguous runs of the sorted order.  One wavefront per query point walks those runs 64 candidates at a time, keeps the ones with
//            0 < d^2 <= r^2 (FP64) in a ring in LDS in candidate order, and hands them out 64 at a time, so the expensive part -- the pair
//            feature of pass one, the 33 weighted adds of pass two -- runs on full wavefronts.
//   pass 1   SPFH: FP64 pair feature per neighbour, three bins, integer counts in LDS; S = count * 100 / k per point, 34 doubles per row
//   pass 2   FPFH: per-lane FP64 sums of S_j / d^2 over the lane's neighbours (ring order: fixed), xor-butterfly over the lanes (fixed tree),
//            per-block rescale to 100, ONE rounding to FP32
//            No floating-point atomics anywhere; the only atomics are integer (cell counts, bin counts): two calls return the same bits.
// match:     128 x 128 all-pairs tiles in LDS, 8 x 8 FP32 FMA micro-tile per lane, d = (|a|^2 + |b|^2) - 2 a.b with the norms stored beside the
//            descriptors, running (distance, index) argmin per source row, ordered merge over the target splits.  Every (i, j) distance is the
//            same FMA chain whichever lane or direction computes it, so the forward and the reciprocal pass agree on every tie.
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "device_math.hpp"
#include "fpfh.hpp"
#include "internal.hpp"
#include "scan.hpp"
#include "scope_sync.hpp"

namespace glim_amd {
namespace fpfh_detail {

using u64 = unsigned long long;
using u32 = unsigned int;
constexpr int FPFH_DIM = 33;
constexpr int FPFH_STRIDE = 36;     // floats per descriptor row on the device
constexpr int SPFH_STRIDE = 34;     // doubles per SPFH row (16-byte loads)
constexpr int MAX_CELLS = 1 << 22;  // dense cell grid: the cell edge doubles until the padded bounding box holds at most this many
constexpr double FP_PI = 3.14159265358979323846;

// ---- grid build ----
__global__ __launch_bounds__(256) void fp_key_kernel(int n, const float4* __restrict__ pts, double inv_h, u64* __restrict__ vkey, int* __restrict__ bb) {
  __shared__ int s_bb[6];
  if (threadIdx.x < 3) s_bb[threadIdx.x] = 0x7fffffff;
  else if (threadIdx.x < 6) s_bb[threadIdx.x] = (int)0x80000000;
  __syncthreads();
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float4 p = pts[i];
    const double t[3] = {(double)p.x * inv_h, (double)p.y * inv_h, (double)p.z * inv_h};
    bool valid = true;
#pragma unroll
    for (int a = 0; a < 3; a++) valid = valid && (t[a] >= -1048576.0 && t[a] < 1048576.0);  // (false for NaN)
    u64 key = EMPTY_KEY;
    if (valid) {
      int c[3];
#pragma unroll
      for (int a = 0; a < 3; a++) {
        c[a] = fast_floor_d(t[a]) + KEY_OFFSET;
        atomicMin(&s_bb[a], c[a]);
        atomicMax(&s_bb[3 + a], c[a]);
      }
      key = (u64)c[0] | ((u64)c[1] << 21) | ((u64)c[2] << 42);
    }
    vkey[i] = key;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    if (s_bb[threadIdx.x] != 0x7fffffff) atomicMin(&bb[threadIdx.x], s_bb[threadIdx.x]);
  } else if (threadIdx.x < 6) {
    if (s_bb[threadIdx.x] != (int)0x80000000) atomicMax(&bb[threadIdx.x], s_bb[threadIdx.x]);
  }
}

// cell index inside the padded box (x innermost) and the cell counts; points without a cell get `ncells` and sort last
__global__ __launch_bounds__(256) void fp_cell_kernel(int n, const u64* __restrict__ vkey, int ox, int oy, int oz, int nx, int ny, int ncells,
                                                      u64* __restrict__ ckey, int* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u64 k = vkey[i];
  if (k == EMPTY_KEY) {
    ckey[i] = (u64)ncells;
    return;
  }
  const int x = (int)(k & 0x1FFFFFull) - ox, y = (int)((k >> 21) & 0x1FFFFFull) - oy, z = (int)((k >> 42) & 0x1FFFFFull) - oz;
  const int c = (z * ny + y) * nx + x;
  ckey[i] = (u64)c;
  atomicAdd(&counts[c], 1);
}

__global__ __launch_bounds__(256) void fp_gather_kernel(int n, const u64* __restrict__ ckey_sorted, const u32* __restrict__ order,
                                                        const float4* __restrict__ pts, const float4* __restrict__ normals,
                                                        float4* __restrict__ spts, float4* __restrict__ snrm, int* __restrict__ scell) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const u32 i = order[j];
  const float4 p = pts[i];
  spts[j] = make_float4(p.x, p.y, p.z, __int_as_float((int)i));
  snrm[j] = normals[i];
  scell[j] = (int)ckey_sorted[j];
}

struct Grid {
  const float4* spts;  // xyz + original index (int bits), (cell, original index) order
  const float4* snrm;
  const int* scell;    // cell of every sorted point
  const int* first;    // first[c] = sorted points in cells < c, c in [0, ncells]
  int nx, ny;
  int nvalid;          // sorted points that have a cell
  double r2;
};

// ---- the neighbour walk both passes share ----
// Calls f(j, d2) once for every j with 0 < d2 <= r2, d2 = (dx^2 + dy^2) + dz^2 in FP64 with separate roundings, j = position in the sorted order.
// All 64 lanes of the block (= one wavefront) enter; lane l of the t-th hand-out gets the (64 t + l)-th neighbour in walk order (rows (dz, dy)
// outermost, sorted position innermost).  Returns k = |N(q)| in every lane.  s_j / s_d: rings of 128 entries.
template <class F>
__device__ __forceinline__ int walk_neighbours(const Grid& g, int q, int* s_j, double* s_d, F&& f) {
  const int lane = threadIdx.x;
  const float4 pq = g.spts[q];
  const double px = (double)pq.x, py = (double)pq.y, pz = (double)pq.z;
  const int cell = g.scell[q];
  int head = 0, held = 0, k = 0;
  for (int dz = -1; dz <= 1; dz++)
    for (int dy = -1; dy <= 1; dy++) {
      // (the border cell all round the box keeps cell - 1 .. cell + 1 of every row inside the grid)
      const int c0 = cell + (dz * g.ny + dy) * g.nx;
      const int begin = g.first[c0 - 1], end = g.first[c0 + 2];
      for (int base = begin; base < end; base += 64) {
        const int j = base + lane;
        bool in = false;
        double d2 = 0.0;
        if (j < end) {
          const float4 c = g.spts[j];
          const double dx = (double)c.x - px, ddy = (double)c.y - py, ddz = (double)c.z - pz;
          d2 = dadd(dadd(dmul(dx, dx), dmul(ddy, ddy)), dmul(ddz, ddz));
          in = d2 > 0.0 && d2 <= g.r2;
        }
        const u64 m = __ballot(in);
        if (in) {
          const int pos = (head + held + __popcll(m & ((1ull << lane) - 1ull))) & 127;
          s_j[pos] = j;
          s_d[pos] = d2;
        }
        const int got = __popcll(m);
        held += got;
        k += got;
        __syncthreads();
        if (held >= 64) {
          const int pos = (head + lane) & 127;
          f(s_j[pos], s_d[pos]);
          head = (head + 64) & 127;
          held -= 64;
          __syncthreads();
        }
      }
    }
  if (lane < held) {
    const int pos = (head + lane) & 127;
    f(s_j[pos], s_d[pos]);
  }
  return k;
}

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) { return fma(ax, bx, fma(ay, by, az * bz)); }
__device__ __forceinline__ int bin11(double t) {  // t = 11 * (normalised feature): floor, clamped to 0..10
  const int b = (int)floor(t);
  return b < 0 ? 0 : (b > 10 ? 10 : b);
}

// pass 1: SPFH of every sorted point
__global__ __launch_bounds__(64) void spfh_kernel(const Grid g, double* __restrict__ S) {
  __shared__ int s_j[128];
  __shared__ double s_d[128];
  __shared__ int s_hist[FPFH_DIM];
  const int q = blockIdx.x, lane = threadIdx.x;
  if (lane < FPFH_DIM) s_hist[lane] = 0;
  __syncthreads();
  const float4 pq = g.spts[q], nq = g.snrm[q];
  const double px = (double)pq.x, py = (double)pq.y, pz = (double)pq.z;
  const double nix = (double)nq.x, niy = (double)nq.y, niz = (double)nq.z;
  const int k = walk_neighbours(g, q, s_j, s_d, [&](int j, double d2) {
    const float4 pj = g.spts[j], nj4 = g.snrm[j];
    double dx = (double)pj.x - px, dy = (double)pj.y - py, dz = (double)pj.z - pz;
    const double njx = (double)nj4.x, njy = (double)nj4.y, njz = (double)nj4.z;
    const double f4 = sqrt(d2);
    const double a1 = dot3(nix, niy, niz, dx, dy, dz) / f4, a2 = dot3(njx, njy, njz, dx, dy, dz) / f4;
    double n1x = nix, n1y = niy, n1z = niz, n2x = njx, n2y = njy, n2z = njz, f3 = a1;
    if (fabs(a1) < fabs(a2)) {
      n1x = njx, n1y = njy, n1z = njz, n2x = nix, n2y = niy, n2z = niz;
      dx = -dx, dy = -dy, dz = -dz;
      f3 = -a2;
    }
    double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;  // v = dp x n1
    const double vn = sqrt(dot3(vx, vy, vz, vx, vy, vz));
    if (vn == 0.0) return;  // skipped, but counted in k
    vx /= vn, vy /= vn, vz /= vn;
    const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;  // w = n1 x v
    const double f2 = dot3(vx, vy, vz, n2x, n2y, n2z);
    const double f1 = atan2(dot3(wx, wy, wz, n2x, n2y, n2z), dot3(n1x, n1y, n1z, n2x, n2y, n2z));
    atomicAdd(&s_hist[bin11(11.0 * (f1 + FP_PI) / (2.0 * FP_PI))], 1);
    atomicAdd(&s_hist[11 + bin11(11.0 * (f2 + 1.0) / 2.0)], 1);
    atomicAdd(&s_hist[22 + bin11(11.0 * (f3 + 1.0) / 2.0)], 1);
  });
  __syncthreads();
  if (lane < SPFH_STRIDE) {
    double v = 0.0;
    if (lane < FPFH_DIM && k > 0) v = (double)(s_hist[lane] * 100) / (double)k;
    S[(size_t)q * SPFH_STRIDE + lane] = v;
  }
}

// pass 2: F_i = sum_j S_j * (1 / d2_ij), each 11-bin block rescaled to 100, one rounding to FP32; row of the point's ORIGINAL index
__global__ __launch_bounds__(64) void fpfh_kernel(const Grid g, const double* __restrict__ S, float* __restrict__ desc) {
  __shared__ int s_j[128];
  __shared__ double s_d[128];
  __shared__ double s_f[FPFH_DIM];
  __shared__ float s_o[FPFH_DIM];
  const int q = blockIdx.x, lane = threadIdx.x;
  double acc[FPFH_DIM];
#pragma unroll
  for (int b = 0; b < FPFH_DIM; b++) acc[b] = 0.0;
  walk_neighbours(g, q, s_j, s_d, [&](int j, double d2) {
    const double w = 1.0 / d2;
    const double2* row = reinterpret_cast<const double2*>(S + (size_t)j * SPFH_STRIDE);
#pragma unroll
    for (int b = 0; b < 16; b++) {
      const double2 s = row[b];
      acc[2 * b] = fma(s.x, w, acc[2 * b]);
      acc[2 * b + 1] = fma(s.y, w, acc[2 * b + 1]);
    }
    acc[32] = fma(row[16].x, w, acc[32]);
  });
  // the 33 lane sums: step-major, so that the 33 chains of a step are independent of one another
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int b = 0; b < FPFH_DIM; b++) acc[b] += __shfl_xor(acc[b], off, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int b = 0; b < FPFH_DIM; b++) s_f[b] = acc[b];
  }
  __syncthreads();
  if (lane < FPFH_DIM) {
    const int b0 = (lane / 11) * 11;
    double sum = 0.0;
    for (int b = 0; b < 11; b++) sum += s_f[b0 + b];
    const double v = s_f[lane];
    s_o[lane] = (float)(sum != 0.0 ? v * (100.0 / sum) : v);
  }
  __syncthreads();
  float* out = desc + (size_t)__float_as_int(g.spts[q].w) * FPFH_STRIDE;
  if (lane < FPFH_DIM) out[lane] = s_o[lane];
  if (lane == 0) {
    float nn = 0.0f;
    for (int b = 0; b < FPFH_DIM; b++) nn = fmaf(s_o[b], s_o[b], nn);  // the matcher's chain of a row with itself
    out[33] = nn;
    out[34] = 0.0f;
    out[35] = 0.0f;
  }
}

// ---- matcher ----
constexpr int MT = 128;        // rows per tile, both sides
constexpr int MT_PITCH = 132;  // floats per k-row of a tile in LDS

__device__ __forceinline__ void load_tile(const float* __restrict__ desc, int rows, int row0, float* s_t, float* s_n) {
  for (int idx = threadIdx.x; idx < MT * FPFH_STRIDE; idx += 256) {
    const int r = idx / FPFH_STRIDE, k = idx - r * FPFH_STRIDE;
    if (k > FPFH_DIM) continue;
    const float v = (row0 + r < rows) ? desc[(size_t)(row0 + r) * FPFH_STRIDE + k] : 0.0f;
    if (k < FPFH_DIM) s_t[k * MT_PITCH + r] = v;
    else s_n[r] = v;
  }
}

// block (x, y): source rows [128 x, 128 x + 128) against target tiles [y * tiles_per_split, (y + 1) * tiles_per_split); part_*[y][row]
__global__ __launch_bounds__(256) void match_kernel(const float* __restrict__ A, int na, const float* __restrict__ B, int nb, int tiles_per_split,
                                                    float* __restrict__ part_d, int* __restrict__ part_i) {
  __shared__ __attribute__((aligned(16))) float s_a[FPFH_DIM * MT_PITCH];
  __shared__ __attribute__((aligned(16))) float s_b[FPFH_DIM * MT_PITCH];
  __shared__ float s_na[MT], s_nb[MT];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int row0 = blockIdx.x * MT;
  load_tile(A, na, row0, s_a, s_na);
  float best_d[8];
  int best_i[8];
#pragma unroll
  for (int r = 0; r < 8; r++) {
    best_d[r] = __int_as_float(0x7f800000);
    best_i[r] = -1;
  }
  const int nt_tiles = (nb + MT - 1) / MT;
  const int t_begin = blockIdx.y * tiles_per_split, t_end = min(nt_tiles, t_begin + tiles_per_split);
  for (int t = t_begin; t < t_end; t++) {
    __syncthreads();  // the previous tile's readers are done (and, first trip, nothing)
    load_tile(B, nb, t * MT, s_b, s_nb);
    __syncthreads();
    float acc[8][8];
#pragma unroll
    for (int r = 0; r < 8; r++)
#pragma unroll
      for (int c = 0; c < 8; c++) acc[r][c] = 0.0f;
#pragma unroll 3
    for (int k = 0; k < FPFH_DIM; k++) {
      const float4 a0 = *reinterpret_cast<const float4*>(&s_a[k * MT_PITCH + ty * 4]);
      const float4 a1 = *reinterpret_cast<const float4*>(&s_a[k * MT_PITCH + 64 + ty * 4]);
      const float4 b0 = *reinterpret_cast<const float4*>(&s_b[k * MT_PITCH + tx * 4]);
      const float4 b1 = *reinterpret_cast<const float4*>(&s_b[k * MT_PITCH + 64 + tx * 4]);
      const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int r = 0; r < 8; r++)
#pragma unroll
        for (int c = 0; c < 8; c++) acc[r][c] = fmaf(a[r], b[c], acc[r][c]);
    }
    // a lane's columns ascend with c and with t: a strict < keeps the smaller index on a tie
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const float nr = s_na[(r >> 2) * 64 + ty * 4 + (r & 3)];
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const int lc = (c >> 2) * 64 + tx * 4 + (c & 3);
        const int col = t * MT + lc;
        const float d = fmaxf(fmaf(-2.0f, acc[r][c], nr + s_nb[lc]), 0.0f);
        if (col < nb && d < best_d[r]) {
          best_d[r] = d;
          best_i[r] = col;
        }
      }
    }
  }
  // the 16 lanes of a row: through LDS (s_b is free once every lane has left the loop), smaller index on a tie
  __syncthreads();
  float* s_rd = s_b;
  int* s_ri = reinterpret_cast<int*>(s_b + MT * 16);
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const int lr = (r >> 2) * 64 + ty * 4 + (r & 3);
    s_rd[lr * 16 + tx] = best_d[r];
    s_ri[lr * 16 + tx] = best_i[r];
  }
  __syncthreads();
  if (threadIdx.x < MT && row0 + (int)threadIdx.x < na) {
    float bd = __int_as_float(0x7f800000);
    int bi = -1;
    for (int x = 0; x < 16; x++) {
      const float d = s_rd[threadIdx.x * 16 + x];
      const int i = s_ri[threadIdx.x * 16 + x];
      if (i >= 0 && (bi < 0 || d < bd || (d == bd && i < bi))) {
        bd = d;
        bi = i;
      }
    }
    part_d[(size_t)blockIdx.y * na + row0 + threadIdx.x] = bd;
    part_i[(size_t)blockIdx.y * na + row0 + threadIdx.x] = bi;
  }
}
static_assert(2 * MT * 16 <= FPFH_DIM * MT_PITCH, "the row reduction fits the target tile");

// splits hold ascending index ranges: merged in order, a strict < keeps the smaller index on a tie
__global__ __launch_bounds__(256) void match_merge_kernel(int na, int splits, const float* __restrict__ part_d, const int* __restrict__ part_i,
                                                          float* __restrict__ out_d, int* __restrict__ out_i) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= na) return;
  float bd = __int_as_float(0x7f800000);
  int bi = -1;
  for (int s = 0; s < splits; s++) {
    const float d = part_d[(size_t)s * na + i];
    const int j = part_i[(size_t)s * na + i];
    if (j >= 0 && (bi < 0 || d < bd)) {
      bd = d;
      bi = j;
    }
  }
  out_d[i] = bd;
  out_i[i] = bi;
}

__global__ __launch_bounds__(256) void match_reciprocal_kernel(int na, int nb, const int* __restrict__ back, int* __restrict__ fwd) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= na) return;
  const int j = fwd[i];
  if (j < 0 || j >= nb || back[j] != i) fwd[i] = -1;
}

inline int bits_for_value(int v) {
  int b = 0;
  while (v > 0) {
    b++;
    v >>= 1;
  }
  return b;
}

// nearest row of B for every row of A, into device arrays out_d / out_i (na entries); nb >= 1, na >= 1
int enqueue_match(glim_amd_ctx* ctx, hipStream_t st, const float* A, int na, const float* B, int nb, float* part_d, int* part_i, int splits,
                  int tiles_per_split, float* out_d, int* out_i) {
  (void)ctx;
  const int a_tiles = (na + MT - 1) / MT;
  match_kernel<<<dim3(a_tiles, splits), 256, 0, st>>>(A, na, B, nb, tiles_per_split, part_d, part_i);
  match_merge_kernel<<<(na + 255) / 256, 256, 0, st>>>(na, splits, part_d, part_i, out_d, out_i);
  GA_HIP(hipGetLastError());
  return GLIM_AMD_OK;
}
// target splits of a direction: enough blocks for two per compute unit, never more than there are target tiles
inline void match_splits(const glim_amd_ctx* ctx, int na, int nb, int* splits, int* tiles_per_split) {
  const int a_tiles = (na + MT - 1) / MT, b_tiles = (nb + MT - 1) / MT;
  const int want = std::max(1, (2 * std::max(ctx->num_cus, 1) + a_tiles - 1) / a_tiles);
  const int s = std::max(1, std::min(want, b_tiles));
  *tiles_per_split = (b_tiles + s - 1) / s;
  *splits = (b_tiles + *tiles_per_split - 1) / *tiles_per_split;
}

// the device side of glim_amd_fpfh_match (fpfh.hpp)
int enqueue_match_both(glim_amd_ctx* ctx, hipStream_t st, const glim_amd_fpfh* target, const glim_amd_fpfh* source, uint32_t flags, MatchBuffers* b) {
  const int na = (int)source->n, nb = (int)target->n;
  const bool reciprocal = (flags & GLIM_AMD_FPFH_RECIPROCAL) != 0;
  int splits_f = 1, tps_f = 1, splits_b = 1, tps_b = 1;
  match_splits(ctx, na, nb, &splits_f, &tps_f);
  if (reciprocal) match_splits(ctx, nb, na, &splits_b, &tps_b);
  const size_t part = std::max((size_t)splits_f * na, reciprocal ? (size_t)splits_b * nb : (size_t)0);
  GA_HIP(pool_malloc(&b->part_d.p, part * sizeof(float)));
  GA_HIP(pool_malloc(&b->part_i.p, part * sizeof(int)));
  GA_HIP(pool_malloc(&b->fwd_d.p, (size_t)na * sizeof(float)));
  GA_HIP(pool_malloc(&b->fwd_i.p, (size_t)na * sizeof(int)));
  GA_TRY(enqueue_match(ctx, st, source->desc, na, target->desc, nb, b->part_d.as<float>(), b->part_i.as<int>(), splits_f, tps_f, b->fwd_d.as<float>(),
                       b->fwd_i.as<int>()));
  if (reciprocal) {
    GA_HIP(pool_malloc(&b->back_d.p, (size_t)nb * sizeof(float)));
    GA_HIP(pool_malloc(&b->back_i.p, (size_t)nb * sizeof(int)));
    GA_TRY(enqueue_match(ctx, st, target->desc, nb, source->desc, na, b->part_d.as<float>(), b->part_i.as<int>(), splits_b, tps_b, b->back_d.as<float>(),
                         b->back_i.as<int>()));
    match_reciprocal_kernel<<<(na + 255) / 256, 256, 0, st>>>(na, nb, b->back_i.as<int>(), b->fwd_i.as<int>());
    GA_HIP(hipGetLastError());
  }
  return GLIM_AMD_OK;
}

using FpfhPtr = std::unique_ptr<glim_amd_fpfh, int (*)(glim_amd_fpfh*)>;

// a descriptor object of `n` rows (storage for one when n = 0), its rows not initialised.  The caller holds ctx->mu and has set the device.
int new_fpfh(glim_amd_ctx* ctx, int64_t n, FpfhPtr* out) {
  FpfhPtr f(new glim_amd_fpfh(), glim_amd_fpfh_destroy);
  f->ctx = ctx;
  f->n = n;
  GA_HIP(pool_malloc(&f->desc, (size_t)std::max<int64_t>(n, 1) * FPFH_STRIDE * sizeof(float)));
  *out = std::move(f);
  return GLIM_AMD_OK;
}

}  // namespace fpfh_detail
}  // namespace glim_amd

extern "C" {

int glim_amd_fpfh_destroy(glim_amd_fpfh* f) {
  if (!f) return GLIM_AMD_OK;
  if (f->ctx) (void)hipSetDevice(f->ctx->device);
  if (f->desc) (void)glim_amd::pool_free(f->desc);
  delete f;
  return GLIM_AMD_OK;
}

int glim_amd_fpfh_size(const glim_amd_fpfh* f, int64_t* n) {
  if (!f || !n) return GLIM_AMD_ERR_INVALID;
  *n = f->n;
  return GLIM_AMD_OK;
}

int glim_amd_fpfh_estimate(const glim_amd_cloud* cloud, double search_radius, glim_amd_fpfh** out) {
  using namespace glim_amd;
  using namespace glim_amd::fpfh_detail;
  if (!cloud || !out) return GLIM_AMD_ERR_INVALID;
  *out = nullptr;
  if (!(search_radius > 0.0) || !std::isfinite(search_radius)) return GLIM_AMD_ERR_INVALID;
  if (!cloud->has_normals || !cloud->normals) return GLIM_AMD_ERR_STATE;
  if (cloud->n > (int64_t)(1 << 28)) return GLIM_AMD_ERR_INVALID;
  glim_amd_ctx* ctx = cloud->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  const int n = (int)cloud->n;
  FpfhPtr f(nullptr, glim_amd_fpfh_destroy);
  GA_TRY(new_fpfh(ctx, n, &f));
  const size_t nn = (size_t)std::max(n, 1);
  if (n == 0) {
    *out = f.release();
    return GLIM_AMD_OK;
  }
  DeviceTemp vkey, bb, ka, kb, va, vb, hist, counts, first, tiles, spts, snrm, scell, S;
  SyncOnExit in_flight(st);
  GA_HIP(hipMemsetAsync(f->desc, 0, nn * FPFH_STRIDE * sizeof(float), st));  // points without a cell (non-finite) keep an all-zero row
  GA_HIP(pool_malloc(&vkey.p, nn * sizeof(u64)));
  GA_HIP(pool_malloc(&bb.p, 6 * sizeof(int)));
  const int blocks = std::max(1, std::min((n + 2047) / 2048, 128));
  // cell edge: just above r (a neighbour is then never more than one cell away, whatever the rounding of the cell assignment), doubled until the
  // padded bounding box is a grid of at most MAX_CELLS cells
  double h = search_radius * 1.000001;
  int h_bb[6], nx = 0, ny = 0, nz = 0;
  for (;;) {
    init_bbox_kernel<<<1, 64, 0, st>>>(bb.as<int>());
    fp_key_kernel<<<blocks, 256, 0, st>>>(n, cloud->pts, 1.0 / h, vkey.as<u64>(), bb.as<int>());
    GA_HIP(hipGetLastError());
    GA_HIP(read_back_sync(ctx, st, h_bb, bb.p, sizeof(h_bb)));
    if (h_bb[0] > h_bb[3]) break;  // no point has a cell
    nx = h_bb[3] - h_bb[0] + 3, ny = h_bb[4] - h_bb[1] + 3, nz = h_bb[5] - h_bb[2] + 3;
    if ((double)nx * (double)ny * (double)nz <= (double)MAX_CELLS) break;
    h *= 2.0;
    if (!std::isfinite(h)) return GLIM_AMD_ERR_RANGE;
  }
  if (h_bb[0] > h_bb[3]) {
    GA_HIP(hipStreamSynchronize(st));
    in_flight.dismiss();
    *out = f.release();
    return GLIM_AMD_OK;
  }
  const int ncells = nx * ny * nz;
  const unsigned int T = (unsigned int)ncells + 1u;
  GA_HIP(pool_malloc(&ka.p, nn * sizeof(u64)));
  GA_HIP(pool_malloc(&kb.p, nn * sizeof(u64)));
  GA_HIP(pool_malloc(&va.p, nn * sizeof(u32)));
  GA_HIP(pool_malloc(&vb.p, nn * sizeof(u32)));
  GA_HIP(pool_malloc(&hist.p, radix_sort_scratch_bytes(n)));
  GA_HIP(pool_malloc(&counts.p, (size_t)T * sizeof(int)));
  GA_HIP(pool_malloc(&first.p, (size_t)T * sizeof(int)));
  GA_HIP(pool_malloc(&tiles.p, scan_scratch_ints(T) * sizeof(int)));
  GA_HIP(pool_malloc(&spts.p, nn * sizeof(float4)));
  GA_HIP(pool_malloc(&snrm.p, nn * sizeof(float4)));
  GA_HIP(pool_malloc(&scell.p, nn * sizeof(int)));
  GA_HIP(hipMemsetAsync(counts.p, 0, (size_t)T * sizeof(int), st));
  fp_cell_kernel<<<(n + 255) / 256, 256, 0, st>>>(n, vkey.as<u64>(), h_bb[0] - 1, h_bb[1] - 1, h_bb[2] - 1, nx, ny, ncells, ka.as<u64>(), counts.as<int>());
  u64* ks = nullptr;
  u32* vs = nullptr;
  GA_HIP(radix_sort_pairs(st, n, bits_for_value(ncells), ka.as<u64>(), va.as<u32>(), kb.as<u64>(), vb.as<u32>(), true, hist.as<int>(), &ks, &vs));
  GA_HIP(exclusive_scan_int(st, counts.as<int>(), T, tiles.as<int>(), first.as<int>()));
  fp_gather_kernel<<<(n + 255) / 256, 256, 0, st>>>(n, ks, vs, cloud->pts, cloud->normals, spts.as<float4>(), snrm.as<float4>(), scell.as<int>());
  GA_HIP(hipGetLastError());
  int nvalid = 0;  // = first[ncells]
  GA_HIP(read_back_sync(ctx, st, &nvalid, first.as<int>() + ncells, sizeof(int)));
  if (nvalid < 0 || nvalid > n) return GLIM_AMD_ERR_STATE;
  if (nvalid > 0) {
    GA_HIP(pool_malloc(&S.p, (size_t)nvalid * SPFH_STRIDE * sizeof(double)));
    Grid g;
    g.spts = spts.as<float4>();
    g.snrm = snrm.as<float4>();
    g.scell = scell.as<int>();
    g.first = first.as<int>();
    g.nx = nx;
    g.ny = ny;
    g.nvalid = nvalid;
    g.r2 = search_radius * search_radius;
    spfh_kernel<<<nvalid, 64, 0, st>>>(g, S.as<double>());
    fpfh_kernel<<<nvalid, 64, 0, st>>>(g, S.as<double>(), f->desc);
    GA_HIP(hipGetLastError());
  }
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  *out = f.release();
  return GLIM_AMD_OK;
}

int glim_amd_fpfh_create(glim_amd_ctx* ctx, int64_t n, const float* descriptors33, glim_amd_fpfh** out) {
  using namespace glim_amd;
  using namespace glim_amd::fpfh_detail;
  if (!ctx || !out) return GLIM_AMD_ERR_INVALID;
  *out = nullptr;
  if (n < 0 || n > (int64_t)(1 << 28) || (n > 0 && !descriptors33)) return GLIM_AMD_ERR_INVALID;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  FpfhPtr f(nullptr, glim_amd_fpfh_destroy);
  GA_TRY(new_fpfh(ctx, n, &f));
  if (n > 0) {
    // the device row: 33 bins | the matcher's FMA chain of the row with itself, as fpfh_kernel stores it | 0 0
    std::vector<float> rows((size_t)n * FPFH_STRIDE, 0.0f);
    for (int64_t i = 0; i < n; i++) {
      float* row = &rows[(size_t)i * FPFH_STRIDE];
      float nn2 = 0.0f;
      for (int b = 0; b < FPFH_DIM; b++) {
        row[b] = descriptors33[(size_t)i * FPFH_DIM + b];
        nn2 = fmaf(row[b], row[b], nn2);
      }
      row[FPFH_DIM] = nn2;
    }
    GA_HIP(hipMemcpyAsync(f->desc, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream()));
    GA_HIP(hipStreamSynchronize(ctx->stream()));
  }
  *out = f.release();
  return GLIM_AMD_OK;
}

int glim_amd_fpfh_download(const glim_amd_fpfh* f, float* descriptors33) {
  using namespace glim_amd;
  using namespace glim_amd::fpfh_detail;
  if (!f || !descriptors33) return GLIM_AMD_ERR_INVALID;
  if (f->n == 0) return GLIM_AMD_OK;
  glim_amd_ctx* ctx = f->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  GA_HIP(hipMemcpy2DAsync(descriptors33, FPFH_DIM * sizeof(float), f->desc, FPFH_STRIDE * sizeof(float), FPFH_DIM * sizeof(float), (size_t)f->n,
                          hipMemcpyDeviceToHost, ctx->stream()));
  GA_HIP(hipStreamSynchronize(ctx->stream()));
  return GLIM_AMD_OK;
}

int glim_amd_fpfh_match(const glim_amd_fpfh* target, const glim_amd_fpfh* source, uint32_t flags, int32_t* nearest, float* sqdist) {
  using namespace glim_amd;
  using namespace glim_amd::fpfh_detail;
  if (!target || !source) return GLIM_AMD_ERR_INVALID;
  if ((glim_amd_ctx*)target->ctx != (glim_amd_ctx*)source->ctx) return GLIM_AMD_ERR_INVALID;
  if (flags & ~(uint32_t)GLIM_AMD_FPFH_RECIPROCAL) return GLIM_AMD_ERR_INVALID;
  const int na = (int)source->n, nb = (int)target->n;
  if (na == 0) return GLIM_AMD_OK;
  if (nb == 0) {
    for (int i = 0; i < na; i++) {
      if (nearest) nearest[i] = -1;
      if (sqdist) sqdist[i] = INFINITY;
    }
    return GLIM_AMD_OK;
  }
  glim_amd_ctx* ctx = source->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  MatchBuffers m;
  SyncOnExit in_flight(st);
  GA_TRY(enqueue_match_both(ctx, st, target, source, flags, &m));
  if (nearest) GA_HIP(hipMemcpyAsync(nearest, m.fwd_i.p, (size_t)na * sizeof(int), hipMemcpyDeviceToHost, st));
  if (sqdist) GA_HIP(hipMemcpyAsync(sqdist, m.fwd_d.p, (size_t)na * sizeof(float), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  return GLIM_AMD_OK;
}

}  // extern "C"
