// graph_solve.hip -- the solve of the global-graph optimisation on gfx950 (include/glim_amd.h "Global-graph optimisation"): the blocked,
// left-looking Cholesky factorisation and the back substitution of graph_solve.hpp over a working matrix in device memory, as ordinary
// launches on one stream.  Per block column, ascending: a panel update (a thread per entry of the panel, its subtractions k < j0), then a
// panel factor (every workgroup finishes the block's diagonal tile in LDS, redundantly and identically, then its own rows below the tile;
// workgroup 0 writes the finished tile into the side area behind the matrix, never over the unfinished tile the others may still load).  Per block column, descending: one back kernel (every workgroup solves the tile's delta in LDS, then takes
// that column's subtractions for its own rows above).  No kernel waits for another workgroup: a kernel boundary is the only ordering.  No
// kernel declares more than 33 KiB of LDS.  Every value comes from an item function of graph_solve.hpp, one owner per entry.
//
// The rule the solve belongs to (records, terms, assembly, decision, retraction) is the bundle's and is run by bundle_align.hip; this unit
// knows the matrix and nothing else.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "graph_solve.hpp"

using namespace glim_amd;
using namespace glim_amd::graph_solve;

namespace {

constexpr int THREADS = 256;
static_assert(TILE <= THREADS && TILE * TILE * sizeof(double) + 2 * TILE * sizeof(double) <= 64 * 1024, "a tile and its two vectors in LDS");

// entry (i, j) of the panel [j0, j1), i >= j: blockIdx.y is the column, the threads run along the rows from j0
__global__ __launch_bounds__(THREADS) void graph_panel_update_kernel(double* W, int n, int ld, int j0, int j1, const int* __restrict__ status) {
  if (*status != 0) return;  // the same for every thread
  const int j = j0 + (int)blockIdx.y, i = j0 + (int)(blockIdx.x * THREADS + threadIdx.x);
  if (j >= j1 || i < j || i > n) return;
  W[(size_t)j * ld + i] = update_entry(W, ld, i, j, j0);  // reads the columns before j0 and its own entry
}

__global__ __launch_bounds__(THREADS) void graph_panel_factor_kernel(double* W, int n, int ld, int j0, int j1, int* fail, const int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ double T[TILE * TILE];
  if (*status != 0) return;
  const int w = j1 - j0, t = threadIdx.x;
  for (int u = t; u < w * w; u += THREADS) {
    const int c = u / w, i = u - c * w;
    if (i >= c) T[c * TILE + i] = W[(size_t)(j0 + c) * ld + j0 + i];
  }
  __syncthreads();
  for (int c = 0; c < w; c++) {  // thread i takes entry (i, c) of the tile; a failed pivot stays in place
    double v = 0.0;
    if (t >= c && t < w) v = tile_entry(T, TILE, t, c);
    if (t == c) {
      const double p = pivot(v);
      if (p > 0.0) T[c * TILE + c] = p;
      else if (blockIdx.x == 0) *fail = 1;
    }
    __syncthreads();
    if (t > c && t < w) T[c * TILE + t] = v / T[c * TILE + c];
    __syncthreads();
  }
  if (blockIdx.x == 0) {  // the finished tile goes beside the matrix: the unfinished one is what the other workgroups of this launch read
    double* D = side_tile(W, n, j0 / TILE);
    for (int u = t; u < w * w; u += THREADS) {
      const int c = u / w, i = u - c * w;
      if (i >= c) D[c * MAX_TILE + i] = T[c * TILE + i];
    }
  }
  const int i = j1 + (int)(blockIdx.x * THREADS) + t;  // a row below the tile, -b's row among them: nobody else touches it in this launch
  if (i <= n)
    for (int c = 0; c < w; c++) W[(size_t)(j0 + c) * ld + i] = row_entry(W, ld, i, j0, T, TILE, c);
}

__global__ __launch_bounds__(THREADS) void graph_back_kernel(double* W, int n, int ld, int k0, int k1, double* __restrict__ delta, const int* __restrict__ fail,
                                                             const int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ double T[TILE * TILE];
  __shared__ double s[TILE], d[TILE];
  if (*status != 0) return;
  const int w = k1 - k0, t = threadIdx.x;
  const double* D = side_tile(W, n, k0 / TILE);  // the finished tile, written by an earlier launch
  for (int u = t; u < w * w; u += THREADS) {
    const int c = u / w, i = u - c * w;
    if (i >= c) T[c * TILE + i] = D[c * MAX_TILE + i];
  }
  if (t < w) s[t] = W[(size_t)(k0 + t) * ld + n];
  __syncthreads();
  for (int k = w - 1; k >= 0; k--) {  // back_tile, thread i keeping s[i]
    if (t == k) d[k] = back_delta(T, TILE, k, s[k]);
    __syncthreads();
    if (t < k) s[t] = back_sub(T, TILE, t, k, s[t], d[k]);
  }
  if (blockIdx.x == 0 && t < w) delta[k0 + t] = *fail ? 0.0 : d[t];
  const int i = (int)(blockIdx.x * THREADS) + t;  // a row above the tile
  if (i < k0) W[(size_t)i * ld + n] = back_row(W, ld, n, i, k0, k1, d);
}

}  // namespace

namespace glim_amd {

hipError_t graph_solve_enqueue(hipStream_t st, double* W, int n, double* delta, int* fail, const int* status) {
  if (n < 1 || n > MAX_DIM) return hipErrorInvalidValue;
  const int ld = leading(n);
  hipError_t e = hipMemsetAsync(fail, 0, sizeof(int), st);
  if (e != hipSuccess) return e;
  for (int j0 = 0; j0 < n; j0 += TILE) {
    const int j1 = std::min(n, j0 + TILE);
    if (j0 > 0) graph_panel_update_kernel<<<dim3((n + 1 - j0 + THREADS - 1) / THREADS, j1 - j0), THREADS, 0, st>>>(W, n, ld, j0, j1, status);
    graph_panel_factor_kernel<<<(n + 1 - j1 + THREADS - 1) / THREADS, THREADS, 0, st>>>(W, n, ld, j0, j1, fail, status);
  }
  for (int k1 = n; k1 > 0;) {
    const int k0 = ((k1 - 1) / TILE) * TILE;
    graph_back_kernel<<<std::max(1, (k0 + THREADS - 1) / THREADS), THREADS, 0, st>>>(W, n, ld, k0, k1, delta, fail, status);
    k1 = k0;
  }
  return hipGetLastError();
}

}  // namespace glim_amd
