// graph_solve.hpp -- the solve of the global-graph optimisation (include/glim_amd.h "Global-graph optimisation"): the Cholesky rule of
// bundle_lm_step.hpp ("solve"), walked by block columns so that a system of 6 * 256 rows is factorised by ordinary launches over device memory.
// It is NOT a second rule.  Every entry of L, of y and of delta goes through the sequence of FP64 operations bundle_lm::solve gives it:
//
//   L[i][j] = (A[i][j] - sum_{k<j} L[i][k] L[j][k]) / L[j][j]     the subtractions one at a time, k ascending; the pivot is the square root
//   delta[k] = s[k] / L[k][k], then s[i] -= L[k][i] delta[k]      for i < k, k descending from n - 1
//
// Only WHO performs an entry's subtractions, and when, differs.  For the block column J = [j0, j1) of width `tile`, in ascending order:
//   panel update   entry (i, j), j in the block, i >= j, row n (-b) included: the subtractions k = 0 .. j0 - 1 (update_entry)
//   panel factor   the block's own diagonal tile, column by column: the subtractions k = j0 .. j - 1, the pivot, the division (tile_entry,
//                  pivot); then every row below the tile, for each column of the block in turn (row_entry)
// and for the block columns in descending order:
//   back           the tile's own delta from the tile's s (back_tile), then s[i] of every row above it (back_row)
// A pivot that is not > 0 or not finite is a failed solve: it is left in place, the later columns are computed and never used, delta is +0.0.
// The FINISHED diagonal tiles are not written over the unfinished ones: every workgroup of a panel factor reads the unfinished tile, so the one
// that writes the finished tile puts it into a side area behind the matrix (side_tile), where nothing of the same launch reads; the back
// kernels read it there.  No result depends on which workgroup of a launch runs first.
//
// The working matrix is COLUMN-major with a padded leading dimension: entry (i, k) at W[k * ld + i], i = 0 .. n (row n carries -b and then y).
// The rows of a column step are neighbours in memory and L[j][k] is one address for all of them.  The layout is not part of the rule.
// factor_blocked() and back_blocked() below are the launch order on the host: tests/cpp/test_graph_solve.cpp compares them with bundle_lm::solve byte for byte, and
// graph_solve.hip runs the same item functions, one owner per entry.  Plain C++ apart from the host/device macro.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GLIM_AMD_GS_HD __host__ __device__
#else
#define GLIM_AMD_GS_HD
#endif

namespace glim_amd {
namespace graph_solve {

constexpr int MAX_DIM = 6 * 256;  // GLIM_AMD_GRAPH_MAX_POSES poses
constexpr int MAX_TILE = 64;      // a tile of MAX_TILE x MAX_TILE doubles is 32 KiB of LDS
// the width the device code is built with: 16, 32 or 64
#ifndef GLIM_AMD_GRAPH_TILE
#define GLIM_AMD_GRAPH_TILE 64
#endif
constexpr int TILE = GLIM_AMD_GRAPH_TILE;
static_assert(TILE == 16 || TILE == 32 || TILE == 64, "the tile widths");

GLIM_AMD_GS_HD inline bool tile_ok(int tile) { return tile == 16 || tile == 32 || tile == 64; }
// the leading dimension: n + 1 rows, rounded up to a 64-byte line
GLIM_AMD_GS_HD inline int leading(int n) { return (n + 1 + 7) & ~7; }
// the matrix, then one MAX_TILE x MAX_TILE side tile (column-major, stride MAX_TILE) per block column: room for the narrowest width
GLIM_AMD_GS_HD inline size_t matrix_doubles(int n) {
  const size_t cols = (size_t)(n > 0 ? n : 1);
  return (size_t)leading(n) * cols + ((cols + 15) / 16) * (size_t)(MAX_TILE * MAX_TILE);
}
// the finished diagonal tile of block column J
GLIM_AMD_GS_HD inline double* side_tile(double* W, int n, int J) { return W + (size_t)leading(n) * (size_t)n + (size_t)J * (MAX_TILE * MAX_TILE); }
GLIM_AMD_GS_HD inline const double* side_tile(const double* W, int n, int J) { return side_tile(const_cast<double*>(W), n, J); }
// entry (i, j) of the finished L (i < n, j <= i) or of y (i == n), wherever it lives
GLIM_AMD_GS_HD inline double factor_entry(const double* W, int n, int tile, int i, int j) {
  const int J = j / tile;
  if (i < n && i / tile == J) return side_tile(W, n, J)[(j - J * tile) * MAX_TILE + (i - J * tile)];
  return W[(size_t)j * leading(n) + i];
}
GLIM_AMD_GS_HD inline bool finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // false for NaN

// panel update: entry (i, j) of W after the subtractions k = 0 .. j0 - 1
GLIM_AMD_GS_HD inline double update_entry(const double* W, int ld, int i, int j, int j0) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double v = W[(size_t)j * ld + i];
#if defined(__clang__)
#pragma unroll 8
#endif
  for (int k = 0; k < j0; k++) v -= W[(size_t)k * ld + i] * W[(size_t)k * ld + j];
  return v;
}

// the pivot from a diagonal entry that has had all its subtractions: the square root, or -1.0 (a failed solve)
GLIM_AMD_GS_HD inline double pivot(double d) {
  if (!(d > 0.0) || !finite(d)) return -1.0;
  return sqrt(d);
}

// the diagonal tile T (column-major, stride ts, local indices): entry (i, c), i >= c, after the subtractions of the tile's columns k < c.
// The caller takes the pivot of (c, c) and divides the entries below it
GLIM_AMD_GS_HD inline double tile_entry(const double* T, int ts, int i, int c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double v = T[c * ts + i];
  for (int k = 0; k < c; k++) v -= T[k * ts + i] * T[k * ts + c];
  return v;
}

// a row i below the tile: entry (i, j0 + c) finished.  The row's entries of the block's earlier columns are read from W, where its owner has
// put them; row j0 + c of L comes from the finished tile
GLIM_AMD_GS_HD inline double row_entry(const double* W, int ld, int i, int j0, const double* T, int ts, int c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double v = W[(size_t)(j0 + c) * ld + i];
  for (int k = 0; k < c; k++) v -= W[(size_t)(j0 + k) * ld + i] * T[k * ts + c];
  return v / T[c * ts + c];
}

// back substitution inside the block column [k0, k1), local indices: s holds the tile's right-hand sides, which have had the subtractions of
// every k >= k1; T is the tile of L.  Step k, descending: the tile's delta (back_delta), then one subtraction for every row above (back_sub)
GLIM_AMD_GS_HD inline double back_delta(const double* T, int ts, int k, double s_k) { return s_k / T[k * ts + k]; }
GLIM_AMD_GS_HD inline double back_sub(const double* T, int ts, int i, int k, double s_i, double d_k) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return s_i - T[i * ts + k] * d_k;
}
GLIM_AMD_GS_HD inline void back_tile(const double* T, int ts, int w, double* s, double* d) {
  for (int k = w - 1; k >= 0; k--) {
    d[k] = back_delta(T, ts, k, s[k]);
    for (int i = 0; i < k; i++) s[i] = back_sub(T, ts, i, k, s[i], d[k]);
  }
}

// a row i above the block column [k0, k1): s[i] after the subtractions k = k1 - 1 .. k0, with the tile's delta d (local indices)
GLIM_AMD_GS_HD inline double back_row(const double* W, int ld, int n, int i, int k0, int k1, const double* d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double v = W[(size_t)i * ld + n];
  for (int k = k1 - 1; k >= k0; k--) v -= W[(size_t)i * ld + k] * d[k - k0];
  return v;
}

// The launch order on the host, in its two halves.  W: the loaded matrix (H + lambda I, -b), column-major with ld = leading(n); after
// factor_blocked L and y are there (factor_entry) (false: a pivot failed); back_blocked then gives delta (+0.0 after a failed pivot) and leaves in row n
// what the device leaves there: s[i] with the subtractions of the block columns after i's own
inline bool factor_blocked(double* W, int n, int tile) {
  const int ld = leading(n);
  bool fail = false;
  double T[MAX_TILE * MAX_TILE];
  for (int j0 = 0; j0 < n; j0 += tile) {
    const int j1 = j0 + tile < n ? j0 + tile : n, w = j1 - j0;
    if (j0 > 0)  // panel update: one owner per entry, any order
      for (int j = j0; j < j1; j++)
        for (int i = j; i <= n; i++) W[(size_t)j * ld + i] = update_entry(W, ld, i, j, j0);
    // panel factor: a workgroup's copy of the tile, finished column by column
    for (int c = 0; c < w; c++)
      for (int i = c; i < w; i++) T[c * MAX_TILE + i] = W[(size_t)(j0 + c) * ld + j0 + i];
    for (int c = 0; c < w; c++) {
      const double p = pivot(tile_entry(T, MAX_TILE, c, c));
      if (p > 0.0) T[c * MAX_TILE + c] = p;
      else fail = true;
      for (int i = c + 1; i < w; i++) T[c * MAX_TILE + i] = tile_entry(T, MAX_TILE, i, c) / T[c * MAX_TILE + c];
    }
    double* D = side_tile(W, n, j0 / tile);  // (workgroup 0)
    for (int c = 0; c < w; c++)
      for (int i = c; i < w; i++) D[c * MAX_TILE + i] = T[c * MAX_TILE + i];
    for (int i = j1; i <= n; i++)  // the rows below the tile, a thread each
      for (int c = 0; c < w; c++) W[(size_t)(j0 + c) * ld + i] = row_entry(W, ld, i, j0, T, MAX_TILE, c);
  }
  return !fail;
}

inline void back_blocked(double* W, int n, int tile, bool fail, double* delta) {
  const int ld = leading(n);
  double s[MAX_TILE], d[MAX_TILE];
  for (int k1 = n; k1 > 0;) {
    const int k0 = ((k1 - 1) / tile) * tile, w = k1 - k0;
    const double* T = side_tile(W, n, k0 / tile);
    for (int c = 0; c < w; c++) s[c] = W[(size_t)(k0 + c) * ld + n];
    back_tile(T, MAX_TILE, w, s, d);
    for (int i = 0; i < k0; i++) W[(size_t)i * ld + n] = back_row(W, ld, n, i, k0, k1, d);
    for (int c = 0; c < w; c++) delta[k0 + c] = fail ? 0.0 : d[c];
    k1 = k0;
  }
}

inline bool solve_blocked(double* W, int n, int tile, double* delta) {
  const bool ok = factor_blocked(W, n, tile);
  back_blocked(W, n, tile, !ok, delta);
  return ok;
}

}  // namespace graph_solve

#if defined(__HIPCC__)
// graph_solve.hip: the launches of one solve on `st`.  W: matrix_doubles(n) doubles holding the loaded matrix; delta: n; fail: one word, set
// to 1 by a failed pivot and to 0 otherwise.  Every kernel returns at once while *status is not 0 (device memory, lm::RUNNING is 0)
hipError_t graph_solve_enqueue(hipStream_t st, double* W, int n, double* delta, int* fail, const int* status);
#endif

}  // namespace glim_amd
