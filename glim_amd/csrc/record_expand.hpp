// record_expand.hpp -- host side of a synchronous linearisation's last step: the compact record of a factor becomes the dense blocks the caller
// takes (glim_amd_linearized6).  Plain C++ (no HIP): the library's glim_amd_expand_compact / glim_amd_factor_set_linearize and the stand-alone
// program of tests/test_record_expand.py include it.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/glim_amd.h"

// the bundle optimisation's decide kernel (bundle_lm_step.hpp) runs the same statements on the device; on the host nothing changes
#if defined(__HIPCC__)
#define GLIM_AMD_EXPAND_HD __host__ __device__
#else
#define GLIM_AMD_EXPAND_HD
#endif

namespace glim_amd {

// The adjoint a binary factor's target blocks go through depends on the pose alone:
//   Ad = Adjoint(delta^-1) = [R^T 0; -R^T hat(t) R^T]   ([omega; v] ordering)
// Only its two distinct non-zero blocks are kept: adj[0..8] = R^T, adj[9..17] = -R^T hat(t) (row-major 3x3 each).  The synchronous call
// computes them while the device works on the request (vgicp.hip glim_amd_factor_set_linearize).
constexpr int ADJOINT_DOUBLES = 18;
GLIM_AMD_EXPAND_HD inline void binary_adjoint(const double* T, double* adj) {
#pragma clang fp contract(off)
  double* Rt = adj;
  for (int r = 0; r < 3; r++)
    for (int cc = 0; cc < 3; cc++) Rt[3 * r + cc] = T[4 * cc + r];
  const double t[3] = {T[3], T[7], T[11]};
  const double Ht[9] = {0.0, -t[2], t[1], t[2], 0.0, -t[0], -t[1], t[0], 0.0};  // hat(t)
  for (int r = 0; r < 3; r++)
    for (int cc = 0; cc < 3; cc++) {
      double s = 0.0;
      for (int m = 0; m < 3; m++) s += Rt[3 * r + m] * Ht[3 * m + cc];
      adj[9 + 3 * r + cc] = -s;
    }
}

// compact record c (COMPACT doubles) -> *out.  adj: binary_adjoint of the factor's pose, or null for a unary factor (target blocks stay zero).
// The products H_tt = Ad^T H_ss Ad, H_ts = -Ad^T H_ss, b_t = -Ad^T b_s leave out the terms that multiply the zero block of Ad; the terms that
// remain are added in the order of the full six-term sums, starting from +0.0 as those do.  A left-out term is +-0 for every finite record, and
// adding it changes no partial sum (a sum that starts at +0.0 is never -0.0), so the result has the bits of the full products.
GLIM_AMD_EXPAND_HD inline void expand_compact_record(const double* c, const double* adj, glim_amd_linearized6* out) {
#pragma clang fp contract(off)
  __builtin_memset(out, 0, sizeof(*out));  // (the builtin: memset itself is a host function to a device compiler)
  out->num_inliers = (int64_t)llround(c[0]);
  out->error = c[1];
  int k = 2;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++) {
      out->H_ss[6 * i + j] = c[k];
      out->H_ss[6 * j + i] = c[k];
      k++;
    }
  for (int i = 0; i < 6; i++) out->b_s[i] = c[k++];
  if (!adj) return;
  // Ad by blocks: rows 0..2 are [Rt 0], rows 3..5 are [L Rt]
  const double *Rt = adj, *L = adj + 9;
  const double *H = out->H_ss, *bs = out->b_s;
  double AtH[36];  // Ad^T H_ss
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 6; j++) {
      double s = 0.0;
      for (int m = 0; m < 3; m++) s += Rt[3 * m + i] * H[6 * m + j];
      for (int m = 0; m < 3; m++) s += L[3 * m + i] * H[6 * (m + 3) + j];
      AtH[6 * i + j] = s;
      double u = 0.0;  // (column i + 3 of Ad is zero in rows 0..2)
      for (int m = 0; m < 3; m++) u += Rt[3 * m + i] * H[6 * (m + 3) + j];
      AtH[6 * (i + 3) + j] = u;
    }
  for (int i = 0; i < 6; i++) {
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
      for (int m = 0; m < 3; m++) s += AtH[6 * i + m] * Rt[3 * m + j];
      for (int m = 0; m < 3; m++) s += AtH[6 * i + m + 3] * L[3 * m + j];
      out->H_tt[6 * i + j] = s;
      double u = 0.0;
      for (int m = 0; m < 3; m++) u += AtH[6 * i + m + 3] * Rt[3 * m + j];
      out->H_tt[6 * i + j + 3] = u;
    }
    for (int j = 0; j < 6; j++) out->H_ts[6 * i + j] = -AtH[6 * i + j];
  }
  for (int i = 0; i < 3; i++) {
    double s = 0.0;
    for (int m = 0; m < 3; m++) s += Rt[3 * m + i] * bs[m];
    for (int m = 0; m < 3; m++) s += L[3 * m + i] * bs[m + 3];
    out->b_t[i] = -s;
    double u = 0.0;
    for (int m = 0; m < 3; m++) u += Rt[3 * m + i] * bs[m + 3];
    out->b_t[i + 3] = -u;
  }
  // symmetrise H_tt against rounding
  for (int i = 0; i < 6; i++)
    for (int j = i + 1; j < 6; j++) {
      const double s = 0.5 * (out->H_tt[6 * i + j] + out->H_tt[6 * j + i]);
      out->H_tt[6 * i + j] = out->H_tt[6 * j + i] = s;
    }
}

}  // namespace glim_amd
