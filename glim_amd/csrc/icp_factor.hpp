// icp_factor.hpp -- the per-point algebra of the ICP factors (gtsam_points::IntegratedICPFactor, IntegratedPointToPlaneICPFactor; semantics in
// include/glim_amd.h "ICP factors"): gicp_point's arithmetic with another metric.  The correspondence, the residual, the 28 accumulators and
// their layout are the GICP factor's (gicp_factor.hpp), so the block epilogue, the ordered sum and the compact record are called unchanged by
// the kernels that run this (gicp.hip's icp_kernel, gicp_align.hip's ICP instantiation of the align kernel).
//   point-to-point  the source-frame metric A is the identity: folded away here, never multiplied through
//   point-to-plane  the target-frame metric is diag(n_x^2, n_y^2, n_z^2) (upstream weights residual and Jacobian ELEMENTWISE by the target
//                   normal), so A = R^T diag(n^2) R, formed in FP32 like gicp_point's S
#pragma once
#include "gicp_factor.hpp"

namespace {

// adds the terms of one matched point to the 28 accumulators.  p: the source point, b: its target point, nrm: the target normal (PLANE only),
// q = T p in FP64
template <bool LINEARIZE, bool PLANE>
__device__ __forceinline__ void icp_point(float (&acc)[NACC], const Rot32& R, const float4 p, const float4 b, const float4 nrm, double qx, double qy, double qz) {
  // residual b_j - q: formed in FP64 (|r| <= the correspondence radius), then FP32
  const float rx = (float)((double)b.x - qx), ry = (float)((double)b.y - qy), rz = (float)((double)b.z - qz);
  const float rsx = R.r00 * rx + R.r10 * ry + R.r20 * rz;
  const float rsy = R.r01 * rx + R.r11 * ry + R.r21 * rz;
  const float rsz = R.r02 * rx + R.r12 * ry + R.r22 * rz;
  const float x = p.x, y = p.y, z = p.z;
  if (!PLANE) {
    // A = I: u = r_s, g = -hat(p)
    acc[27] += rsx * rsx + rsy * rsy + rsz * rsz;
    if (LINEARIZE) {
      acc[0] += y * y + z * z;
      acc[1] -= x * y;
      acc[2] -= x * z;
      acc[3] += z * z + x * x;
      acc[4] -= y * z;
      acc[5] += x * x + y * y;
      acc[7] -= z; acc[8] += y;
      acc[9] += z; acc[11] -= x;
      acc[12] -= y; acc[13] += x;
      acc[15] += 1.0f; acc[18] += 1.0f; acc[20] += 1.0f;
      acc[21] += rsy * z - rsz * y;
      acc[22] += rsz * x - rsx * z;
      acc[23] += rsx * y - rsy * x;
      acc[24] += rsx; acc[25] += rsy; acc[26] += rsz;
    }
    return;
  }
  // A = R^T diag(n^2) R (source frame, symmetric)
  const float w0 = nrm.x * nrm.x, w1 = nrm.y * nrm.y, w2 = nrm.z * nrm.z;
  const float m00 = w0 * R.r00, m01 = w0 * R.r01, m02 = w0 * R.r02;
  const float m10 = w1 * R.r10, m11 = w1 * R.r11, m12 = w1 * R.r12;
  const float m20 = w2 * R.r20, m21 = w2 * R.r21, m22 = w2 * R.r22;
  const float A00 = R.r00 * m00 + R.r10 * m10 + R.r20 * m20;
  const float A01 = R.r00 * m01 + R.r10 * m11 + R.r20 * m21;
  const float A02 = R.r00 * m02 + R.r10 * m12 + R.r20 * m22;
  const float A11 = R.r01 * m01 + R.r11 * m11 + R.r21 * m21;
  const float A12 = R.r01 * m02 + R.r11 * m12 + R.r21 * m22;
  const float A22 = R.r02 * m02 + R.r12 * m12 + R.r22 * m22;
  const float ux = A00 * rsx + A01 * rsy + A02 * rsz;
  const float uy = A01 * rsx + A11 * rsy + A12 * rsz;
  const float uz = A02 * rsx + A12 * rsy + A22 * rsz;
  acc[27] += rsx * ux + rsy * uy + rsz * uz;
  if (LINEARIZE) {
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
}

// the target normal of position j of the sorted order, through the original index the position keeps in w
__device__ __forceinline__ float4 icp_normal(const float4* __restrict__ normals, const float4 b) { return normals[__float_as_int(b.w)]; }

}  // namespace
