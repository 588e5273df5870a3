// vgicp_batch.hpp -- what the VGICP fine registration (vgicp_align.hip, include/glim_amd.h "VGICP fine registration") asks of vgicp.hip: the
// evaluation of B independent VGICP factors at poses that live on the device, gated by a status word per factor.
//
//   the plan    a TRANSIENT plan over the B (voxel map, cloud) pairs, built by plan_build -- the rule a caller's factor set of the same pairs in the
//               same order gets: the same points per thread, the same block map, the same rows.  It is never adopted by a set, never parked in the
//               context's cache and never served by a resident session; the batch's destructor gives its buffers back.
//   a round     vgicp_batch_round: the row kernel over the plane-form segment and over the general segment (compute_row, the body vgicp_kernel
//               runs, behind the status check) and one finalising block per factor (finalize_factor, the body finalize_kernel runs).  The record of
//               factor f lands at records() + 29 f, evaluated at the pose poses() + 12 f: bit for bit what glim_amd_factor_set_linearize returns
//               for the same set at that pose.  A factor whose status word is not 0 costs one load per block: its rows and its record stay.
// The caller holds the context's mutex while the batch lives, has made the context's device current, and has waited for the stream before the
// batch is destroyed.
#pragma once
#include "internal.hpp"

namespace glim_amd {

struct VgicpBatch {
  glim_amd_factor_set set;     // the pairs, and the stream everything is enqueued on (the context's first)
  FactorPlan* plan = nullptr;  // owned
  VgicpBatch() = default;
  VgicpBatch(const VgicpBatch&) = delete;
  VgicpBatch& operator=(const VgicpBatch&) = delete;
  ~VgicpBatch();
  hipStream_t stream() const { return set.stream; }
  double* poses() const { return plan->d_poses; }            // device: 12 doubles per factor, written by whoever decides the next candidate
  const double* records() const { return plan->d_compact; }  // device: COMPACT doubles per factor
  void seen_complete() { plan->maybe_busy = false; }         // the caller has waited for the stream: the destructor need not
};

// GLIM_AMD_OK, or what plan_build returns; nothing is launched beyond the lazily built caches of the clouds and maps (factor streams, plane view)
int vgicp_batch_open(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, uint32_t flags, int count, VgicpBatch* b);
// status of factor f: status[f * stride] (device memory, 0 = evaluate)
int vgicp_batch_round(VgicpBatch* b, const int* status, int stride);

}  // namespace glim_amd
