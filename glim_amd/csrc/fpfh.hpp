// fpfh.hpp -- what fpfh.hip gives the global-registration entries (registration_host.hpp, for ransac.hip and gnc.hip): the descriptor object and
// the device side of the matcher.  Both are defined in fpfh.hip.
#pragma once
#include <cstdint>

#include "internal.hpp"

struct glim_amd_fpfh {
  CtxRef ctx;
  int64_t n = 0;
  float* desc = nullptr;  // n x FPFH_STRIDE: 33 bins | squared norm of the row (the matcher's FMA chain) | 0 0
};

namespace glim_amd {
namespace fpfh_detail {

// the device side of glim_amd_fpfh_match: nearest target row of every source row into b->fwd_i / b->fwd_d, the reciprocal pass when asked for.
// Both sets are non-empty; the caller holds ctx->mu, synchronises `st` and keeps `b` until then.
struct MatchBuffers {
  DeviceTemp part_d, part_i, fwd_d, fwd_i, back_d, back_i;
};
int enqueue_match_both(glim_amd_ctx* ctx, hipStream_t st, const glim_amd_fpfh* target, const glim_amd_fpfh* source, uint32_t flags, MatchBuffers* b);

}  // namespace fpfh_detail
}  // namespace glim_amd
