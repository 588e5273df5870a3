// ransac_table.hpp -- the pieces of ransac.hip that gnc.hip uses as well: the occupancy table of the target, the round buffers and the scoring
// launch.  Declared here, defined in ransac.hip; the scoring kernel stays there and is reached only through launch_score.
#pragma once
#include "internal.hpp"
#include "registration_host.hpp"
#include "sample_hash.hpp"

namespace glim_amd {
namespace ransac_detail {

using glim_amd::sample_hash;
using u64 = unsigned long long;
using u32 = unsigned int;

struct Table {
  DeviceTemp keys;
  u32 slots = 0;
  int in_lds = 0;
};

// occupancy set of `n` target points at 1 / inv_res; synchronises `st` once (the voxel count)
int build_table(glim_amd_ctx* ctx, hipStream_t st, const float4* pts, int n, double inv_res, Table* out);

// what a round of hypotheses lives in: ROUND entries of samples, status, poses and counts, and the fold state
struct RoundBuffers {
  DeviceTemp samples, status, poses, counts, state;
  int alloc();
};

// the first `count` hypotheses of `b` against the table of voxels of edge `resolution`.  Enough blocks for four per compute unit, never fewer
// than 16 hypotheses per block (the table copy and the point loads are per block)
void launch_score(const reg_detail::Pair& p, double resolution, const Table& t, const RoundBuffers& b, int count);

}  // namespace ransac_detail
}  // namespace glim_amd
