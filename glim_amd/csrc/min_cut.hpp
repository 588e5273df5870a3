// min_cut.hpp -- interface of the maximum-flow / minimum-cut solver of the map editor's min-cut segmentation (min_cut.hip): a round-based
// push-relabel on an undirected integer-capacity graph with per-node source and sink capacities.  Called by map_edit.hip
// (glim_amd_edit_min_cut) with the candidates' neighbour graph and by glim_amd_diag_max_flow with a caller's graph.
#pragma once
#include <hip/hip_runtime.h>

#include "internal.hpp"

namespace glim_amd {

struct MaxFlowResult {
  long long flow = 0;  // the maximum flow in capacity units (0 with GLIM_AMD_EDIT_ROUND_LIMIT)
  int rounds = 0;      // push rounds enqueued
  int looks = 0;       // chunks of push rounds, i.e. exact relabellings after the first
  int status = GLIM_AMD_EDIT_OK;  // or GLIM_AMD_EDIT_ROUND_LIMIT
};

// n nodes; num_edges undirected edges (edges[e].x, edges[e].y), x != y, of capacity cap[e] >= 0 in either direction; node v is tied to the
// source with source_cap[v] >= 0 and to the sink with sink_cap[v] >= 0.  All arrays in device memory.  flags: n + 1 ints on the device;
// flags[v] = 1 iff v is reachable from the source in the residual graph of a maximum flow (the minimal source side of a minimum cut),
// flags[n] = 0; all 0 when max_rounds (> 0) push rounds did not finish the flow.  Caller holds ctx->mu with the device set; the function
// enqueues on `st`, reads its counters back between chunks and returns with the stream idle.
int max_flow_source_side(::glim_amd_ctx* ctx, hipStream_t st, int n, int num_edges, const int2* edges, const int* cap, const int* source_cap,
                         const int* sink_cap, int max_rounds, int* flags, MaxFlowResult* out);

}  // namespace glim_amd
