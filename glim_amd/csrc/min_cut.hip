// min_cut.hip -- maximum flow / minimum cut on the device for the map editor's min-cut segmentation (points_selector.cpp:774-797; semantics:
// include/glim_amd.h "Map editing", min-cut; interface: min_cut.hpp).  A round-based push-relabel in which no atomic decides a result.
//
// Formulation: the flow runs from the BACKGROUND side.  Excess starts as each node's sink capacity, every node may absorb up to its own
// source capacity, and the flow is the total absorbed.  The graph is symmetric, so swapping the terminals turns "can reach absorbing
// capacity in the residual graph" into "is reachable from the source": the nodes whose exact height is finite after the last relabelling
// are the minimal source side of a minimum cut.  Excess that cannot reach absorbing capacity stays where it is; no second phase turns the
// preflow into a flow, because the arcs it would change lie among nodes that cannot reach absorbing capacity either.
//
// Layout: CSR by tail node; the arcs of edge e are a = 2 e (x -> y) and a ^ 1 (y -> x), ordered within a node by arc id (a stable sort of
// the tails through sort.hip).  Per slot: the head node, the slot of the reverse arc, the 32-bit residual.  Per node: 64-bit excess, 32-bit
// absorbing capacity, height.
//
// Passes (one lane per node or per arc, 256-thread blocks):
//   mc_arc_key_kernel / mc_row_kernel / mc_slot_kernel   the CSR from the edge list
//   mc_init_kernel          excess, absorbing capacity (what a node can hand from its own sink arc to its own source arc is moved here)
//   mc_label_init_kernel, mc_label_round_kernel   exact relabelling: pull rounds over the residual arcs, shaped like map_edit.hip's growth
//   mc_decide_kernel, mc_apply_kernel             one push round
//   mc_active_kernel        number of nodes with excess and a finite height (a counter the host looks at)
//   mc_flag_kernel, mc_sum_kernel                 membership flags and the flow, block partials in block order
#include <algorithm>
#include <climits>
#include <vector>

#include "min_cut.hpp"
#include "scope_sync.hpp"

namespace glim_amd {
namespace mincut {

using u64 = unsigned long long;
using u32 = unsigned int;
using i64 = long long;

constexpr int RPL = GLIM_AMD_EDIT_ROUNDS_PER_LOOK;
constexpr int INF = INT_MAX;  // height of a node that reaches no absorbing capacity

static inline int grid_for(int n) { return (n + 255) / 256; }

// keys[a] = tail of arc a
static __global__ __launch_bounds__(256) void mc_arc_key_kernel(const int2* __restrict__ edges, int A, u64* __restrict__ keys) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= A) return;
  const int2 e = edges[a >> 1];
  keys[a] = (u64)(u32)((a & 1) ? e.y : e.x);
}

// keys sorted by tail, vals the arcs: node v owns the slots [rs[v], re[v]) (both zero for a node without arcs: the arrays are cleared
// first); pos[a] = the slot of arc a
static __global__ __launch_bounds__(256) void mc_row_kernel(const u64* __restrict__ keys, const u32* __restrict__ vals, int A, int* __restrict__ rs,
                                                            int* __restrict__ re, int* __restrict__ pos) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= A) return;
  const u64 k = keys[s];
  if (s == 0 || keys[s - 1] != k) rs[k] = s;
  if (s == A - 1 || keys[s + 1] != k) re[k] = s + 1;
  pos[vals[s]] = s;
}

static __global__ __launch_bounds__(256) void mc_slot_kernel(const u32* __restrict__ vals, const int* __restrict__ pos, const int2* __restrict__ edges,
                                                             const int* __restrict__ cap, int A, int* __restrict__ nbr, int* __restrict__ rev,
                                                             int* __restrict__ res) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= A) return;
  const int a = (int)vals[s];
  const int2 e = edges[a >> 1];
  nbr[s] = (a & 1) ? e.x : e.y;
  rev[s] = pos[a ^ 1];
  res[s] = cap[a >> 1];
}

static __global__ __launch_bounds__(256) void mc_init_kernel(const int* __restrict__ source_cap, const int* __restrict__ sink_cap, int n,
                                                             i64* __restrict__ excess, int* __restrict__ absorb, int* __restrict__ push_slot,
                                                             int* __restrict__ push_amt) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const int t = min(source_cap[v], sink_cap[v]);
  excess[v] = (i64)(sink_cap[v] - t);
  absorb[v] = source_cap[v] - t;
  push_slot[v] = -1;
  push_amt[v] = 0;
}

static __global__ __launch_bounds__(256) void mc_label_init_kernel(const int* __restrict__ absorb, int n, int* __restrict__ h) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v < n) h[v] = absorb[v] > 0 ? 1 : INF;
}

// One pull round of the exact relabelling: an unlabelled node takes height rho iff one of its residual arcs leads to a node of a height
// < rho.  Heights are read and written with plain 32-bit accesses: a height written in THIS round is rho, which the test `< rho` rejects
// like the INF it replaced, so what a lane sees of its neighbours' stores does not matter.  prev: the counter of the round before (null:
// run anyway); a round after one that labelled nothing returns at once.  cnt: nodes this round labelled (a counter, not a result).
static __global__ __launch_bounds__(256) void mc_label_round_kernel(const int* __restrict__ rs, const int* __restrict__ re, const int* __restrict__ nbr,
                                                                    const int* __restrict__ res, int n, int rho, int* h, const int* __restrict__ prev,
                                                                    int* __restrict__ cnt) {
  if (prev && *prev == 0) return;
  const int v = blockIdx.x * 256 + threadIdx.x;
  bool hit = false;
  if (v < n && h[v] == INF) {
    const int s1 = re[v];
    for (int s = rs[v]; s < s1; s++) {
      if (res[s] > 0 && h[nbr[s]] < rho) {
        hit = true;
        break;
      }
    }
    if (hit) h[v] = rho;
  }
  const u64 mask = __ballot(hit);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd(cnt, __popcll(mask));
}

// cnt += nodes that hold excess and reach absorbing capacity (after an exact relabelling: the flow is maximal iff there is none)
static __global__ __launch_bounds__(256) void mc_active_kernel(const i64* __restrict__ excess, const int* __restrict__ h, int n, int* __restrict__ cnt) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  const bool active = v < n && excess[v] > 0 && h[v] < INF;
  const u64 mask = __ballot(active);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd(cnt, __popcll(mask));
}

// Push round, first half.  A node with excess and a finite height first absorbs; with excess left it takes its residual arc to the lowest
// neighbour by THIS round's heights (the first such slot), and either records one push over it in its own slot -- its own height being
// greater -- or writes its new height, lowest + 1 (INF without a residual arc), into the next-height buffer.  Every store goes to the lane's
// own node.  prev: active nodes of the round before (a round after an idle one returns at once); cnt: active nodes of this round.
static __global__ __launch_bounds__(256) void mc_decide_kernel(const int* __restrict__ rs, const int* __restrict__ re, const int* __restrict__ nbr,
                                                               const int* __restrict__ res, const int* __restrict__ h, int n, i64* __restrict__ excess,
                                                               int* __restrict__ absorb, int* __restrict__ hn, int* __restrict__ push_slot,
                                                               int* __restrict__ push_amt, const int* __restrict__ prev, int* __restrict__ cnt) {
  if (*prev == 0) return;
  const int v = blockIdx.x * 256 + threadIdx.x;
  bool active = false;
  if (v < n) {
    const int hv = h[v];
    int nh = hv, ps = -1, pa = 0;
    i64 ex = excess[v];
    if (ex > 0 && hv < INF) {
      active = true;
      const int ab = absorb[v];
      if (ab > 0) {
        const int t = (int)min(ex, (i64)ab);
        ex -= t;
        excess[v] = ex;
        absorb[v] = ab - t;
      }
      if (ex > 0) {
        int hmin = INF, smin = -1;
        const int s1 = re[v];
        for (int s = rs[v]; s < s1; s++) {
          if (res[s] <= 0) continue;
          const int hw = h[nbr[s]];
          if (hw < hmin) hmin = hw, smin = s;
        }
        if (smin < 0) nh = INF;
        else if (hv > hmin) ps = smin, pa = (int)min(ex, (i64)res[smin]);
        else nh = hmin + 1;
      }
    }
    hn[v] = nh;
    push_slot[v] = ps;
    push_amt[v] = pa;
  }
  const u64 mask = __ballot(active);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd(cnt, __popcll(mask));
}

// Push round, second half.  Every node subtracts its own recorded push, then scans its arcs and, for each neighbour whose recorded push is
// the reverse arc, adds that amount to the arc's residual and to its own excess; it takes its next height.  Reads of other nodes touch only
// what mc_decide_kernel wrote; every store goes to the lane's own node and slots.  cur: this round's active count (zero: nothing recorded).
static __global__ __launch_bounds__(256) void mc_apply_kernel(const int* __restrict__ rs, const int* __restrict__ re, const int* __restrict__ nbr,
                                                              const int* __restrict__ rev, const int* __restrict__ hn, const int* __restrict__ push_slot,
                                                              const int* __restrict__ push_amt, int n, int* __restrict__ res, i64* __restrict__ excess,
                                                              int* __restrict__ h, const int* __restrict__ cur) {
  if (*cur == 0) return;
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  i64 ex = excess[v];
  const int ps = push_slot[v];
  if (ps >= 0) {
    const int pa = push_amt[v];
    res[ps] -= pa;
    ex -= pa;
  }
  const int s1 = re[v];
  for (int s = rs[v]; s < s1; s++) {
    const int w = nbr[s];
    if (push_slot[w] == rev[s]) {
      const int pa = push_amt[w];
      res[s] += pa;
      ex += pa;
    }
  }
  excess[v] = ex;
  h[v] = hn[v];
}

// flags[v] = the exact height of v is finite; flags[n] = 0; partial[block] = what the block's nodes absorbed (a fixed butterfly per block)
static __global__ __launch_bounds__(256) void mc_flag_kernel(const int* __restrict__ h, const int* __restrict__ source_cap, const int* __restrict__ absorb, int n, int* __restrict__ flags, i64* __restrict__ partial) {
  __shared__ i64 s_sum[4];
  const int v = blockIdx.x * 256 + threadIdx.x;
  i64 a = 0;
  if (v < n) {
    flags[v] = h[v] < INF ? 1 : 0;
    a = (i64)source_cap[v] - (i64)absorb[v];  // includes what mc_init_kernel moved from the node's own sink arc
  } else if (v == n) {
    flags[v] = 0;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
}

static __global__ __launch_bounds__(256) void mc_sum_kernel(const i64* __restrict__ partial, int blocks, i64* __restrict__ total) {
  __shared__ i64 s_sum[4];
  i64 a = 0;
  for (int b = threadIdx.x; b < blocks; b += 256) a += partial[b];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) total[0] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
}

}  // namespace mincut

int max_flow_source_side(glim_amd_ctx* ctx, hipStream_t st, int n, int num_edges, const int2* edges, const int* cap, const int* source_cap,
                         const int* sink_cap, int max_rounds, int* flags, MaxFlowResult* out) {
  using namespace mincut;
  *out = MaxFlowResult();
  if (n < 0 || num_edges < 0 || n > (1 << 30) || num_edges > (1 << 30) - 256 || max_rounds < 0) return GLIM_AMD_ERR_INVALID;
  if (n == 0) return GLIM_AMD_OK;
  const int limit = max_rounds > 0 ? max_rounds : GLIM_AMD_EDIT_MIN_CUT_MAX_ROUNDS;
  // every buffer is sized by the node count and the arc count
  const int A = 2 * num_edges, nb = grid_for(n), fb = grid_for(n + 1);
  const size_t nn = (size_t)n, aa = (size_t)std::max(A, 1);
  DeviceTemp ka, kb, va, vb, sort_scratch, rs, re, pos, nbr, rev, res, excess, absorb, h, hn, push_slot, push_amt, cnt, partial, total;
  GA_HIP(pool_malloc(&rs.p, nn * sizeof(int)));
  GA_HIP(pool_malloc(&re.p, nn * sizeof(int)));
  GA_HIP(pool_malloc(&nbr.p, aa * sizeof(int)));
  GA_HIP(pool_malloc(&rev.p, aa * sizeof(int)));
  GA_HIP(pool_malloc(&res.p, aa * sizeof(int)));
  GA_HIP(pool_malloc(&excess.p, nn * sizeof(i64)));
  GA_HIP(pool_malloc(&absorb.p, nn * sizeof(int)));
  GA_HIP(pool_malloc(&h.p, nn * sizeof(int)));
  GA_HIP(pool_malloc(&hn.p, nn * sizeof(int)));
  GA_HIP(pool_malloc(&push_slot.p, nn * sizeof(int)));
  GA_HIP(pool_malloc(&push_amt.p, nn * sizeof(int)));
  GA_HIP(pool_malloc(&cnt.p, (size_t)(RPL + 2) * sizeof(int)));
  GA_HIP(pool_malloc(&partial.p, (size_t)fb * sizeof(i64)));
  GA_HIP(pool_malloc(&total.p, sizeof(i64)));
  if (A > 0) {
    GA_HIP(pool_malloc(&ka.p, aa * sizeof(u64)));
    GA_HIP(pool_malloc(&kb.p, aa * sizeof(u64)));
    GA_HIP(pool_malloc(&va.p, aa * sizeof(u32)));
    GA_HIP(pool_malloc(&vb.p, aa * sizeof(u32)));
    GA_HIP(pool_malloc(&pos.p, aa * sizeof(int)));
    GA_HIP(pool_malloc(&sort_scratch.p, radix_sort_scratch_bytes(A)));
  }
  SyncOnExit in_flight(st);
  GA_HIP(hipMemsetAsync(rs.p, 0, nn * sizeof(int), st));
  GA_HIP(hipMemsetAsync(re.p, 0, nn * sizeof(int), st));
  if (A > 0) {
    const int ab = grid_for(A);
    int bits = 1;
    while (((int64_t)1 << bits) < (int64_t)n) bits++;
    mc_arc_key_kernel<<<ab, 256, 0, st>>>(edges, A, ka.as<u64>());
    GA_HIP(hipGetLastError());
    u64* keys = nullptr;
    u32* vals = nullptr;
    GA_HIP(radix_sort_pairs(st, A, bits, ka.as<u64>(), va.as<u32>(), kb.as<u64>(), vb.as<u32>(), true, sort_scratch.as<int>(), &keys, &vals));
    mc_row_kernel<<<ab, 256, 0, st>>>(keys, vals, A, rs.as<int>(), re.as<int>(), pos.as<int>());
    mc_slot_kernel<<<ab, 256, 0, st>>>(vals, pos.as<int>(), edges, cap, A, nbr.as<int>(), rev.as<int>(), res.as<int>());
    GA_HIP(hipGetLastError());
  }
  mc_init_kernel<<<nb, 256, 0, st>>>(source_cap, sink_cap, n, excess.as<i64>(), absorb.as<int>(), push_slot.as<int>(), push_amt.as<int>());
  GA_HIP(hipGetLastError());

  // exact heights, then "is any node with excess still reachable": chunks of RPL pull rounds, one look per chunk; cnt[RPL + 1] is only
  // meaningful in the look that finds the relabelling finished.  A breadth-first search over n nodes has at most n levels.
  auto relabel = [&](int* active) -> int {
    mc_label_init_kernel<<<nb, 256, 0, st>>>(absorb.as<int>(), n, h.as<int>());
    GA_HIP(hipGetLastError());
    int enqueued = 0;
    bool done = false;
    while (!done) {
      GA_HIP(hipMemsetAsync(cnt.p, 1, sizeof(int), st));  // "the round before the chunk labelled something"
      GA_HIP(hipMemsetAsync(cnt.as<int>() + 1, 0, (size_t)(RPL + 1) * sizeof(int), st));
      for (int i = 1; i <= RPL; i++)
        mc_label_round_kernel<<<nb, 256, 0, st>>>(rs.as<int>(), re.as<int>(), nbr.as<int>(), res.as<int>(), n, 1 + enqueued + i, h.as<int>(),
                                                  cnt.as<int>() + i - 1, cnt.as<int>() + i);
      mc_active_kernel<<<nb, 256, 0, st>>>(excess.as<i64>(), h.as<int>(), n, cnt.as<int>() + RPL + 1);
      GA_HIP(hipGetLastError());
      int h_cnt[RPL + 2];
      GA_HIP(read_back_sync(ctx, st, h_cnt, cnt.p, sizeof(h_cnt)));
      for (int i = 1; i <= RPL && !done; i++)
        if (h_cnt[i] == 0) done = true;
      enqueued += RPL;
      if (enqueued > n) done = true;
      *active = h_cnt[RPL + 1];
    }
    return GLIM_AMD_OK;
  };

  int active = 0;
  GA_TRY(relabel(&active));
  while (active > 0 && out->rounds < limit) {
    const int chunk = std::min(RPL, limit - out->rounds);
    GA_HIP(hipMemsetAsync(cnt.p, 1, sizeof(int), st));  // "the round before the chunk had an active node"
    GA_HIP(hipMemsetAsync(cnt.as<int>() + 1, 0, (size_t)RPL * sizeof(int), st));
    for (int i = 1; i <= chunk; i++) {
      mc_decide_kernel<<<nb, 256, 0, st>>>(rs.as<int>(), re.as<int>(), nbr.as<int>(), res.as<int>(), h.as<int>(), n, excess.as<i64>(), absorb.as<int>(),
                                           hn.as<int>(), push_slot.as<int>(), push_amt.as<int>(), cnt.as<int>() + i - 1, cnt.as<int>() + i);
      mc_apply_kernel<<<nb, 256, 0, st>>>(rs.as<int>(), re.as<int>(), nbr.as<int>(), rev.as<int>(), hn.as<int>(), push_slot.as<int>(), push_amt.as<int>(), n,
                                          res.as<int>(), excess.as<i64>(), h.as<int>(), cnt.as<int>() + i);
    }
    GA_HIP(hipGetLastError());
    out->rounds += chunk;
    out->looks++;
    GA_TRY(relabel(&active));
  }
  if (active > 0) {  // the round limit: no flags, no flow
    out->status = GLIM_AMD_EDIT_ROUND_LIMIT;
    GA_HIP(hipMemsetAsync(flags, 0, (nn + 1) * sizeof(int), st));
    GA_HIP(hipStreamSynchronize(st));
    in_flight.dismiss();
    return GLIM_AMD_OK;
  }
  mc_flag_kernel<<<fb, 256, 0, st>>>(h.as<int>(), source_cap, absorb.as<int>(), n, flags, partial.as<i64>());
  mc_sum_kernel<<<1, 256, 0, st>>>(partial.as<i64>(), fb, total.as<i64>());
  GA_HIP(hipGetLastError());
  GA_HIP(read_back_sync(ctx, st, &out->flow, total.p, sizeof(i64)));
  in_flight.dismiss();
  return GLIM_AMD_OK;
}

}  // namespace glim_amd

extern "C" {

int glim_amd_diag_max_flow(glim_amd_ctx* ctx, int32_t n, int64_t num_edges, const int32_t* edges, const int32_t* edge_cap, const int32_t* source_cap,
                           const int32_t* sink_cap, int32_t max_rounds, int32_t* member, int64_t* flow, int32_t* rounds, int32_t* looks, int32_t* status) {
  using namespace glim_amd;
  if (glim_amd_device_count() <= 0) return GLIM_AMD_ERR_NO_DEVICE;
  if (!ctx || !flow || !rounds || !looks || !status || n < 0 || num_edges < 0 || n > (1 << 30) || num_edges > (int64_t)(1 << 30) - 256 || max_rounds < 0)
    return GLIM_AMD_ERR_INVALID;
  if (n > 0 && (!source_cap || !sink_cap || !member)) return GLIM_AMD_ERR_INVALID;
  if (num_edges > 0 && (!edges || !edge_cap)) return GLIM_AMD_ERR_INVALID;
  for (int64_t e = 0; e < num_edges; e++) {
    const int32_t i = edges[2 * e], j = edges[2 * e + 1];
    if (i < 0 || j < 0 || i >= n || j >= n || i == j || edge_cap[e] < 0) return GLIM_AMD_ERR_INVALID;
  }
  for (int32_t v = 0; v < n; v++)
    if (source_cap[v] < 0 || sink_cap[v] < 0) return GLIM_AMD_ERR_INVALID;
  *flow = 0, *rounds = 0, *looks = 0, *status = GLIM_AMD_EDIT_OK;
  if (n == 0) return GLIM_AMD_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  const size_t nn = (size_t)n, ee = (size_t)std::max<int64_t>(num_edges, 1);
  DeviceTemp d_edges, d_cap, d_src, d_snk, d_flags;
  GA_HIP(pool_malloc(&d_edges.p, ee * sizeof(int2)));
  GA_HIP(pool_malloc(&d_cap.p, ee * sizeof(int)));
  GA_HIP(pool_malloc(&d_src.p, nn * sizeof(int)));
  GA_HIP(pool_malloc(&d_snk.p, nn * sizeof(int)));
  GA_HIP(pool_malloc(&d_flags.p, (nn + 1) * sizeof(int)));
  SyncOnExit in_flight(st);
  if (num_edges > 0) {
    GA_HIP(hipMemcpyAsync(d_edges.p, edges, (size_t)num_edges * sizeof(int2), hipMemcpyHostToDevice, st));
    GA_HIP(hipMemcpyAsync(d_cap.p, edge_cap, (size_t)num_edges * sizeof(int), hipMemcpyHostToDevice, st));
  }
  GA_HIP(hipMemcpyAsync(d_src.p, source_cap, nn * sizeof(int), hipMemcpyHostToDevice, st));
  GA_HIP(hipMemcpyAsync(d_snk.p, sink_cap, nn * sizeof(int), hipMemcpyHostToDevice, st));
  MaxFlowResult r;
  GA_TRY(max_flow_source_side(ctx, st, n, (int)num_edges, d_edges.as<int2>(), d_cap.as<int>(), d_src.as<int>(), d_snk.as<int>(), max_rounds,
                              d_flags.as<int>(), &r));
  GA_HIP(hipMemcpyAsync(member, d_flags.p, nn * sizeof(int), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  *flow = r.flow, *rounds = r.rounds, *looks = r.looks, *status = r.status;
  return GLIM_AMD_OK;
}

}  // extern "C"
