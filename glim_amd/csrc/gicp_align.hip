// gicp_align.hip -- GICP fine registration on gfx950 (include/glim_amd.h "GICP fine registration"): B independent Levenberg-Marquardt loops over
// the rigid GICP factor, one host synchronisation.  The per-point algebra, the block epilogue, the ordered sum and the target description are
// gicp_factor.hpp's (the map's description ivox_map.hpp's), shared with gicp.hip: called here, not copied.  The host scaffold is align_host.hpp's.
// This is the scheme of every loop; vgicp_align.hip (VGICP, scan-to-keyframes), ct_align.hip (CT-GICP) and bundle_align.hip (sub-map bundle,
// global graph) say what their round is and refer here for the rest.
//
//   problem table   per problem: the factor kernel's arguments (target half from gicp_target(), source half from set_source), the map's search
//                   object when the targets are device iVoxes, and where its partial rows are (first, count)
//   block table     (problem, begin, end) per block, as ct_gicp_kernel's.  A problem's points are cut EXACTLY as run_gicp cuts that source alone --
//                   the same points_per_thread(ctx, n), the same chunk order -- and its rows are added by the same ordered sum, so every trial
//                   record is bit for bit what glim_amd_gicp_linearize returns at that pose (tests/test_gicp_align_gpu.py).
//   a round         two ordinary launches: align_linearize_kernel over all blocks (a block of a finished problem reads the status and returns;
//                   its row is never read), then align_decide_kernel, one block per problem: the ordered sum into the compact record, the step
//                   rule of lm_step.hpp, the next candidate pose and the state, one trace entry when a trace was asked for.
//   the call        1 + max_trials rounds are enqueued up front, then one copy of the states, then ONE hipStreamSynchronize.  No persistent
//                   kernel, no grid-wide wait, no host decision in between; every loop in both kernels has a bound known at launch.
//
// The ICP fine registration (include/glim_amd.h "ICP fine registration") is the same scheme with the ICP factors' per-point algebra
// (icp_factor.hpp) in the linearising kernel: icp_align_linearize_kernel, then the same decide kernel.  Its trial budget is 400, and an ICP loop
// stops after a dozen or two trials, so its rounds are enqueued in chunks: at most 41 at a time, then the states are copied back and the call
// stops enqueueing when no status is RUNNING.  The state lives on the device, so the chunk length moves no bit of a result; the GICP loop
// passes chunk 0 and keeps its single synchronisation.  The global graph (bundle_align.hip) enqueues in chunks in the same way.
#include "align_host.hpp"
#include "device_math.hpp"
#include "gicp_factor.hpp"
#include "icp_factor.hpp"
#include "ivox_map.hpp"
#include "lm_step.hpp"

namespace {

struct AlignProblem {
  GicpArgs a;      // a.T is not used: the pose of a round is the state's candidate
  IvoxSearch nn;   // iVox targets only
  int first, nb;   // the problem's partial rows
  const float4* normals;  // the target cloud's normals in its original order (the point-to-plane ICP factor only)
};

template <class NN>
__device__ __forceinline__ NN align_search(const AlignProblem& p);
template <>
__device__ __forceinline__ IndexSearch align_search<IndexSearch>(const AlignProblem&) {
  return IndexSearch{};
}
template <>
__device__ __forceinline__ IvoxSearch align_search<IvoxSearch>(const AlignProblem& p) {
  return p.nn;
}

// gicp_kernel<true> over the blocks of every running problem: block (problem, begin, end) takes the points gicp_kernel's block of the same chunk
// takes, lane by lane in the same order, at the problem's candidate pose
template <class NN>
__global__ __launch_bounds__(BLOCK) void align_linearize_kernel(const AlignProblem* __restrict__ table, const int4* __restrict__ blocks,
                                                                const lm::State* __restrict__ states, float* __restrict__ partials) {
  __shared__ float s_red[4][PARTIAL_STRIDE];
  const int4 blk = blocks[blockIdx.x];
  if (states[blk.x].status != lm::RUNNING) return;  // the same for every thread of the block
  const GicpArgs a = table[blk.x].a;
  const NN nn = align_search<NN>(table[blk.x]);
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = states[blk.x].cand[k];
  const Rot32 R(T);
  float acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; j++) acc[j] = 0.f;
  int inliers = 0;
  for (int i = blk.y + (int)threadIdx.x; i < blk.z; i += BLOCK) {
    const float4 p = a.pts[i];
    double qx, qy, qz;
    transform_point_d(T, (double)p.x, (double)p.y, (double)p.z, qx, qy, qz);
    double best_d;
    const int j = nn.find(a, qx, qy, qz, best_d);
    if (j < 0) continue;
    inliers++;
    float A[6];
    gicp_point<true>(acc, R.r00, R.r01, R.r02, R.r10, R.r11, R.r12, R.r20, R.r21, R.r22, p, a.sorted[j], a.tA[j], a.tB[j], a.covA[i], a.covB[i], qx, qy, qz, A);
  }
  store_partial_row(acc, inliers, s_red, partials);
}

// icp_kernel<true, PLANE> (gicp.hip) over the blocks of every running problem, in the same way: the ICP fine registration
template <bool PLANE>
__global__ __launch_bounds__(BLOCK) void icp_align_linearize_kernel(const AlignProblem* __restrict__ table, const int4* __restrict__ blocks,
                                                                    const lm::State* __restrict__ states, float* __restrict__ partials) {
  __shared__ float s_red[4][PARTIAL_STRIDE];
  const int4 blk = blocks[blockIdx.x];
  if (states[blk.x].status != lm::RUNNING) return;  // the same for every thread of the block
  const GicpArgs a = table[blk.x].a;
  const float4* __restrict__ normals = table[blk.x].normals;
  const IndexSearch nn{};
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = states[blk.x].cand[k];
  const Rot32 R(T);
  float acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; j++) acc[j] = 0.f;
  int inliers = 0;
  for (int i = blk.y + (int)threadIdx.x; i < blk.z; i += BLOCK) {
    const float4 p = a.pts[i];
    double qx, qy, qz;
    transform_point_d(T, (double)p.x, (double)p.y, (double)p.z, qx, qy, qz);
    double best_d;
    const int j = nn.find(a, qx, qy, qz, best_d);
    if (j < 0) continue;
    inliers++;
    const float4 b = a.sorted[j];
    icp_point<true, PLANE>(acc, R, p, b, PLANE ? icp_normal(normals, b) : make_float4(0.f, 0.f, 0.f, 0.f), qx, qy, qz);
  }
  store_partial_row(acc, inliers, s_red, partials);
}

// one block of 256 threads per problem: gicp_finalize_kernel's sum of the problem's rows, then the step rule in thread 0
__global__ __launch_bounds__(256) void align_decide_kernel(const AlignProblem* __restrict__ table, const float* __restrict__ partials, lm::State* __restrict__ states,
                                                           const lm::Params prm, glim_amd_align_trace_entry* __restrict__ trace, int round, int rounds) {
  __shared__ double s_part[8][PARTIAL_STRIDE];
  __shared__ double s_sum[PARTIAL_STRIDE];
  const int p = blockIdx.x;
  if (states[p].status != lm::RUNNING) return;  // the same for every thread of the block
  sum_partial_rows(partials + (size_t)table[p].first * PARTIAL_STRIDE, table[p].nb, s_part, s_sum);
  if (threadIdx.x != 0) return;
  double rec[COMPACT];
  for (int t = 0; t < COMPACT; t++) rec[t] = compact_entry(s_sum, t);
  lm::State s;
  decide_problem(prm, states + p, s, rec, trace ? trace + ((size_t)p * rounds + round) : nullptr);
}

void icp_default_params(glim_amd_lm_params* p) {
  lm_default_params(p);
  p->max_iterations = 200;  // manual_loop_close_modal.cpp:490
}

// the most rounds the ICP fine registration enqueues before it looks at the statuses: the most the other loops enqueue by default (1 + 2 x 20)
constexpr int ICP_ROUNDS_PER_CHUNK = 41;

// the batch over either kind of target: Handle = glim_amd_nn_index or glim_amd_ivox.  trace: count * (1 + max_trials) entries, or null.
// metric: the factor of the loop (the ICP factors: an index only).  chunk: rounds enqueued between two looks at the statuses; 0: all of them up
// front and ONE synchronisation.  The state lives on the device: the chunk length moves no bit of a result.
template <class Handle>
int run_align(const Handle* const* targets, const glim_amd_cloud* const* sources, const double* T_init12, const double* max_dists, int32_t count,
              const glim_amd_lm_params* params, glim_amd_align_result* out, glim_amd_align_trace_entry* trace_host, Metric metric = Metric::GICP, int chunk = 0,
              void (*defaults)(glim_amd_lm_params*) = lm_default_params) {
  if (count < 0) return GLIM_AMD_ERR_INVALID;
  if (count == 0) return GLIM_AMD_OK;
  if (!targets || !sources || !T_init12 || !max_dists || !out) return GLIM_AMD_ERR_INVALID;
  lm::Params prm;
  int rounds;
  GA_TRY(resolve_params(params, defaults, &prm, &rounds));
  for (int i = 0; i < count; i++)
    if (!(max_dists[i] >= 0.0)) return GLIM_AMD_ERR_INVALID;
  glim_amd_ctx* ctx = one_context(targets, sources, count, nullptr);
  if (!ctx) return GLIM_AMD_ERR_INVALID;

  std::unique_lock<std::mutex> held(ctx->mu);  // once for the batch: the descriptions below are taken without the lock
  std::vector<AlignProblem> table((size_t)count);
  std::vector<int4> blocks;
  std::vector<lm::State> states((size_t)count);
  bool ivox = false;
  for (int i = 0; i < count; i++) {
    const GicpTarget t = gicp_target(targets[i], false);
    const glim_amd_cloud* source = sources[i];
    if (source->n > t.max_source) return GLIM_AMD_ERR_INVALID;
    GA_TRY(metric_state(metric, t, source));
    if (source->n == 0 || t.empty) return GLIM_AMD_ERR_INVALID;
    const int max_ring = t.rings(max_dists[i]);
    if (max_ring < 0) return GLIM_AMD_ERR_UNSUPPORTED;
    ivox = t.ivox;
    AlignProblem& pr = table[(size_t)i];
    memset(&pr, 0, sizeof(pr));
    pr.a = t.args;
    pr.normals = t.normals;
    const int n = (int)source->n;
    set_source(&pr.a, source, points_per_thread(ctx, n), max_dists[i]);
    pr.a.max_ring = max_ring;
    pr.nn = t.nn;
    pr.first = (int)blocks.size();
    const int chunk = BLOCK * pr.a.ppt;
    for (int b = 0; b < n; b += chunk) blocks.push_back(make_int4(i, b, std::min(n, b + chunk), 0));
    pr.nb = (int)blocks.size() - pr.first;
    lm::init(prm, T_init12 + 12 * (size_t)i, states[(size_t)i]);
  }
  const int nb = (int)blocks.size();

  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  DeviceTemp d_table, d_blocks, d_states, d_partials;
  TraceBuffer trace;
  SyncOnExit in_flight(st);  // an error exit after the launches waits for the stream before the scratch goes back to the pool
  GA_HIP(pool_malloc(&d_table.p, table.size() * sizeof(AlignProblem)));
  GA_HIP(pool_malloc(&d_blocks.p, blocks.size() * sizeof(int4)));
  GA_HIP(pool_malloc(&d_states.p, states.size() * sizeof(lm::State)));
  GA_HIP(pool_malloc(&d_partials.p, (size_t)nb * PARTIAL_STRIDE * sizeof(float)));
  GA_TRY(trace.open(trace_host, (size_t)count * rounds * sizeof(glim_amd_align_trace_entry), st));
  GA_HIP(hipMemcpyAsync(d_table.p, table.data(), table.size() * sizeof(AlignProblem), hipMemcpyHostToDevice, st));
  GA_HIP(hipMemcpyAsync(d_blocks.p, blocks.data(), blocks.size() * sizeof(int4), hipMemcpyHostToDevice, st));
  GA_HIP(hipMemcpyAsync(d_states.p, states.data(), states.size() * sizeof(lm::State), hipMemcpyHostToDevice, st));
  auto linearize = align_linearize_kernel<IndexSearch>;
  if (ivox) linearize = align_linearize_kernel<IvoxSearch>;
  else if (metric == Metric::ICP_POINT) linearize = icp_align_linearize_kernel<false>;
  else if (metric == Metric::ICP_PLANE) linearize = icp_align_linearize_kernel<true>;
  for (int r = 0;;) {
    for (const int end = chunk > 0 ? std::min(rounds, r + chunk) : rounds; r < end; r++) {
      linearize<<<nb, BLOCK, 0, st>>>(d_table.as<AlignProblem>(), d_blocks.as<int4>(), d_states.as<lm::State>(), d_partials.as<float>());
      align_decide_kernel<<<count, 256, 0, st>>>(d_table.as<AlignProblem>(), d_partials.as<float>(), d_states.as<lm::State>(), prm,
                                                 trace.d.as<glim_amd_align_trace_entry>(), r, rounds);
    }
    GA_HIP(hipGetLastError());
    GA_HIP(hipMemcpyAsync(states.data(), d_states.p, states.size() * sizeof(lm::State), hipMemcpyDeviceToHost, st));
    if (r == rounds) break;
    // a chunk's end: the statuses come back with the states, and the loop stops enqueueing when no problem is running
    GA_HIP(hipStreamSynchronize(st));
    if (std::none_of(states.begin(), states.end(), [](const lm::State& s) { return s.status == lm::RUNNING; })) break;
  }
  GA_TRY(trace.fetch(st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  for (int i = 0; i < count; i++) align_result(states[(size_t)i], out + i);
  return GLIM_AMD_OK;
}

}  // namespace

extern "C" {

int glim_amd_gicp_align_default_params(glim_amd_lm_params* params) { return default_params_out(params, lm_default_params); }

int glim_amd_gicp_align_batch(const glim_amd_nn_index* const* targets, const glim_amd_cloud* const* sources, const double* T_init12,
                              const double* max_correspondence_distances, int32_t count, const glim_amd_lm_params* params, glim_amd_align_result* out) {
  return run_align(targets, sources, T_init12, max_correspondence_distances, count, params, out, nullptr);
}

int glim_amd_gicp_align_batch_incremental(const glim_amd_ivox* const* targets, const glim_amd_cloud* const* sources, const double* T_init12,
                                          const double* max_correspondence_distances, int32_t count, const glim_amd_lm_params* params, glim_amd_align_result* out) {
  return run_align(targets, sources, T_init12, max_correspondence_distances, count, params, out, nullptr);
}

int glim_amd_debug_gicp_align_trace(int32_t ivox, const void* const* targets, const glim_amd_cloud* const* sources, const double* T_init12,
                                    const double* max_correspondence_distances, int32_t count, const glim_amd_lm_params* params, glim_amd_align_result* out,
                                    glim_amd_align_trace_entry* trace) {
  if (!trace && count > 0) return GLIM_AMD_ERR_INVALID;
  if (ivox) return run_align(reinterpret_cast<const glim_amd_ivox* const*>(targets), sources, T_init12, max_correspondence_distances, count, params, out, trace);
  return run_align(reinterpret_cast<const glim_amd_nn_index* const*>(targets), sources, T_init12, max_correspondence_distances, count, params, out, trace);
}

int glim_amd_icp_align_default_params(glim_amd_lm_params* params) { return default_params_out(params, icp_default_params); }

int glim_amd_icp_align_batch(const glim_amd_nn_index* const* targets, const glim_amd_cloud* const* sources, const double* T_init12,
                             const double* max_correspondence_distances, uint32_t flags, int32_t count, const glim_amd_lm_params* params, glim_amd_align_result* out) {
  if (flags & ~(uint32_t)GLIM_AMD_ICP_POINT_TO_PLANE) return GLIM_AMD_ERR_INVALID;  // GLIM_AMD_FACTOR_BINARY: the target is fixed
  return run_align(targets, sources, T_init12, max_correspondence_distances, count, params, out, nullptr, icp_metric(flags), ICP_ROUNDS_PER_CHUNK,
                   icp_default_params);
}

int glim_amd_debug_icp_align_trace(const glim_amd_nn_index* const* targets, const glim_amd_cloud* const* sources, const double* T_init12,
                                   const double* max_correspondence_distances, uint32_t flags, int32_t count, const glim_amd_lm_params* params,
                                   glim_amd_align_result* out, glim_amd_align_trace_entry* trace, int32_t rounds_per_chunk) {
  if (flags & ~(uint32_t)GLIM_AMD_ICP_POINT_TO_PLANE) return GLIM_AMD_ERR_INVALID;
  if ((!trace && count > 0) || rounds_per_chunk < 0) return GLIM_AMD_ERR_INVALID;
  return run_align(targets, sources, T_init12, max_correspondence_distances, count, params, out, trace, icp_metric(flags),
                   rounds_per_chunk > 0 ? rounds_per_chunk : ICP_ROUNDS_PER_CHUNK, icp_default_params);
}

}  // extern "C"
