// gicp_align.hip -- GICP fine registration on gfx950 (include/glim_amd.h "GICP fine registration"): B independent Levenberg-Marquardt loops over
// the rigid GICP factor, one host synchronisation.  The per-point algebra, the block epilogue, the ordered sum and the target description are
// gicp_factor.hpp's (the map's description ivox_map.hpp's), shared with gicp.hip: called here, not copied.
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
#include <cmath>
#include <cstddef>
#include <cstring>
#include <mutex>
#include <vector>

#include "device_math.hpp"
#include "gicp_factor.hpp"
#include "internal.hpp"
#include "ivox_map.hpp"
#include "lm_step.hpp"
#include "scope_sync.hpp"

using namespace glim_amd;

namespace {

static_assert(sizeof(lm::Params) == sizeof(glim_amd_lm_params), "lm::Params is the layout of glim_amd_lm_params");
static_assert(offsetof(lm::Params, error_scale) == offsetof(glim_amd_lm_params, error_scale), "lm::Params is the layout of glim_amd_lm_params");
static_assert(lm::RECORD == COMPACT, "the compact record");
static_assert(lm::CONVERGED == GLIM_AMD_ALIGN_CONVERGED && lm::MAX_ITERATIONS == GLIM_AMD_ALIGN_MAX_ITERATIONS && lm::MAX_TRIALS == GLIM_AMD_ALIGN_MAX_TRIALS &&
                  lm::LAMBDA_BOUND == GLIM_AMD_ALIGN_LAMBDA_BOUND && lm::NO_CORRESPONDENCES == GLIM_AMD_ALIGN_NO_CORRESPONDENCES &&
                  lm::NUMERIC == GLIM_AMD_ALIGN_NUMERIC,
              "status values");
constexpr int ALIGN_MAX_TRIALS = 4096;

struct AlignProblem {
  GicpArgs a;      // a.T is not used: the pose of a round is the state's candidate
  IvoxSearch nn;   // iVox targets only
  int first, nb;   // the problem's partial rows
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
  lm::State s = states[p];
  glim_amd_align_trace_entry e;
  for (int k = 0; k < 12; k++) e.T_candidate[k] = s.cand[k];
  e.lambda = s.lambda;
  lm::step(prm, s, rec);
  states[p] = s;
  if (trace) {
    for (int t = 0; t < COMPACT; t++) e.compact[t] = rec[t];
    e.accepted = s.accepted;
    e.status = s.status;
    trace[(size_t)p * rounds + round] = e;
  }
}

bool lm_params_ok(const glim_amd_lm_params& p) {
  const double v[] = {p.lambda_initial, p.lambda_factor, p.lambda_upper_bound, p.lambda_lower_bound, p.relative_error_tol, p.absolute_error_tol, p.error_scale};
  for (double x : v)
    if (!std::isfinite(x)) return false;
  return p.lambda_factor > 1.0 && p.lambda_initial >= 0.0 && p.error_scale > 0.0 && p.max_iterations >= 0 && p.max_trials >= 0 && p.max_trials <= ALIGN_MAX_TRIALS &&
         p.max_iterations <= ALIGN_MAX_TRIALS;
}

void lm_default_params(glim_amd_lm_params* p) {
  memset(p, 0, sizeof(*p));
  p->lambda_initial = 1e-5;
  p->lambda_factor = 10.0;
  p->lambda_upper_bound = 1e5;
  p->lambda_lower_bound = 0.0;
  p->relative_error_tol = 1e-5;
  p->absolute_error_tol = 1e-5;
  p->max_iterations = 10;
  p->max_trials = 0;
  p->error_scale = 1.0;
}

// the batch over either kind of target: Handle = glim_amd_nn_index or glim_amd_ivox.  trace: count * (1 + max_trials) entries, or null
template <class Handle>
int run_align(const Handle* const* targets, const glim_amd_cloud* const* sources, const double* T_init12, const double* max_dists, int32_t count,
              const glim_amd_lm_params* params, glim_amd_align_result* out, glim_amd_align_trace_entry* trace_host) {
  if (count < 0) return GLIM_AMD_ERR_INVALID;
  if (count == 0) return GLIM_AMD_OK;
  if (!targets || !sources || !T_init12 || !max_dists || !out) return GLIM_AMD_ERR_INVALID;
  glim_amd_lm_params prm_c;
  if (params) prm_c = *params;
  else lm_default_params(&prm_c);
  if (!lm_params_ok(prm_c)) return GLIM_AMD_ERR_INVALID;
  if (prm_c.max_trials == 0) prm_c.max_trials = 2 * prm_c.max_iterations;
  if (prm_c.max_trials > ALIGN_MAX_TRIALS) return GLIM_AMD_ERR_INVALID;
  for (int i = 0; i < count; i++) {
    if (!(max_dists[i] >= 0.0) || !targets[i] || !sources[i]) return GLIM_AMD_ERR_INVALID;
  }
  glim_amd_ctx* ctx = targets[0]->ctx;
  for (int i = 0; i < count; i++) {
    if ((glim_amd_ctx*)targets[i]->ctx != ctx || (glim_amd_ctx*)sources[i]->ctx != ctx) return GLIM_AMD_ERR_INVALID;
  }
  lm::Params prm;
  memcpy(&prm, &prm_c, sizeof(prm));
  const int rounds = 1 + prm.max_trials;

  std::unique_lock<std::mutex> held(ctx->mu);  // once for the batch: the descriptions below are taken without the lock
  std::vector<AlignProblem> table((size_t)count);
  std::vector<int4> blocks;
  std::vector<lm::State> states((size_t)count);
  bool ivox = false;
  for (int i = 0; i < count; i++) {
    const GicpTarget t = gicp_target(targets[i], false);
    const glim_amd_cloud* source = sources[i];
    if (source->n > t.max_source) return GLIM_AMD_ERR_INVALID;
    if (!source->has_covs || !t.usable) return GLIM_AMD_ERR_STATE;
    if (source->n == 0 || t.empty) return GLIM_AMD_ERR_INVALID;
    const int max_ring = t.rings(max_dists[i]);
    if (max_ring < 0) return GLIM_AMD_ERR_UNSUPPORTED;
    ivox = t.ivox;
    AlignProblem& pr = table[(size_t)i];
    memset(&pr, 0, sizeof(pr));
    pr.a = t.args;
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
  DeviceTemp d_table, d_blocks, d_states, d_partials, d_trace;
  SyncOnExit in_flight(st);  // an error exit after the launches waits for the stream before the scratch goes back to the pool
  GA_HIP(pool_malloc(&d_table.p, table.size() * sizeof(AlignProblem)));
  GA_HIP(pool_malloc(&d_blocks.p, blocks.size() * sizeof(int4)));
  GA_HIP(pool_malloc(&d_states.p, states.size() * sizeof(lm::State)));
  GA_HIP(pool_malloc(&d_partials.p, (size_t)nb * PARTIAL_STRIDE * sizeof(float)));
  const size_t trace_bytes = (size_t)count * rounds * sizeof(glim_amd_align_trace_entry);
  if (trace_host) {
    GA_HIP(pool_malloc(&d_trace.p, trace_bytes));
    GA_HIP(hipMemsetAsync(d_trace.p, 0, trace_bytes, st));
  }
  GA_HIP(hipMemcpyAsync(d_table.p, table.data(), table.size() * sizeof(AlignProblem), hipMemcpyHostToDevice, st));
  GA_HIP(hipMemcpyAsync(d_blocks.p, blocks.data(), blocks.size() * sizeof(int4), hipMemcpyHostToDevice, st));
  GA_HIP(hipMemcpyAsync(d_states.p, states.data(), states.size() * sizeof(lm::State), hipMemcpyHostToDevice, st));
  for (int r = 0; r < rounds; r++) {
    if (ivox) align_linearize_kernel<IvoxSearch><<<nb, BLOCK, 0, st>>>(d_table.as<AlignProblem>(), d_blocks.as<int4>(), d_states.as<lm::State>(), d_partials.as<float>());
    else align_linearize_kernel<IndexSearch><<<nb, BLOCK, 0, st>>>(d_table.as<AlignProblem>(), d_blocks.as<int4>(), d_states.as<lm::State>(), d_partials.as<float>());
    align_decide_kernel<<<count, 256, 0, st>>>(d_table.as<AlignProblem>(), d_partials.as<float>(), d_states.as<lm::State>(), prm,
                                               d_trace.as<glim_amd_align_trace_entry>(), r, rounds);
  }
  GA_HIP(hipGetLastError());
  GA_HIP(hipMemcpyAsync(states.data(), d_states.p, states.size() * sizeof(lm::State), hipMemcpyDeviceToHost, st));
  if (trace_host) GA_HIP(hipMemcpyAsync(trace_host, d_trace.p, trace_bytes, hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  for (int i = 0; i < count; i++) {
    const lm::State& s = states[(size_t)i];
    glim_amd_align_result& o = out[i];
    memset(&o, 0, sizeof(o));
    memcpy(o.T_target_source, s.T, sizeof(o.T_target_source));
    memcpy(o.compact, s.rec, sizeof(o.compact));
    o.error = s.rec[1];
    o.num_inliers = (int64_t)llround(s.rec[0]);
    o.iterations = s.iterations;
    o.trials = s.trials;
    o.status = s.status;
    o.lambda = s.lambda;
  }
  return GLIM_AMD_OK;
}

}  // namespace

extern "C" {

int glim_amd_gicp_align_default_params(glim_amd_lm_params* params) {
  if (!params) return GLIM_AMD_ERR_INVALID;
  lm_default_params(params);
  return GLIM_AMD_OK;
}

int glim_amd_gicp_align_batch(const glim_amd_nn_index* const* targets, const glim_amd_cloud* const* sources, const double* T_init12,
                              const double* max_correspondence_distances, int32_t count, const glim_amd_lm_params* params,
                              glim_amd_align_result* out) {
  return run_align(targets, sources, T_init12, max_correspondence_distances, count, params, out, nullptr);
}

int glim_amd_gicp_align_batch_incremental(const glim_amd_ivox* const* targets, const glim_amd_cloud* const* sources, const double* T_init12,
                                   const double* max_correspondence_distances, int32_t count, const glim_amd_lm_params* params,
                                   glim_amd_align_result* out) {
  return run_align(targets, sources, T_init12, max_correspondence_distances, count, params, out, nullptr);
}

int glim_amd_debug_gicp_align_trace(int32_t ivox, const void* const* targets, const glim_amd_cloud* const* sources, const double* T_init12,
                                    const double* max_correspondence_distances, int32_t count, const glim_amd_lm_params* params,
                                    glim_amd_align_result* out, glim_amd_align_trace_entry* trace) {
  if (!trace && count > 0) return GLIM_AMD_ERR_INVALID;
  if (ivox) return run_align(reinterpret_cast<const glim_amd_ivox* const*>(targets), sources, T_init12, max_correspondence_distances, count, params, out, trace);
  return run_align(reinterpret_cast<const glim_amd_nn_index* const*>(targets), sources, T_init12, max_correspondence_distances, count, params, out, trace);
}

}  // extern "C"
