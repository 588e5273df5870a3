// vgicp_align.hip -- the Levenberg-Marquardt loops over vgicp_batch.hpp on gfx950: the VGICP fine registration and the scan-to-keyframes
// registration.  The scheme is gicp_align.hip's, the host scaffold align_host.hpp's.
//
// The VGICP fine registration (include/glim_amd.h "VGICP fine registration") is the scheme over voxel-map targets.  The factor's hot loop, its
// plan and its ordered sum live in vgicp.hip and stay there: a round is vgicp_batch_round (vgicp_batch.hpp: vgicp.hip's row kernels and
// finalising blocks behind the status check, over a transient plan of the batch's pairs, leaving finished compact records on the device) and
// vgicp_align_decide_kernel here, which runs the step rule of lm_step.hpp on those records and writes each problem's next candidate into the
// plan's pose buffer.
//
// The scan-to-keyframes VGICP registration (include/glim_amd.h "Scan-to-keyframes VGICP registration") is the same scheme over ONE pose per
// problem and M unary VGICP factors with fixed target poses: a round is vgicp_batch_round over the F factors of all problems at T_f = P_f^-1 X,
// each behind a status word of its own, and the keyframe decide kernel (below) -- a six-parameter solve per problem, no dense bundle
// (keyframe_lm_step.hpp, which takes the prior's term products from the bundle's rule).
#include "align_host.hpp"
#include "keyframe_lm_step.hpp"
#include "lm_step.hpp"
#include "vgicp_batch.hpp"

namespace {

// ---- the VGICP fine registration: the decide step over records vgicp.hip's round left on the device (vgicp_batch.hpp) ----
// one thread per problem: the step rule on the finished compact record, the state, and the next candidate into the pose buffer the row kernels
// of the next round read
constexpr int VGICP_DECIDE_THREADS = 64;
__global__ __launch_bounds__(VGICP_DECIDE_THREADS) void vgicp_align_decide_kernel(const double* __restrict__ records, double* __restrict__ poses, lm::State* __restrict__ states,
                                                                                  int count, const lm::Params prm, glim_amd_align_trace_entry* __restrict__ trace, int round,
                                                                                  int rounds) {
  const int p = (int)(blockIdx.x * VGICP_DECIDE_THREADS + threadIdx.x);
  if (p >= count) return;
  if (states[p].status != lm::RUNNING) return;
  double rec[COMPACT];
  for (int t = 0; t < COMPACT; t++) rec[t] = records[(size_t)p * COMPACT + t];
  lm::State s;
  decide_problem(prm, states + p, s, rec, trace ? trace + ((size_t)p * rounds + round) : nullptr);
  for (int k = 0; k < 12; k++) poses[12 * (size_t)p + k] = s.cand[k];
}

// ---- the scan-to-keyframes VGICP registration: one pose per problem, M factors with fixed target poses (keyframe_lm_step.hpp) ----
static_assert(keyframe_lm::MAX_TARGETS == GLIM_AMD_KEYFRAME_ALIGN_MAX_TARGETS, "the cap");
constexpr int KEYFRAME_THREADS = 64;
static_assert(keyframe_lm::MAX_TARGETS <= KEYFRAME_THREADS && lm::RECORD <= KEYFRAME_THREADS, "a lane per factor, a lane per entry of the record");

struct KeyframeProblem {
  int first, M;  // the problem's factors: first .. first + M of the batch
  int prior;     // its prior in the table of priors, or -1
};
struct KeyframeTrace {  // device arrays of the diag entry, or all null
  glim_amd_align_trace_entry* rounds;
  double *prior, *Tf, *rec;
};

// T_f of the initial poses, where round 0 evaluates the factors: one wavefront per problem, a lane per factor
__global__ __launch_bounds__(KEYFRAME_THREADS) void keyframe_pose_kernel(const KeyframeProblem* __restrict__ table, const double* __restrict__ Pinv,
                                                                         const lm::State* __restrict__ states, double* __restrict__ poses) {
  const KeyframeProblem g = table[blockIdx.x];
  const int f = threadIdx.x;
  if (f < g.M) keyframe_lm::factor_pose(Pinv + 12 * (size_t)(g.first + f), states[blockIdx.x].cand, poses + 12 * (size_t)(g.first + f));
}

// One wavefront per problem: keyframe_lm::step across the lanes.  The prior's contribution in one lane; lane t < 29 takes entry t of the
// summed record, walking the problem's M records in ascending order; lane 0 runs the step rule on the sum in LDS; lane f < M then writes the
// pose factor f is evaluated at next, or, when the problem has stopped, the status word that gates the factor's blocks.  F = all factors of
// the batch (the stride of a round in the trace).  The sequence is keyframe_lm::step's, statement for statement (the g++ test runs that one;
// tests/test_keyframe_align_gpu.py holds this one to the same restatement): a change to either is a change to both.
__global__ __launch_bounds__(KEYFRAME_THREADS) void keyframe_decide_kernel(const KeyframeProblem* __restrict__ table, const double* __restrict__ Pinv,
                                                                           const double* __restrict__ priors, const double* __restrict__ records,
                                                                           double* __restrict__ poses, lm::State* __restrict__ states, int* __restrict__ factor_status,
                                                                           double* __restrict__ kept, int F, const lm::Params prm, const KeyframeTrace tr, int round,
                                                                           int rounds) {
  __shared__ double s_rec[lm::RECORD];
  __shared__ double s_prior[keyframe_lm::PRIOR];
  __shared__ lm::State s_state;
  __shared__ int s_bad;
  const int p = blockIdx.x, t = threadIdx.x;
  if (states[p].status != lm::RUNNING) return;  // the same for every lane
  const KeyframeProblem g = table[p];
  const double* recs = records + (size_t)lm::RECORD * g.first;
  double* Tf = poses + 12 * (size_t)g.first;
  if (t == 0) s_bad = 0;
  if (t < keyframe_lm::PRIOR) s_prior[t] = 0.0;
  __syncthreads();
  if (t == 0 && g.prior >= 0) keyframe_lm::prior_contribution(priors + (size_t)keyframe_lm::PRIOR_TERM * g.prior, states[p].cand, s_prior);
  if (t < g.M && !lm::all_finite(Tf + 12 * t, 12)) s_bad = 1;
  __syncthreads();
  if (t < lm::RECORD) {
    const double v = keyframe_lm::sum_entry(recs, g.M, t);
    s_rec[t] = g.prior >= 0 ? keyframe_lm::add_prior(v, s_prior, t) : v;
  }
  if (tr.rounds) {
    const size_t at = (size_t)round * F + g.first;
    for (int u = t; u < 12 * g.M; u += KEYFRAME_THREADS) tr.Tf[12 * at + u] = Tf[u];
    for (int u = t; u < lm::RECORD * g.M; u += KEYFRAME_THREADS) tr.rec[lm::RECORD * at + u] = recs[u];
    if (t < keyframe_lm::PRIOR) tr.prior[((size_t)p * rounds + round) * keyframe_lm::PRIOR + t] = s_prior[t];
  }
  __syncthreads();
  if (t == 0) {
    glim_amd_align_trace_entry* entry = tr.rounds ? tr.rounds + ((size_t)p * rounds + round) : nullptr;
    if (s_bad) {  // a T_f that is not finite: the factors' records there say nothing
      s_state = states[p];
      s_state.accepted = 0;
      s_state.status = lm::NUMERIC;
      states[p] = s_state;
      if (entry) {
        glim_amd_align_trace_entry e;
        for (int k = 0; k < 12; k++) e.T_candidate[k] = s_state.cand[k];
        e.lambda = s_state.lambda;
        for (int k = 0; k < COMPACT; k++) e.compact[k] = s_rec[k];
        e.accepted = 0;
        e.status = lm::NUMERIC;
        *entry = e;
      }
    } else {
      decide_problem(prm, states + p, s_state, s_rec, entry);
    }
  }
  __syncthreads();
  if (s_state.accepted)  // the records of what is kept: factor_compact_out
    for (int u = t; u < lm::RECORD * g.M; u += KEYFRAME_THREADS) kept[(size_t)lm::RECORD * g.first + u] = recs[u];
  if (t < g.M) {
    if (s_state.status == lm::RUNNING) keyframe_lm::factor_pose(Pinv + 12 * (size_t)(g.first + t), s_state.cand, Tf + 12 * t);
    else factor_status[g.first + t] = s_state.status;
  }
}

// the batch over voxel-map targets: a round is vgicp.hip's evaluation of the batch's transient plan (vgicp_batch.hpp: the row kernels of both
// plan segments, one finalising block per problem) and the decide kernel above.  trace: count * (1 + max_trials) entries, or null
int run_vgicp_align(const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const double* T_init12, uint32_t flags, int32_t count,
                    const glim_amd_lm_params* params, glim_amd_align_result* out, glim_amd_align_trace_entry* trace_host) {
  if (count < 0) return GLIM_AMD_ERR_INVALID;
  if (count == 0) return GLIM_AMD_OK;
  if (!targets || !sources || !T_init12 || !out) return GLIM_AMD_ERR_INVALID;
  if (flags & ~(uint32_t)GLIM_AMD_FACTOR_SURFACE_VALIDATION) return GLIM_AMD_ERR_INVALID;  // GLIM_AMD_FACTOR_BINARY: the target is fixed
  lm::Params prm;
  int rounds;
  GA_TRY(resolve_params(params, lm_default_params, &prm, &rounds));
  glim_amd_ctx* ctx = one_context(targets, sources, count, nullptr);
  if (!ctx) return GLIM_AMD_ERR_INVALID;
  GA_TRY(vgicp_pairs_ok(targets, sources, count));
  std::vector<lm::State> states((size_t)count);
  for (int i = 0; i < count; i++) lm::init(prm, T_init12 + 12 * (size_t)i, states[(size_t)i]);

  std::unique_lock<std::mutex> held(ctx->mu);  // once for the batch
  GA_HIP(hipSetDevice(ctx->device));
  VgicpBatch batch;  // (destroyed last: its plan goes back after the stream has been waited for)
  DeviceTemp d_states;
  TraceBuffer trace;
  GA_TRY(vgicp_batch_open(ctx, targets, sources, flags, count, &batch));
  hipStream_t st = batch.stream();
  SyncOnExit in_flight(st);  // an error exit after the launches waits for the stream before the scratch goes back to the pool
  GA_HIP(pool_malloc(&d_states.p, states.size() * sizeof(lm::State)));
  GA_TRY(trace.open(trace_host, (size_t)count * rounds * sizeof(glim_amd_align_trace_entry), st));
  GA_HIP(hipMemcpyAsync(d_states.p, states.data(), states.size() * sizeof(lm::State), hipMemcpyHostToDevice, st));
  GA_HIP(hipMemcpyAsync(batch.poses(), T_init12, (size_t)count * 12 * sizeof(double), hipMemcpyHostToDevice, st));
  static_assert(sizeof(lm::State) % sizeof(int) == 0 && offsetof(lm::State, status) % sizeof(int) == 0, "the status word of a state, in ints");
  const int* d_status = reinterpret_cast<const int*>(d_states.as<char>() + offsetof(lm::State, status));
  const int stride = (int)(sizeof(lm::State) / sizeof(int));
  const int decide_blocks = (count + VGICP_DECIDE_THREADS - 1) / VGICP_DECIDE_THREADS;
  for (int r = 0; r < rounds; r++) {
    GA_TRY(vgicp_batch_round(&batch, d_status, stride));
    vgicp_align_decide_kernel<<<decide_blocks, VGICP_DECIDE_THREADS, 0, st>>>(batch.records(), batch.poses(), d_states.as<lm::State>(), count, prm,
                                                                             trace.d.as<glim_amd_align_trace_entry>(), r, rounds);
  }
  GA_HIP(hipGetLastError());
  GA_HIP(hipMemcpyAsync(states.data(), d_states.p, states.size() * sizeof(lm::State), hipMemcpyDeviceToHost, st));
  GA_TRY(trace.fetch(st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  batch.seen_complete();
  for (int i = 0; i < count; i++) align_result(states[(size_t)i], out + i);
  return GLIM_AMD_OK;
}

// The scan-to-keyframes registration: problem i has the factors first_target[i] .. first_target[i + 1] of ONE batch over all F pairs (a source
// appears once per target of its problem).  A round is vgicp_batch_round, every factor behind a status word of its own (F ints, zero while
// the factor's problem runs), and the keyframe decide kernel, which leaves the next round's T_f in the batch's pose buffer.  trace: the four
// arrays of the diag entry, or all null.
int run_keyframe_align(const glim_amd_cloud* const* sources, const int32_t* first_target, const glim_amd_voxelmap* const* targets, const double* T_world_target12,
                       const double* X_init12, const glim_amd_bundle_prior* priors, int32_t P, uint32_t flags, int32_t count, const glim_amd_lm_params* params,
                       glim_amd_align_result* out, double* factor_compact_out, const KeyframeTrace& trace_host) {
  if (count < 0 || P < 0) return GLIM_AMD_ERR_INVALID;
  if (count == 0) return GLIM_AMD_OK;
  if (!sources || !first_target || !targets || !T_world_target12 || !X_init12 || !out || (P > 0 && !priors)) return GLIM_AMD_ERR_INVALID;
  if (flags & ~(uint32_t)GLIM_AMD_FACTOR_SURFACE_VALIDATION) return GLIM_AMD_ERR_INVALID;  // GLIM_AMD_FACTOR_BINARY: the targets are fixed
  lm::Params prm;
  int rounds;
  GA_TRY(resolve_params(params, lm_default_params, &prm, &rounds));
  if (first_target[0] != 0) return GLIM_AMD_ERR_INVALID;
  for (int i = 0; i < count; i++)
    if (first_target[i + 1] <= first_target[i]) return GLIM_AMD_ERR_INVALID;  // descending, or a problem with no target
  for (int i = 0; i < count; i++)
    if (first_target[i + 1] - first_target[i] > keyframe_lm::MAX_TARGETS) return GLIM_AMD_ERR_UNSUPPORTED;
  const int F = first_target[count];
  std::vector<const glim_amd_cloud*> pair_sources((size_t)F);
  std::vector<KeyframeProblem> table((size_t)count);
  for (int i = 0; i < count; i++) {
    table[(size_t)i] = KeyframeProblem{first_target[i], first_target[i + 1] - first_target[i], -1};
    for (int f = first_target[i]; f < first_target[i + 1]; f++) pair_sources[(size_t)f] = sources[i];
  }
  std::vector<double> terms((size_t)keyframe_lm::PRIOR_TERM * P);
  for (int q = 0; q < P; q++) {
    const glim_amd_bundle_prior& pr = priors[q];
    if (pr.pose < 0 || pr.pose >= count || table[(size_t)pr.pose].prior >= 0) return GLIM_AMD_ERR_INVALID;
    if (!all_finite_host(pr.T, 12) || !all_finite_host(pr.information, 36)) return GLIM_AMD_ERR_INVALID;
    table[(size_t)pr.pose].prior = q;
    memcpy(&terms[(size_t)keyframe_lm::PRIOR_TERM * q], pr.T, 12 * sizeof(double));
    memcpy(&terms[(size_t)keyframe_lm::PRIOR_TERM * q + 12], pr.information, 36 * sizeof(double));
  }
  glim_amd_ctx* ctx = one_context(targets, pair_sources.data(), F, nullptr);
  if (!ctx) return GLIM_AMD_ERR_INVALID;
  GA_TRY(vgicp_pairs_ok(targets, pair_sources.data(), F));
  std::vector<lm::State> states((size_t)count);
  std::vector<double> Pinv(12 * (size_t)F);
  for (int i = 0; i < count; i++) lm::init(prm, X_init12 + 12 * (size_t)i, states[(size_t)i]);
  for (int f = 0; f < F; f++) keyframe_lm::target_inverse(T_world_target12 + 12 * (size_t)f, &Pinv[12 * (size_t)f]);

  std::unique_lock<std::mutex> held(ctx->mu);  // once for the batch
  GA_HIP(hipSetDevice(ctx->device));
  VgicpBatch batch;  // (destroyed last: its plan goes back after the stream has been waited for)
  DeviceTemp d_states, d_table, d_Pinv, d_terms, d_status, d_kept;
  TraceBuffer trounds, tprior, tTf, trec;
  GA_TRY(vgicp_batch_open(ctx, targets, pair_sources.data(), flags, F, &batch));
  hipStream_t st = batch.stream();
  SyncOnExit in_flight(st);  // an error exit after the launches waits for the stream before the scratch goes back to the pool
  const size_t kept_bytes = (size_t)F * lm::RECORD * sizeof(double);
  GA_HIP(pool_malloc(&d_states.p, states.size() * sizeof(lm::State)));
  GA_HIP(pool_malloc(&d_table.p, table.size() * sizeof(KeyframeProblem)));
  GA_HIP(pool_malloc(&d_Pinv.p, Pinv.size() * sizeof(double)));
  GA_HIP(pool_malloc(&d_terms.p, std::max<size_t>(8, terms.size() * sizeof(double))));
  GA_HIP(pool_malloc(&d_status.p, (size_t)F * sizeof(int)));
  GA_HIP(pool_malloc(&d_kept.p, kept_bytes));
  // (the entry point has seen to it that the four arrays come together; an array the caller did not give opens nothing)
  GA_TRY(trounds.open(trace_host.rounds, (size_t)count * rounds * sizeof(glim_amd_align_trace_entry), st));
  GA_TRY(tprior.open(trace_host.prior, (size_t)count * rounds * keyframe_lm::PRIOR * sizeof(double), st));
  GA_TRY(tTf.open(trace_host.Tf, (size_t)rounds * F * 12 * sizeof(double), st));
  GA_TRY(trec.open(trace_host.rec, (size_t)rounds * F * lm::RECORD * sizeof(double), st));
  const KeyframeTrace tr{trounds.d.as<glim_amd_align_trace_entry>(), tprior.d.as<double>(), tTf.d.as<double>(), trec.d.as<double>()};
  GA_HIP(hipMemcpyAsync(d_states.p, states.data(), states.size() * sizeof(lm::State), hipMemcpyHostToDevice, st));
  GA_HIP(hipMemcpyAsync(d_table.p, table.data(), table.size() * sizeof(KeyframeProblem), hipMemcpyHostToDevice, st));
  GA_HIP(hipMemcpyAsync(d_Pinv.p, Pinv.data(), Pinv.size() * sizeof(double), hipMemcpyHostToDevice, st));
  if (P > 0) GA_HIP(hipMemcpyAsync(d_terms.p, terms.data(), terms.size() * sizeof(double), hipMemcpyHostToDevice, st));
  GA_HIP(hipMemsetAsync(d_status.p, 0, (size_t)F * sizeof(int), st));
  GA_HIP(hipMemsetAsync(d_kept.p, 0, kept_bytes, st));
  keyframe_pose_kernel<<<count, KEYFRAME_THREADS, 0, st>>>(d_table.as<KeyframeProblem>(), d_Pinv.as<double>(), d_states.as<lm::State>(), batch.poses());
  for (int r = 0; r < rounds; r++) {
    GA_TRY(vgicp_batch_round(&batch, d_status.as<int>(), 1));
    keyframe_decide_kernel<<<count, KEYFRAME_THREADS, 0, st>>>(d_table.as<KeyframeProblem>(), d_Pinv.as<double>(), d_terms.as<double>(), batch.records(), batch.poses(),
                                                               d_states.as<lm::State>(), d_status.as<int>(), d_kept.as<double>(), F, prm, tr, r, rounds);
  }
  GA_HIP(hipGetLastError());
  std::vector<double> kept_host(factor_compact_out ? (size_t)F * lm::RECORD : 0);
  GA_HIP(hipMemcpyAsync(states.data(), d_states.p, states.size() * sizeof(lm::State), hipMemcpyDeviceToHost, st));
  if (factor_compact_out) GA_HIP(hipMemcpyAsync(kept_host.data(), d_kept.p, kept_bytes, hipMemcpyDeviceToHost, st));
  for (TraceBuffer* t : {&trounds, &tprior, &tTf, &trec}) GA_TRY(t->fetch(st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  batch.seen_complete();
  if (factor_compact_out) memcpy(factor_compact_out, kept_host.data(), kept_bytes);
  for (int i = 0; i < count; i++) align_result(states[(size_t)i], out + i);
  return GLIM_AMD_OK;
}

}  // namespace

extern "C" {

int glim_amd_vgicp_align_default_params(glim_amd_lm_params* params) { return default_params_out(params, lm_default_params); }

int glim_amd_vgicp_align_batch(const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const double* T_init12, uint32_t flags, int32_t count,
                               const glim_amd_lm_params* params, glim_amd_align_result* out) {
  return run_vgicp_align(targets, sources, T_init12, flags, count, params, out, nullptr);
}

int glim_amd_debug_vgicp_align_trace(const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const double* T_init12, uint32_t flags, int32_t count,
                                     const glim_amd_lm_params* params, glim_amd_align_result* out, glim_amd_align_trace_entry* trace) {
  if (!trace && count > 0) return GLIM_AMD_ERR_INVALID;
  return run_vgicp_align(targets, sources, T_init12, flags, count, params, out, trace);
}

int glim_amd_keyframe_align_default_params(glim_amd_lm_params* params) { return default_params_out(params, lm_default_params); }

int glim_amd_keyframe_align_batch(const glim_amd_cloud* const* sources, const int32_t* first_target, const glim_amd_voxelmap* const* targets,
                                  const double* T_world_target12, const double* X_init12, const glim_amd_bundle_prior* priors, int32_t num_priors, uint32_t flags,
                                  int32_t count, const glim_amd_lm_params* params, glim_amd_align_result* out, double* factor_compact_out) {
  return run_keyframe_align(sources, first_target, targets, T_world_target12, X_init12, priors, num_priors, flags, count, params, out, factor_compact_out,
                            KeyframeTrace{nullptr, nullptr, nullptr, nullptr});
}

int glim_amd_debug_keyframe_align_trace(const glim_amd_cloud* const* sources, const int32_t* first_target, const glim_amd_voxelmap* const* targets,
                                        const double* T_world_target12, const double* X_init12, const glim_amd_bundle_prior* priors, int32_t num_priors, uint32_t flags,
                                        int32_t count, const glim_amd_lm_params* params, glim_amd_align_result* out, double* factor_compact_out,
                                        glim_amd_align_trace_entry* rounds, double* prior_trace, double* Tf_trace, double* compact_trace) {
  if (count > 0 && (!rounds || !prior_trace || !Tf_trace || !compact_trace)) return GLIM_AMD_ERR_INVALID;
  return run_keyframe_align(sources, first_target, targets, T_world_target12, X_init12, priors, num_priors, flags, count, params, out, factor_compact_out,
                            KeyframeTrace{rounds, prior_trace, Tf_trace, compact_trace});
}

}  // extern "C"
