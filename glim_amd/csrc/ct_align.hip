// ct_align.hip -- the CT frame alignment on gfx950 (include/glim_amd.h "CT-GICP frame alignment"): the scheme of gicp_align.hip over ONE
// continuous-time factor and two poses, on the host scaffold of align_host.hpp.  A round is the pose table kernel (T_k | D0_k | D1_k of every bucket from the candidate pair,
// ct_se3.hpp), the factor's search pass and bucket pass over the blocks and buffers the factor already has (ct_factor.hpp: the bodies
// glim_amd_ct_gicp_linearize runs), and the CT decide kernel: the ordered sum of the bucket rows, the two terms and the step rule of
// ct_lm_step.hpp.  All 1 + max_trials rounds are enqueued up front: ONE synchronisation.
//
// The test window of ct_se3.hpp (glim_amd_debug_se3_eval) is here too: this unit evaluates that header.
#include "align_host.hpp"
#include "ct_factor.hpp"
#include "ct_lm_step.hpp"

namespace {

static_assert(sizeof(ct_lm::Terms) == sizeof(glim_amd_ct_align_terms), "ct_lm::Terms is the layout of glim_amd_ct_align_terms");
static_assert(offsetof(ct_lm::Terms, kb) == offsetof(glim_amd_ct_align_terms, between_precision), "ct_lm::Terms is the layout of glim_amd_ct_align_terms");
static_assert(ct_lm::RECORD == CT_ROW, "the record of the continuous-time factor");
static_assert(sizeof(ct_lm::State) % sizeof(double) == 0, "the state is copied in 8-byte words");
constexpr int CT_STATE_WORDS = (int)(sizeof(ct_lm::State) / sizeof(double));
constexpr int CT_POSE_THREADS = 128;

// one block: the bucket pose table at the candidate pair.  Thread 0 runs what the buckets share (Log(X^-1 Y), J_r^-1, -Ad) into LDS, then the
// buckets go across the threads
__global__ __launch_bounds__(CT_POSE_THREADS) void ct_align_poses_kernel(const ct_lm::State* __restrict__ state, const double* __restrict__ table, int nbk,
                                                                         double* __restrict__ poses) {
  __shared__ ct_se3::CtPoseShared s_shared;
  __shared__ double s_X[12];
  if (state->status != lm::RUNNING) return;  // the same for every thread of the block
  if (threadIdx.x == 0) {
    double X[12], Y[12];
#pragma unroll
    for (int k = 0; k < 12; k++) {
      X[k] = state->candX[k];
      Y[k] = state->candY[k];
      s_X[k] = X[k];
    }
    ct_se3::ct_pose_shared(X, Y, s_shared);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nbk; k += CT_POSE_THREADS) ct_se3::ct_pose_bucket(s_X, s_shared, table[k], poses + (size_t)k * CT_POSE_STRIDE);
}

// the test window of ct_se3.hpp (glim_amd_debug_se3_eval): one thread per case runs ct_se3::se3_eval on its own slice and nothing else
constexpr int SE3_EVAL_THREADS = 64;
__global__ __launch_bounds__(SE3_EVAL_THREADS) void se3_eval_kernel(int op, int count, const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * SE3_EVAL_THREADS + threadIdx.x;
  if (i >= count) return;
  ct_se3::se3_eval(op, in + (size_t)i * ct_se3::se3_eval_in(op), out + (size_t)i * ct_se3::se3_eval_out(op));
}

// ct_gicp_kernel<true> and ct_bucket_kernel behind the status check (no keep_* pointers: what the factor keeps for error() stays as it was)
template <class NN>
__global__ __launch_bounds__(BLOCK) void ct_align_linearize_kernel(const GicpArgs a, const CtArgs c, const ct_lm::State* __restrict__ state,
                                                                   float* __restrict__ partials, const NN nn) {
  __shared__ float s_red[4][PARTIAL_STRIDE];
  if (state->status != lm::RUNNING) return;  // the same for every thread of the block
  ct_gicp_block<true, NN>(a, c, partials, nn, s_red);
}

__global__ __launch_bounds__(64) void ct_align_bucket_kernel(const float* __restrict__ partials, const int* __restrict__ bucket_first, const double* __restrict__ poses,
                                                             const ct_lm::State* __restrict__ state, double* __restrict__ rows) {
  __shared__ CtBucketShared s;
  if (state->status != lm::RUNNING) return;  // the same for every thread of the block
  ct_bucket_block(partials, bucket_first, poses, rows, s);
}

// one block: ct_sum_kernel's sum of the bucket rows into LDS (the same additions in three passes of 256 threads), then the terms and the step
// rule in thread 0 on the state in LDS.  The 12 x 12 system, the Cholesky factor and the state are LDS arrays, indexed freely without a
// per-thread copy; 256 threads leave thread 0 the whole register file, so the unrolled SE(3) algebra of the terms does not spill.
constexpr int CT_DECIDE_THREADS = 256;
__global__ __launch_bounds__(CT_DECIDE_THREADS) void ct_align_decide_kernel(const double* __restrict__ rows, int nbk, ct_lm::State* __restrict__ state,
                                                                         const ct_lm::Terms terms, const lm::Params prm,
                                                                         glim_amd_ct_align_trace_entry* __restrict__ trace, int round) {
  __shared__ double s_part[8][96];
  __shared__ double s_rec[96];
  __shared__ double s_work[ct_lm::WORK];
  __shared__ double s_before[25];  // the candidate pair and its lambda, for the trace
  __shared__ ct_lm::State s_state;
  __shared__ ct_lm::Terms s_terms;
  if (state->status != lm::RUNNING) return;  // the same for every thread of the block
  const int t = threadIdx.x;
  if (t == 0) s_terms = terms;
  double* words = reinterpret_cast<double*>(&s_state);
  const double* in = reinterpret_cast<const double*>(state);
  for (int u = t; u < CT_STATE_WORDS; u += CT_DECIDE_THREADS) words[u] = in[u];
  ct_sum_rows<CT_DECIDE_THREADS>(rows, nbk, s_part, s_rec);
  __syncthreads();
  if (t < 12) s_before[t] = s_state.candX[t];
  else if (t < 24) s_before[t] = s_state.candY[t - 12];
  else if (t == 24) s_before[24] = s_state.lambda;
  else if (t == 25) s_work[1] = 0.0;  // the traced cost of a round that ends before its system is assembled
  __syncthreads();
  if (t == 0) ct_lm::step(prm, s_terms, s_state, s_rec, s_work);
  __syncthreads();
  double* outw = reinterpret_cast<double*>(state);
  for (int u = t; u < CT_STATE_WORDS; u += CT_DECIDE_THREADS) outw[u] = words[u];
  if (trace) {
    glim_amd_ct_align_trace_entry& e = trace[round];
    if (t < 12) e.X[t] = s_before[t];
    else if (t < 24) e.Y[t - 12] = s_before[t];
    else if (t == 24) e.lambda = s_before[24];
    else if (t == 25) e.cost = s_work[1];
    else if (t == 26) e.accepted = s_state.accepted;
    else if (t == 27) e.status = s_state.status;
    if (t >= 32 && t < 32 + CT_ROW) e.record[t - 32] = s_rec[t - 32];
  }
}

void ct_default_params(glim_amd_lm_params* p) {
  lm_default_params(p);
  p->lambda_initial = 1e-10, p->absolute_error_tol = 1e-2, p->max_iterations = 8;
}

// the launches of one evaluation of the factor at the state's candidate pair
void launch_ct_round(const GicpTarget& t, const glim_amd_ct_gicp_factor* f, const GicpArgs& a, const CtArgs& c, const ct_lm::State* d_state, hipStream_t st) {
  ct_align_poses_kernel<<<1, CT_POSE_THREADS, 0, st>>>(d_state, f->d_table, f->nbk, f->d_poses);
  with_search(t, [&](auto nn) { ct_align_linearize_kernel<decltype(nn)><<<f->nb, BLOCK, 0, st>>>(a, c, d_state, f->d_partials, nn); });
  ct_align_bucket_kernel<<<f->nbk, 64, 0, st>>>(f->d_partials, f->d_bucket_first, f->d_poses, d_state, f->d_rows);
}

// trace_host: 1 + max_trials entries, or null
int run_ct_align(glim_amd_ct_gicp_factor* f, const double* X_init, const double* Y_init, const glim_amd_ct_align_terms* terms, const glim_amd_lm_params* params,
                 glim_amd_ct_align_result* out, glim_amd_ct_align_trace_entry* trace_host) {
  if (!f || !X_init || !Y_init || !out) return GLIM_AMD_ERR_INVALID;
  ct_lm::Terms tm;
  memset(&tm, 0, sizeof(tm));
  if (terms) memcpy(&tm, terms, sizeof(tm));
  if (!(tm.kp >= 0.0) || !(tm.kb >= 0.0) || !std::isfinite(tm.kp) || !std::isfinite(tm.kb)) return GLIM_AMD_ERR_INVALID;
  if ((tm.kp > 0.0 && !all_finite_host(tm.P, 12)) || (tm.kb > 0.0 && !all_finite_host(tm.D, 12))) return GLIM_AMD_ERR_INVALID;
  lm::Params prm;
  int rounds;
  GA_TRY(resolve_params(params, ct_default_params, &prm, &rounds));

  const GicpTarget t = ct_target(f);  // holds the context's lock for the whole call
  if (!f->src->has_covs || !t.usable) return GLIM_AMD_ERR_STATE;
  if (f->n == 0 || t.empty) return GLIM_AMD_ERR_INVALID;
  GicpArgs a = t.args;
  set_source(&a, f->src, 1, f->max_dist);
  a.max_ring = t.rings(f->max_dist);
  if (a.max_ring < 0) return GLIM_AMD_ERR_UNSUPPORTED;
  CtArgs c{};
  c.blocks = f->d_blocks;
  c.poses = f->d_poses;
  ct_lm::State state;
  memset(&state, 0, sizeof(state));
  ct_lm::init(prm, X_init, Y_init, state);

  glim_amd_ctx* ctx = f->ctx;
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  DeviceTemp d_state;
  TraceBuffer trace;
  SyncOnExit in_flight(st);  // an error exit after the launches waits for the stream before the scratch goes back to the pool
  GA_HIP(pool_malloc(&d_state.p, sizeof(ct_lm::State)));
  GA_TRY(trace.open(trace_host, (size_t)rounds * sizeof(glim_amd_ct_align_trace_entry), st));
  GA_HIP(hipMemcpyAsync(d_state.p, &state, sizeof(state), hipMemcpyHostToDevice, st));
  for (int r = 0; r < rounds; r++) {
    launch_ct_round(t, f, a, c, d_state.as<ct_lm::State>(), st);
    ct_align_decide_kernel<<<1, CT_DECIDE_THREADS, 0, st>>>(f->d_rows, f->nbk, d_state.as<ct_lm::State>(), tm, prm, trace.d.as<glim_amd_ct_align_trace_entry>(), r);
  }
  GA_HIP(hipGetLastError());
  GA_HIP(hipMemcpyAsync(&state, d_state.p, sizeof(state), hipMemcpyDeviceToHost, st));
  GA_TRY(trace.fetch(st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  memset(out, 0, sizeof(*out));
  memcpy(out->X, state.X, sizeof(out->X));
  memcpy(out->Y, state.Y, sizeof(out->Y));
  ct_expand_record(state.rec, &out->linearized);
  out->cost = state.sys[1], out->location_cost = state.cost_p, out->between_cost = state.cost_b;
  out->lambda = state.lambda, out->iterations = state.iterations, out->trials = state.trials, out->status = state.status;
  return GLIM_AMD_OK;
}

}  // namespace

extern "C" {

int glim_amd_ct_align_default_params(glim_amd_lm_params* params) { return default_params_out(params, ct_default_params); }

int glim_amd_ct_align(glim_amd_ct_gicp_factor* factor, const double* X_init12, const double* Y_init12, const glim_amd_ct_align_terms* terms,
                      const glim_amd_lm_params* params, glim_amd_ct_align_result* out) {
  return run_ct_align(factor, X_init12, Y_init12, terms, params, out, nullptr);
}

int glim_amd_debug_ct_align_trace(glim_amd_ct_gicp_factor* factor, const double* X_init12, const double* Y_init12, const glim_amd_ct_align_terms* terms,
                                  const glim_amd_lm_params* params, glim_amd_ct_align_result* out, glim_amd_ct_align_trace_entry* trace) {
  if (!trace) return GLIM_AMD_ERR_INVALID;
  return run_ct_align(factor, X_init12, Y_init12, terms, params, out, trace);
}

int glim_amd_debug_ct_align_poses(glim_amd_ct_gicp_factor* f, const double* X12, const double* Y12, int32_t* num_buckets, int32_t table_cap, double* T12_out,
                                  double* D0_out, double* D1_out) {
  if (!f || !X12 || !Y12 || table_cap < 0) return GLIM_AMD_ERR_INVALID;
  if (num_buckets) *num_buckets = f->nbk;
  const int m = std::min(table_cap, f->nbk);
  if (m == 0) return GLIM_AMD_OK;
  lm::Params prm;
  memset(&prm, 0, sizeof(prm));
  ct_lm::State state;
  memset(&state, 0, sizeof(state));
  ct_lm::init(prm, X12, Y12, state);
  glim_amd_ctx* ctx = f->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  DeviceTemp d_state;
  std::vector<double> full((size_t)f->nbk * CT_POSE_STRIDE);
  SyncOnExit in_flight(st);
  GA_HIP(pool_malloc(&d_state.p, sizeof(ct_lm::State)));
  GA_HIP(hipMemcpyAsync(d_state.p, &state, sizeof(state), hipMemcpyHostToDevice, st));
  ct_align_poses_kernel<<<1, CT_POSE_THREADS, 0, st>>>(d_state.as<ct_lm::State>(), f->d_table, f->nbk, f->d_poses);
  GA_HIP(hipGetLastError());
  GA_HIP(hipMemcpyAsync(full.data(), f->d_poses, full.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  for (int k = 0; k < m; k++) {
    const double* o = full.data() + (size_t)k * CT_POSE_STRIDE;
    if (T12_out) memcpy(T12_out + 12 * (size_t)k, o, 12 * sizeof(double));
    if (D0_out) memcpy(D0_out + 36 * (size_t)k, o + 12, 36 * sizeof(double));
    if (D1_out) memcpy(D1_out + 36 * (size_t)k, o + 48, 36 * sizeof(double));
  }
  return GLIM_AMD_OK;
}

int glim_amd_debug_se3_eval(glim_amd_ctx* ctx, int32_t op, int32_t count, const double* in, double* out) {
  if (!ctx || !in || !out || count < 0 || op < 0 || op >= ct_se3::SE3_EVAL_OPS) return GLIM_AMD_ERR_INVALID;
  if (count == 0) return GLIM_AMD_OK;
  const size_t ni = (size_t)count * ct_se3::se3_eval_in(op), no = (size_t)count * ct_se3::se3_eval_out(op);
  std::unique_lock<std::mutex> held(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  DeviceTemp d;  // the inputs, then the outputs
  SyncOnExit in_flight(st);
  GA_HIP(pool_malloc(&d.p, (ni + no) * sizeof(double)));
  double *d_in = d.as<double>(), *d_out = d_in + ni;
  GA_HIP(hipMemcpyAsync(d_in, in, ni * sizeof(double), hipMemcpyHostToDevice, st));
  se3_eval_kernel<<<(count + SE3_EVAL_THREADS - 1) / SE3_EVAL_THREADS, SE3_EVAL_THREADS, 0, st>>>(op, count, d_in, d_out);
  GA_HIP(hipGetLastError());
  GA_HIP(hipMemcpyAsync(out, d_out, no * sizeof(double), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  return GLIM_AMD_OK;
}

}  // extern "C"
