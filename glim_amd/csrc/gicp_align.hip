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
//
// The VGICP fine registration (include/glim_amd.h "VGICP fine registration") is the same scheme over voxel-map targets.  The factor's hot loop,
// its plan and its ordered sum live in vgicp.hip and stay there: a round is vgicp_batch_round (vgicp_batch.hpp: vgicp.hip's row kernels and
// finalising blocks behind the status check, over a transient plan of the batch's pairs, leaving finished compact records on the device) and
// vgicp_align_decide_kernel here, which runs the step rule on those records and writes each problem's next candidate into the plan's pose
// buffer.  The step rule is included by this file alone.
//
// The CT frame alignment (include/glim_amd.h "CT-GICP frame alignment") is the same scheme over ONE continuous-time factor and two poses: a round
// is the pose table kernel (T_k | D0_k | D1_k of every bucket from the candidate pair, ct_se3.hpp), the factor's search pass and bucket pass over
// the blocks and buffers the factor already has (ct_factor.hpp: the bodies glim_amd_ct_gicp_linearize runs), and the CT decide kernel: the
// ordered sum of the bucket rows, the two terms and the step rule of ct_lm_step.hpp.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <mutex>
#include <vector>

#include "ct_factor.hpp"
#include "ct_lm_step.hpp"
#include "device_math.hpp"
#include "gicp_factor.hpp"
#include "internal.hpp"
#include "ivox_map.hpp"
#include "lm_step.hpp"
#include "scope_sync.hpp"
#include "vgicp_batch.hpp"

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
  lm::State s = states[p];
  glim_amd_align_trace_entry e;
  for (int k = 0; k < 12; k++) e.T_candidate[k] = s.cand[k];
  e.lambda = s.lambda;
  lm::step(prm, s, rec);
  states[p] = s;
  for (int k = 0; k < 12; k++) poses[12 * (size_t)p + k] = s.cand[k];
  if (trace) {
    for (int t = 0; t < COMPACT; t++) e.compact[t] = rec[t];
    e.accepted = s.accepted;
    e.status = s.status;
    trace[(size_t)p * rounds + round] = e;
  }
}

// ---- the CT frame alignment ----
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

void ct_default_params(glim_amd_lm_params* p) {
  lm_default_params(p);
  p->lambda_initial = 1e-10;
  p->absolute_error_tol = 1e-2;
  p->max_iterations = 8;
}

bool pose_finite(const double* T) {
  for (int k = 0; k < 12; k++)
    if (!std::isfinite(T[k])) return false;
  return true;
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
  if ((tm.kp > 0.0 && !pose_finite(tm.P)) || (tm.kb > 0.0 && !pose_finite(tm.D))) return GLIM_AMD_ERR_INVALID;
  glim_amd_lm_params prm_c;
  if (params) prm_c = *params;
  else ct_default_params(&prm_c);
  if (!lm_params_ok(prm_c)) return GLIM_AMD_ERR_INVALID;
  if (prm_c.max_trials == 0) prm_c.max_trials = 2 * prm_c.max_iterations;
  if (prm_c.max_trials > ALIGN_MAX_TRIALS) return GLIM_AMD_ERR_INVALID;
  lm::Params prm;
  memcpy(&prm, &prm_c, sizeof(prm));
  const int rounds = 1 + prm.max_trials;

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
  DeviceTemp d_state, d_trace;
  SyncOnExit in_flight(st);  // an error exit after the launches waits for the stream before the scratch goes back to the pool
  GA_HIP(pool_malloc(&d_state.p, sizeof(ct_lm::State)));
  const size_t trace_bytes = (size_t)rounds * sizeof(glim_amd_ct_align_trace_entry);
  if (trace_host) {
    GA_HIP(pool_malloc(&d_trace.p, trace_bytes));
    GA_HIP(hipMemsetAsync(d_trace.p, 0, trace_bytes, st));
  }
  GA_HIP(hipMemcpyAsync(d_state.p, &state, sizeof(state), hipMemcpyHostToDevice, st));
  for (int r = 0; r < rounds; r++) {
    launch_ct_round(t, f, a, c, d_state.as<ct_lm::State>(), st);
    ct_align_decide_kernel<<<1, CT_DECIDE_THREADS, 0, st>>>(f->d_rows, f->nbk, d_state.as<ct_lm::State>(), tm, prm, d_trace.as<glim_amd_ct_align_trace_entry>(), r);
  }
  GA_HIP(hipGetLastError());
  GA_HIP(hipMemcpyAsync(&state, d_state.p, sizeof(state), hipMemcpyDeviceToHost, st));
  if (trace_host) GA_HIP(hipMemcpyAsync(trace_host, d_trace.p, trace_bytes, hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  memset(out, 0, sizeof(*out));
  memcpy(out->X, state.X, sizeof(out->X));
  memcpy(out->Y, state.Y, sizeof(out->Y));
  ct_expand_record(state.rec, &out->linearized);
  out->cost = state.sys[1];
  out->location_cost = state.cost_p;
  out->between_cost = state.cost_b;
  out->lambda = state.lambda;
  out->iterations = state.iterations;
  out->trials = state.trials;
  out->status = state.status;
  return GLIM_AMD_OK;
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

// the batch over voxel-map targets: a round is vgicp.hip's evaluation of the batch's transient plan (vgicp_batch.hpp: the row kernels of both
// plan segments, one finalising block per problem) and the decide kernel above.  trace: count * (1 + max_trials) entries, or null
int run_vgicp_align(const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const double* T_init12, uint32_t flags, int32_t count,
                    const glim_amd_lm_params* params, glim_amd_align_result* out, glim_amd_align_trace_entry* trace_host) {
  if (count < 0) return GLIM_AMD_ERR_INVALID;
  if (count == 0) return GLIM_AMD_OK;
  if (!targets || !sources || !T_init12 || !out) return GLIM_AMD_ERR_INVALID;
  if (flags & ~(uint32_t)GLIM_AMD_FACTOR_SURFACE_VALIDATION) return GLIM_AMD_ERR_INVALID;  // GLIM_AMD_FACTOR_BINARY: the target is fixed
  glim_amd_lm_params prm_c;
  if (params) prm_c = *params;
  else lm_default_params(&prm_c);
  if (!lm_params_ok(prm_c)) return GLIM_AMD_ERR_INVALID;
  if (prm_c.max_trials == 0) prm_c.max_trials = 2 * prm_c.max_iterations;
  if (prm_c.max_trials > ALIGN_MAX_TRIALS) return GLIM_AMD_ERR_INVALID;
  for (int i = 0; i < count; i++)
    if (!targets[i] || !sources[i]) return GLIM_AMD_ERR_INVALID;
  glim_amd_ctx* ctx = targets[0]->ctx;
  for (int i = 0; i < count; i++)
    if ((glim_amd_ctx*)targets[i]->ctx != ctx || (glim_amd_ctx*)sources[i]->ctx != ctx) return GLIM_AMD_ERR_INVALID;
  for (int i = 0; i < count; i++) {  // what glim_amd_factor_set_add answers for the pair, then the empty source
    if (!targets[i]->buckets || !sources[i]->has_covs) return GLIM_AMD_ERR_STATE;
    if (sources[i]->n == 0 || sources[i]->n > (int64_t)(1u << 28)) return GLIM_AMD_ERR_INVALID;
  }
  lm::Params prm;
  memcpy(&prm, &prm_c, sizeof(prm));
  const int rounds = 1 + prm.max_trials;
  std::vector<lm::State> states((size_t)count);
  for (int i = 0; i < count; i++) lm::init(prm, T_init12 + 12 * (size_t)i, states[(size_t)i]);

  std::unique_lock<std::mutex> held(ctx->mu);  // once for the batch
  GA_HIP(hipSetDevice(ctx->device));
  VgicpBatch batch;  // (destroyed last: its plan goes back after the stream has been waited for)
  DeviceTemp d_states, d_trace;
  GA_TRY(vgicp_batch_open(ctx, targets, sources, flags, count, &batch));
  hipStream_t st = batch.stream();
  SyncOnExit in_flight(st);  // an error exit after the launches waits for the stream before the scratch goes back to the pool
  GA_HIP(pool_malloc(&d_states.p, states.size() * sizeof(lm::State)));
  const size_t trace_bytes = (size_t)count * rounds * sizeof(glim_amd_align_trace_entry);
  if (trace_host) {
    GA_HIP(pool_malloc(&d_trace.p, trace_bytes));
    GA_HIP(hipMemsetAsync(d_trace.p, 0, trace_bytes, st));
  }
  GA_HIP(hipMemcpyAsync(d_states.p, states.data(), states.size() * sizeof(lm::State), hipMemcpyHostToDevice, st));
  GA_HIP(hipMemcpyAsync(batch.poses(), T_init12, (size_t)count * 12 * sizeof(double), hipMemcpyHostToDevice, st));
  static_assert(sizeof(lm::State) % sizeof(int) == 0 && offsetof(lm::State, status) % sizeof(int) == 0, "the status word of a state, in ints");
  const int* d_status = reinterpret_cast<const int*>(d_states.as<char>() + offsetof(lm::State, status));
  const int stride = (int)(sizeof(lm::State) / sizeof(int));
  const int decide_blocks = (count + VGICP_DECIDE_THREADS - 1) / VGICP_DECIDE_THREADS;
  for (int r = 0; r < rounds; r++) {
    GA_TRY(vgicp_batch_round(&batch, d_status, stride));
    vgicp_align_decide_kernel<<<decide_blocks, VGICP_DECIDE_THREADS, 0, st>>>(batch.records(), batch.poses(), d_states.as<lm::State>(), count, prm,
                                                                             d_trace.as<glim_amd_align_trace_entry>(), r, rounds);
  }
  GA_HIP(hipGetLastError());
  GA_HIP(hipMemcpyAsync(states.data(), d_states.p, states.size() * sizeof(lm::State), hipMemcpyDeviceToHost, st));
  if (trace_host) GA_HIP(hipMemcpyAsync(trace_host, d_trace.p, trace_bytes, hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  batch.seen_complete();
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

int glim_amd_vgicp_align_default_params(glim_amd_lm_params* params) {
  if (!params) return GLIM_AMD_ERR_INVALID;
  lm_default_params(params);
  return GLIM_AMD_OK;
}

int glim_amd_vgicp_align_batch(const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const double* T_init12, uint32_t flags,
                               int32_t count, const glim_amd_lm_params* params, glim_amd_align_result* out) {
  return run_vgicp_align(targets, sources, T_init12, flags, count, params, out, nullptr);
}

int glim_amd_debug_vgicp_align_trace(const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const double* T_init12, uint32_t flags,
                                     int32_t count, const glim_amd_lm_params* params, glim_amd_align_result* out, glim_amd_align_trace_entry* trace) {
  if (!trace && count > 0) return GLIM_AMD_ERR_INVALID;
  return run_vgicp_align(targets, sources, T_init12, flags, count, params, out, trace);
}

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

int glim_amd_ct_align_default_params(glim_amd_lm_params* params) {
  if (!params) return GLIM_AMD_ERR_INVALID;
  ct_default_params(params);
  return GLIM_AMD_OK;
}

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

}  // extern "C"
