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
// The ICP fine registration (include/glim_amd.h "ICP fine registration") is the same scheme with the ICP factors' per-point algebra
// (icp_factor.hpp) in the linearising kernel: icp_align_linearize_kernel, then the same decide kernel.  Its trial budget is 400, and an ICP loop
// stops after a dozen or two trials, so its rounds are enqueued in chunks: at most 41 at a time, then the states are copied back and the call
// stops enqueueing when no status is RUNNING.  The state lives on the device, so the chunk length moves no bit of a result; every other loop
// of this file passes chunk 0 and keeps its single synchronisation.
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
//
// The sub-map bundle optimisation (include/glim_amd.h "Sub-map bundle optimisation") is the same scheme over N poses and F binary VGICP factors:
// a round is vgicp_batch_round over the F factors at the candidate's relative poses, all behind the problem's one status word, and the bundle
// decide kernel: one workgroup that expands the records, assembles the dense 6N x 6N system, factorises it in LDS, retracts the poses and
// writes the next round's relative poses, every value by the item functions of bundle_lm_step.hpp.
//
// The global-graph optimisation (include/glim_amd.h "Global-graph optimisation") is the bundle at up to 256 poses: the same host scaffold, the
// same factors' round and the same item functions, but the systems live in device memory and the decide step is a sequence of launches
// (graph_round below; the blocked solve's launches are graph_align.hip's, graph_solve.hpp).  Its rounds are enqueued a few at a time, as the
// ICP loop's are.
//
// Both take damping terms and Huber widths of the between terms (include/glim_amd.h "Damping terms and Huber between terms") through the same
// item functions: the two arrays live in device memory beside the graph, and so do the betweens' weights -- those of a round's evaluation, and
// those of the kept evaluation, which the kernel that keeps a candidate's poses and records copies with them.
//
// The scan-to-keyframes VGICP registration (include/glim_amd.h "Scan-to-keyframes VGICP registration") is the same scheme over ONE pose per
// problem and M unary VGICP factors with fixed target poses: a round is vgicp_batch_round over the F factors of all problems at T_f = P_f^-1 X,
// each behind a status word of its own, and the keyframe decide kernel: one wavefront per problem that sums the problem's M records in
// ascending order, 29 independent sums in 29 lanes, adds the prior's contribution, runs the step rule of lm_step.hpp on the sum and fans the
// next candidate out to the M factor poses -- a six-parameter solve per problem, no dense bundle (keyframe_lm_step.hpp).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <mutex>
#include <vector>

#include "bundle_lm_step.hpp"
#include "ct_factor.hpp"
#include "ct_lm_step.hpp"
#include "device_math.hpp"
#include "gicp_factor.hpp"
#include "graph_solve.hpp"
#include "icp_factor.hpp"
#include "internal.hpp"
#include "ivox_map.hpp"
#include "keyframe_lm_step.hpp"
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

// what the decide kernels of both batches do with a problem's record, in one thread: the step rule on the state, and the round's trace entry
// when a trace was asked for (`entry`: the problem's entry of this round, or null).  s: the state after the round
__device__ __forceinline__ void decide_problem(const lm::Params& prm, lm::State* __restrict__ state, lm::State& s, const double* rec,
                                               glim_amd_align_trace_entry* __restrict__ entry) {
  s = *state;
  glim_amd_align_trace_entry e;
  for (int k = 0; k < 12; k++) e.T_candidate[k] = s.cand[k];
  e.lambda = s.lambda;
  lm::step(prm, s, rec);
  *state = s;
  if (entry) {
    for (int t = 0; t < COMPACT; t++) e.compact[t] = rec[t];
    e.accepted = s.accepted;
    e.status = s.status;
    *entry = e;
  }
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

// ---- the sub-map bundle optimisation ----
static_assert(sizeof(glim_amd_linearized6) == 122 * sizeof(double), "a factor's blocks, in doubles");
static_assert(sizeof(bundle_lm::Scalars) % sizeof(double) == 0 && offsetof(bundle_lm::Scalars, status) % sizeof(int) == 0, "the scalars of a state");
static_assert(bundle_lm::MAX_POSES == GLIM_AMD_BUNDLE_MAX_POSES && bundle_lm::MAX_FACTORS == GLIM_AMD_BUNDLE_MAX_FACTORS &&
                  bundle_lm::MAX_TERMS == GLIM_AMD_BUNDLE_MAX_TERMS,
              "the caps");
constexpr int BUNDLE_THREADS = 512;
static_assert(BUNDLE_THREADS > bundle_lm::MAX_DIM, "a thread per row of the solve, the right-hand side included");
static_assert(2 * bundle_lm::MAX_FACTORS + 2 * bundle_lm::MAX_TERMS <= bundle_lm::MAX_SYSTEM, "the cost sums are staged where the system is assembled afterwards");

struct BundleTrace {  // device arrays of the diag entry, or all null
  double *X, *Tf, *rec;
  glim_amd_bundle_trace_round* rounds;
};

// T_f of the initial poses, where round 0 evaluates the factors
__global__ __launch_bounds__(256) void bundle_pose_kernel(const bundle_lm::Problem pr) {
  for (int f = threadIdx.x; f < pr.g.F; f += 256) bundle_lm::relative_pose(pr.cand, pr.g.ft, pr.g.fs, f, pr.Tf);
}

// One workgroup: bundle_lm::step across the threads.  Every value is produced by the header's item function, one owner per item: a factor's
// blocks and a term's contribution (a thread each), an entry of the system (a thread each, its sum in the list's order), column j of the
// Cholesky factor (thread i takes L[i][j]; the thread of row j + 1 goes on to the pivot of column j + 1, so a column costs ONE barrier), the
// back substitution by columns (thread i keeps s[i] in a register), a pose's retraction, a factor's relative pose.  The system is packed rows in
// LDS: the rows of a column step start at different offsets mod 64, row j is a broadcast.  one_thread: thread 0 runs step() as it stands.
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_decide_kernel(const bundle_lm::Problem pr, const lm::Params prm, const double* __restrict__ recs,
                                                                       const BundleTrace tr, int round, int one_thread) {
#pragma clang fp contract(off)
  using namespace bundle_lm;
  __shared__ double s_W[MAX_SYSTEM];
  __shared__ double s_delta[MAX_DIM];
  __shared__ double s_sums[4];
  __shared__ Scalars s_sc;
  __shared__ int s_bad, s_keep, s_fail;
  if (pr.s->status != lm::RUNNING) return;  // the same for every thread of the block
  const int t = threadIdx.x;
  const Graph& g = pr.g;
  const int N = g.N, F = g.F, n = 6 * N, nsys = system_doubles(n);
  const double lambda_before = pr.s->lambda;
  if (tr.rounds) {
    for (int u = t; u < 12 * N; u += BUNDLE_THREADS) tr.X[(size_t)round * 12 * N + u] = pr.cand[u];
    for (int u = t; u < 12 * F; u += BUNDLE_THREADS) tr.Tf[(size_t)round * 12 * F + u] = pr.Tf[u];
    for (int u = t; u < lm::RECORD * F; u += BUNDLE_THREADS) tr.rec[(size_t)round * lm::RECORD * F + u] = recs[u];
  }
  auto finish = [&](const Scalars& s) {  // thread 0
    *pr.s = s;
    if (tr.rounds) {
      glim_amd_bundle_trace_round e;
      e.lambda = lambda_before;
      e.cost = s.trial_cost;
      e.accepted = s.accepted;
      e.status = s.status;
      tr.rounds[round] = e;
    }
  };
  if (t == 0) {
    s_sc = *pr.s;
    s_sc.accepted = 0;
    s_bad = s_fail = s_keep = 0;
  }
  __syncthreads();
  if (one_thread) {
    if (t == 0) {
      Problem q = pr;
      q.W = s_W;
      step(prm, q, recs);
      finish(*pr.s);
    }
    return;
  }
  bool bad = false;
  for (int u = t; u < lm::RECORD * F; u += BUNDLE_THREADS) bad = bad || !lm::finite(recs[u]);
  for (int u = t; u < 12 * N; u += BUNDLE_THREADS) bad = bad || !lm::finite(pr.cand[u]);
  if (bad) s_bad = 1;
  __syncthreads();
  if (s_bad) {
    if (t == 0) {
      s_sc.status = lm::NUMERIC;
      finish(s_sc);
    }
    return;
  }
  for (int w = t; w < F + g.P + g.Q; w += BUNDLE_THREADS) {
    if (w < F) expand_factor(recs, pr.Tf, w, pr.lin);
    else if (w < F + g.P) prior_term(g, pr.cand, w - F, pr.pc);
    else between_term(g, pr.cand, w - F - g.P, pr.bc, pr.wt);
  }
  for (int f = t; f < F; f += BUNDLE_THREADS) {
    s_W[f] = recs[lm::RECORD * f + 1];
    s_W[F + f] = recs[lm::RECORD * f];
  }
  __syncthreads();
  for (int q = t; q < g.P; q += BUNDLE_THREADS) s_W[2 * F + q] = pr.pc[PRIOR_STRIDE * q + 42];
  for (int q = t; q < g.Q; q += BUNDLE_THREADS) s_W[2 * F + g.P + q] = pr.bc[BETWEEN_STRIDE * q + 156];
  __syncthreads();
  if (t == 0) s_sums[0] = sum_ascending(s_W, F, 1);
  if (t == 64) s_sums[1] = sum_ascending(s_W + F, F, 1);
  if (t == 128) s_sums[2] = sum_ascending(s_W + 2 * F, g.P, 1);
  if (t == 192) s_sums[3] = sum_ascending(s_W + 2 * F + g.P, g.Q, 1);
  __syncthreads();
  for (int u = t, r = 0; u < tri(n); u += BUNDLE_THREADS) {
    while (tri(r + 1) <= u) r++;
    s_W[u] = assemble_entry(g, pr.lin, pr.pc, pr.bc, r, u - tri(r));
  }
  for (int r = t; r < n; r += BUNDLE_THREADS) s_W[tri(n) + r] = assemble_rhs(g, pr.lin, pr.pc, pr.bc, r);
  __syncthreads();
  for (int u = t; u < nsys; u += BUNDLE_THREADS) bad = bad || !lm::finite(s_W[u]);
  if (bad) s_bad = 1;
  __syncthreads();
  if (t == 0) {
    const double cost = (s_sums[0] + s_sums[2]) + s_sums[3];
    if (s_bad || !lm::finite(cost)) {
      s_sc.status = lm::NUMERIC;
      s_keep = -1;
    } else {
      s_keep = decide(prm, F, s_sc, cost, s_sums[0], s_sums[2], s_sums[3], s_sums[1]) ? 1 : 0;
    }
  }
  __syncthreads();
  const int keep = s_keep;
  const bool running = s_sc.status == lm::RUNNING;
  if (keep > 0) {
    for (int u = t; u < 12 * N; u += BUNDLE_THREADS) pr.X[u] = pr.cand[u];
    for (int u = t; u < lm::RECORD * F; u += BUNDLE_THREADS) pr.rec[u] = recs[u];
    for (int u = t; u < g.Q; u += BUNDLE_THREADS) pr.wk[u] = pr.wt[u];  // the weights of the kept evaluation (its thread wrote wt[u] before the barriers)
  }
  if (keep > 0 || running) {  // the kept system goes out, the solve's matrix comes in; a thread owns the same entries in both
    const double lambda = s_sc.lambda;
    for (int u = t, i = 0; u < nsys; u += BUNDLE_THREADS) {
      while (i < n && tri(i + 1) <= u) i++;
      if (keep > 0) pr.S[u] = s_W[u];
      if (running) s_W[u] = solve_load(keep > 0 ? s_W : pr.S, n, lambda, u, i, u - tri(i));
    }
  }
  if (!running) {
    if (t == 0) finish(s_sc);
    return;
  }
  __syncthreads();
  if (t == 0) {
    const double d = chol_pivot(s_W, 0);
    if (d > 0.0) s_W[0] = d;
    else s_fail = 1;
  }
  __syncthreads();
  for (int j = 0; j < n; j++) {  // (a failed pivot is left in place: the columns after it are computed and never used)
    const int i = j + 1 + t;
    if (i <= n) {
      s_W[tri(i) + j] = chol_entry(s_W, i, j);
      if (t == 0 && i < n) {
        const double d = chol_pivot(s_W, i);
        if (d > 0.0) s_W[tri(i) + i] = d;
        else s_fail = 1;
      }
    }
    __syncthreads();
  }
  const bool solved = s_fail == 0;
  if (solved) {
    double s = t < n ? s_W[tri(n) + t] : 0.0;
    for (int k = n - 1; k >= 0; k--) {
      if (t == k) s_delta[k] = s / s_W[tri(k) + k];
      __syncthreads();
      if (t < k) s -= s_W[tri(k) + t] * s_delta[k];
    }
  } else if (t < n) {
    s_delta[t] = 0.0;
  }
  __syncthreads();
  if (t < n) pr.delta[t] = s_delta[t];
  if (t < N) {
    if (solved) {
      lm::retract(pr.X + 12 * t, s_delta + 6 * t, pr.cand + 12 * t);
    } else {
      for (int i = 0; i < 12; i++) pr.cand[12 * t + i] = pr.X[12 * t + i];
    }
  }
  __syncthreads();
  bad = false;
  for (int u = t; u < 12 * N; u += BUNDLE_THREADS) bad = bad || !lm::finite(pr.cand[u]);
  if (bad) s_bad = 1;
  __syncthreads();
  if (!s_bad)
    for (int f = t; f < F; f += BUNDLE_THREADS) relative_pose(pr.cand, g.ft, g.fs, f, pr.Tf);
  if (t == 0) {
    s_sc.solve_ok = solved ? 1 : 0;
    if (s_bad) s_sc.status = lm::NUMERIC;
    finish(s_sc);
  }
}

// ---- the global-graph optimisation ----
// bundle_lm::step once more, at up to GLIM_AMD_GRAPH_MAX_POSES poses: the same item functions, one owner per item, but as a sequence of ordinary
// launches with the systems in device memory.  A kernel boundary on the one stream is the only ordering; what a later kernel of the round has to
// know of an earlier one's outcome (the decision, a non-finite value, a failed pivot) it reads in device memory: the problem's Scalars and
// GraphWords.  The solve's matrix is graph_solve.hpp's and its launches are graph_align.hip's.
static_assert(GLIM_AMD_GRAPH_MAX_POSES * 6 == graph_solve::MAX_DIM, "the caps");
static_assert(GLIM_AMD_GRAPH_MAX_FACTORS >= GLIM_AMD_GRAPH_MAX_POSES * (GLIM_AMD_GRAPH_MAX_POSES - 1) / 2, "every pair of the poses");
constexpr int GRAPH_THREADS = 256;
constexpr int GRAPH_SUM_CHUNK = 512;
constexpr int GRAPH_ROUNDS_PER_CHUNK = 4;

struct GraphWords {
  double lambda_before;  // of the round: what its trace entry reports
  int bad_in;            // a record, a candidate or an assembled entry of the round is not finite
  int bad_out;           // a next candidate is not finite
  int keep;              // the round's decision: the candidate is kept
  int fail;              // the round's solve met a pivot that is not > 0
};

struct GraphScratch {
  double* E;  // system_doubles(n): the evaluated system, packed as the rule has it (Problem::W)
  double* M;  // graph_solve::matrix_doubles(n): the solve's matrix, column-major
  GraphWords* words;
};
size_t graph_scratch_doubles(int n) { return (size_t)bundle_lm::system_doubles(n) + graph_solve::matrix_doubles(n) + sizeof(GraphWords) / sizeof(double); }
GraphScratch graph_scratch_at(double* d, int n) {
  GraphScratch g;
  g.E = d;
  g.M = g.E + bundle_lm::system_doubles(n);
  g.words = reinterpret_cast<GraphWords*>(g.M + graph_solve::matrix_doubles(n));
  return g;
}
static_assert(sizeof(GraphWords) % sizeof(double) == 0, "the words follow the matrix");

__device__ __forceinline__ int graph_thread() { return (int)((blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x); }
__device__ __forceinline__ int graph_threads() { return (int)(gridDim.y * gridDim.x * blockDim.x); }

__device__ __forceinline__ void graph_trace_round(const bundle_lm::Problem& pr, const GraphWords* w, const BundleTrace& tr, int round) {
  if (!tr.rounds) return;
  glim_amd_bundle_trace_round e;
  e.lambda = w->lambda_before;
  e.cost = pr.s->trial_cost;
  e.accepted = pr.s->accepted;
  e.status = pr.s->status;
  tr.rounds[round] = e;
}

// the items of a round: a factor's blocks, a term's contribution (a thread each); the finite check of what the round was given; the trace's
// copies of it
__global__ __launch_bounds__(GRAPH_THREADS) void graph_items_kernel(const bundle_lm::Problem pr, GraphWords* w, const double* __restrict__ recs, const BundleTrace tr,
                                                                    int round) {
  using namespace bundle_lm;
  if (pr.s->status != lm::RUNNING) return;  // the same for every thread of the grid
  const Graph& g = pr.g;
  const int N = g.N, F = g.F, t = graph_thread(), T = graph_threads();
  if (tr.rounds) {
    for (int u = t; u < 12 * N; u += T) tr.X[(size_t)round * 12 * N + u] = pr.cand[u];
    for (int u = t; u < 12 * F; u += T) tr.Tf[(size_t)round * 12 * F + u] = pr.Tf[u];
    for (int u = t; u < lm::RECORD * F; u += T) tr.rec[(size_t)round * lm::RECORD * F + u] = recs[u];
  }
  bool bad = false;
  for (int u = t; u < lm::RECORD * F; u += T) bad = bad || !lm::finite(recs[u]);
  for (int u = t; u < 12 * N; u += T) bad = bad || !lm::finite(pr.cand[u]);
  if (bad) w->bad_in = 1;
  const int pose_items = F + g.P + g.Q, items = pose_items + g.nav.VP + g.nav.VB + g.nav.I;
  for (int i = t; i < items; i += T) {
    if (i < F) expand_factor(recs, pr.Tf, i, pr.lin);
    else if (i < F + g.P) prior_term(g, pr.cand, i - F, pr.pc);
    else if (i < pose_items) between_term(g, pr.cand, i - F - g.P, pr.bc, pr.wt);
    else if (i < pose_items + g.nav.VP) nav::vector_prior_term(g.nav, pr.cand, i - pose_items);
    else if (i < pose_items + g.nav.VP + g.nav.VB) nav::vector_between_term(g.nav, pr.cand, i - pose_items - g.nav.VP);
    else nav::imu_term(g.nav, pr.cand, i - pose_items - g.nav.VP - g.nav.VB);
  }
}

// the evaluated system: blockIdx.y is the row (row n: b), the threads run along the columns; an entry is its list's sum
__global__ __launch_bounds__(GRAPH_THREADS) void graph_assemble_kernel(const bundle_lm::Problem pr, GraphWords* w) {
  using namespace bundle_lm;
  if (pr.s->status != lm::RUNNING) return;
  const int n = 6 * pr.g.N, r = (int)blockIdx.y, c = (int)(blockIdx.x * GRAPH_THREADS + threadIdx.x);
  if (c >= n || (r < n && c > r)) return;
  const double v = r < n ? assemble_entry(pr.g, pr.lin, pr.pc, pr.bc, r, c) : assemble_rhs(pr.g, pr.lin, pr.pc, pr.bc, c);
  pr.W[tri(r) + c] = v;
  if (!lm::finite(v)) w->bad_in = 1;
}

// One small workgroup: the seven ascending sums (the factors' two, the priors' and the betweens' by a wavefront's first thread each, the
// vector priors', the vector betweens' and the IMU terms' by the 33rd thread of the first three wavefronts, over values the workgroup stages in
// LDS chunk by chunk) and bundle_lm::decide.  The decision goes into the problem's Scalars and words, where the later kernels of the round read it
__global__ __launch_bounds__(GRAPH_THREADS) void graph_decide_kernel(const bundle_lm::Problem pr, const lm::Params prm, GraphWords* w, const double* __restrict__ recs,
                                                                     const BundleTrace tr, int round) {
#pragma clang fp contract(off)
  using namespace bundle_lm;
  __shared__ double s_v[7][GRAPH_SUM_CHUNK];
  __shared__ double s_sums[7];
  const int t = threadIdx.x;
  if (pr.s->status != lm::RUNNING) {  // the same for every thread
    if (t == 0) w->keep = 0;
    return;
  }
  const Graph& g = pr.g;
  const int F = g.F, most = max(max(F, max(g.P, g.Q)), max(g.nav.VP, max(g.nav.VB, g.nav.I)));
  const int owns = t % 64 == 0 ? t / 64 : t % 64 == 32 && t < 192 ? 4 + t / 64 : -1;  // the sum this thread owns
  const int count = owns < 0 ? 0 : owns < 2 ? F : owns == 2 ? g.P : owns == 3 ? g.Q : owns == 4 ? g.nav.VP : owns == 5 ? g.nav.VB : g.nav.I;
  double sum = 0.0;  // of the thread that owns a sum: sum_ascending over the chunks
  for (int base = 0; base < most; base += GRAPH_SUM_CHUNK) {
    for (int u = t; u < GRAPH_SUM_CHUNK; u += GRAPH_THREADS) {
      const int i = base + u;
      if (i < F) {
        s_v[0][u] = recs[(size_t)lm::RECORD * i + 1];
        s_v[1][u] = recs[(size_t)lm::RECORD * i];
      }
      if (i < g.P) s_v[2][u] = pr.pc[(size_t)PRIOR_STRIDE * i + 42];
      if (i < g.Q) s_v[3][u] = pr.bc[(size_t)BETWEEN_STRIDE * i + 156];
      if (i < g.nav.VP) s_v[4][u] = g.nav.vpc[(size_t)nav::VPRIOR_STRIDE * i + 42];
      if (i < g.nav.VB) s_v[5][u] = g.nav.vbc[(size_t)nav::VBETWEEN_STRIDE * i + 156];
      if (i < g.nav.I) s_v[6][u] = g.nav.ic[(size_t)nav::IMU_STRIDE * i + nav::IMU_STRIDE - 1];
    }
    __syncthreads();
    if (owns >= 0) {
      const int end = min(GRAPH_SUM_CHUNK, count - base);
      for (int u = 0; u < end; u++) sum += s_v[owns][u];
    }
    __syncthreads();
  }
  if (owns >= 0) s_sums[owns] = sum;
  __syncthreads();
  if (t != 0) return;
  Scalars sc = *pr.s;
  sc.accepted = 0;
  w->lambda_before = sc.lambda;
  const double cost = total_cost(s_sums[0], s_sums[2], s_sums[3], s_sums[4], s_sums[5], s_sums[6]);
  int keep = 0;
  if (w->bad_in || !lm::finite(cost)) sc.status = lm::NUMERIC;
  else keep = decide(prm, F, sc, cost, s_sums[0], s_sums[2], s_sums[3], s_sums[1], s_sums[4], s_sums[5], s_sums[6]) ? 1 : 0;
  *pr.s = sc;
  w->keep = keep;
  w->bad_in = w->bad_out = 0;
  if (sc.status != lm::RUNNING) graph_trace_round(pr, w, tr, round);  // the round ends here
}

// entry (i, j) of the solve's matrix from a packed system
__device__ __forceinline__ void graph_load_entry(const double* S, int n, double lambda, int i, int j, double* M) {
  const int u = bundle_lm::tri(i) + j;
  M[(size_t)j * graph_solve::leading(n) + i] = bundle_lm::solve_load(S, n, lambda, u, i, j);
}

// a kept candidate: its poses, records and system become the kept ones; while the loop runs: the solve's matrix from the kept system
__global__ __launch_bounds__(GRAPH_THREADS) void graph_keep_load_kernel(const bundle_lm::Problem pr, const GraphWords* __restrict__ w, const double* __restrict__ recs,
                                                                        double* M) {
  using namespace bundle_lm;
  const bool keep = w->keep > 0, running = pr.s->status == lm::RUNNING;
  if (!keep && !running) return;
  const int N = pr.g.N, F = pr.g.F, n = 6 * N;
  if (keep) {
    const int t = graph_thread(), T = graph_threads();
    for (int u = t; u < 12 * N; u += T) pr.X[u] = pr.cand[u];
    for (int u = t; u < lm::RECORD * F; u += T) pr.rec[u] = recs[u];
    for (int u = t; u < pr.g.Q; u += T) pr.wk[u] = pr.wt[u];
  }
  const int i = (int)blockIdx.y, j = (int)(blockIdx.x * GRAPH_THREADS + threadIdx.x);
  if (j >= n || (i < n && j > i)) return;
  const int u = tri(i) + j;
  if (keep) pr.S[u] = pr.W[u];
  if (running) graph_load_entry(keep ? pr.W : pr.S, n, pr.s->lambda, i, j, M);
}

__global__ __launch_bounds__(GRAPH_THREADS) void graph_load_kernel(const double* __restrict__ S, int n, double lambda, double* M) {
  const int i = (int)blockIdx.y, j = (int)(blockIdx.x * GRAPH_THREADS + threadIdx.x);
  if (j >= n || (i < n && j > i)) return;
  graph_load_entry(S, n, lambda, i, j, M);
}

// the next candidates: a node each, retracted by its kind.  After a failed solve they are the kept poses (the solve has left delta at +0.0)
__global__ __launch_bounds__(GRAPH_THREADS) void graph_retract_kernel(const bundle_lm::Problem pr, GraphWords* w) {
  if (pr.s->status != lm::RUNNING) return;
  const int k = (int)(blockIdx.x * GRAPH_THREADS + threadIdx.x);
  if (k >= pr.g.N) return;
  if (!w->fail) {
    nav::retract_node(nav::kind_of(pr.g.nav, k), pr.X + 12 * k, pr.delta + 6 * k, pr.cand + 12 * k);
  } else {
    for (int i = 0; i < 12; i++) pr.cand[12 * k + i] = pr.X[12 * k + i];
  }
  if (!lm::all_finite(pr.cand + 12 * k, 12)) w->bad_out = 1;
}

// the next round's T_f, a factor each, and the end of the round's bookkeeping (the first thread)
__global__ __launch_bounds__(GRAPH_THREADS) void graph_next_kernel(const bundle_lm::Problem pr, const GraphWords* w, const BundleTrace tr, int round) {
  // (the first thread may set NUMERIC below while another workgroup starts: that workgroup has nothing to do either way)
  if (pr.s->status != lm::RUNNING) return;
  const int bad = w->bad_out, f = (int)(blockIdx.x * GRAPH_THREADS + threadIdx.x);
  if (!bad && f < pr.g.F) bundle_lm::relative_pose(pr.cand, pr.g.ft, pr.g.fs, f, pr.Tf);
  if (f == 0) {
    pr.s->solve_ok = w->fail ? 0 : 1;
    if (bad) pr.s->status = lm::NUMERIC;
    graph_trace_round(pr, w, tr, round);
  }
}

// the cross-check variant: one thread runs step() as it stands, with W in device memory
__global__ __launch_bounds__(64) void graph_one_thread_kernel(const bundle_lm::Problem pr, const lm::Params prm, GraphWords* w, const double* __restrict__ recs,
                                                              const BundleTrace tr, int round) {
  using namespace bundle_lm;
  if (pr.s->status != lm::RUNNING) return;
  const int t = threadIdx.x, N = pr.g.N, F = pr.g.F;
  if (tr.rounds) {
    for (int u = t; u < 12 * N; u += 64) tr.X[(size_t)round * 12 * N + u] = pr.cand[u];
    for (int u = t; u < 12 * F; u += 64) tr.Tf[(size_t)round * 12 * F + u] = pr.Tf[u];
    for (int u = t; u < lm::RECORD * F; u += 64) tr.rec[(size_t)round * lm::RECORD * F + u] = recs[u];
  }
  if (t != 0) return;
  w->lambda_before = pr.s->lambda;
  Problem q = pr;
  step(prm, q, recs);
  graph_trace_round(pr, w, tr, round);
}

// the launches of one round behind the factors' evaluation
int graph_round(const bundle_lm::Problem& pr, const GraphScratch& gs, const lm::Params& prm, const double* d_recs, const int* d_status, const BundleTrace& tr, int round,
                int one_thread, hipStream_t st) {
  const bundle_lm::Graph& g = pr.g;
  if (one_thread) {
    graph_one_thread_kernel<<<1, 64, 0, st>>>(pr, prm, gs.words, d_recs, tr, round);
    return GLIM_AMD_OK;
  }
  const int n = 6 * g.N;
  auto blocks = [](int count) { return std::max(1, (count + GRAPH_THREADS - 1) / GRAPH_THREADS); };
  const dim3 square(blocks(n), n + 1);
  graph_items_kernel<<<blocks(g.F + g.P + g.Q + g.nav.VP + g.nav.VB + g.nav.I), GRAPH_THREADS, 0, st>>>(pr, gs.words, d_recs, tr, round);
  graph_assemble_kernel<<<square, GRAPH_THREADS, 0, st>>>(pr, gs.words);
  graph_decide_kernel<<<1, GRAPH_THREADS, 0, st>>>(pr, prm, gs.words, d_recs, tr, round);
  graph_keep_load_kernel<<<square, GRAPH_THREADS, 0, st>>>(pr, gs.words, d_recs, gs.M);
  GA_HIP(graph_solve_enqueue(st, gs.M, n, pr.delta, &gs.words->fail, d_status));
  graph_retract_kernel<<<blocks(g.N), GRAPH_THREADS, 0, st>>>(pr, gs.words);
  graph_next_kernel<<<blocks(g.F), GRAPH_THREADS, 0, st>>>(pr, gs.words, tr, round);
  return GLIM_AMD_OK;
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

void icp_default_params(glim_amd_lm_params* p) {
  lm_default_params(p);
  p->max_iterations = 200;  // manual_loop_close_modal.cpp:490
}

void bundle_default_params(glim_amd_lm_params* p) {
  lm_default_params(p);
  p->max_iterations = 20;
}

bool all_finite_host(const double* v, int n) {
  for (int k = 0; k < n; k++)
    if (!std::isfinite(v[k])) return false;
  return true;
}

// ---- the host scaffold the four run_* functions share ----
// the caller's parameters, or the loop's defaults, checked and resolved (max_trials 0 = twice max_iterations); rounds = 1 + max_trials
int resolve_params(const glim_amd_lm_params* params, void (*defaults)(glim_amd_lm_params*), lm::Params* prm, int* rounds) {
  glim_amd_lm_params c;
  if (params) c = *params;
  else defaults(&c);
  if (!lm_params_ok(c)) return GLIM_AMD_ERR_INVALID;
  if (c.max_trials == 0) c.max_trials = 2 * c.max_iterations;
  if (c.max_trials > ALIGN_MAX_TRIALS) return GLIM_AMD_ERR_INVALID;
  memcpy(prm, &c, sizeof(*prm));
  *rounds = 1 + prm->max_trials;
  return GLIM_AMD_OK;
}

// every handle is non-null and of one context: `ctx`, or the first target's when `ctx` is null.  Returns that context, or null
template <class Handle>
glim_amd_ctx* one_context(const Handle* const* targets, const glim_amd_cloud* const* sources, int count, glim_amd_ctx* ctx) {
  for (int i = 0; i < count; i++) {
    if (!targets[i] || !sources[i]) return nullptr;
    if (!ctx) ctx = (glim_amd_ctx*)targets[i]->ctx;
    if ((glim_amd_ctx*)targets[i]->ctx != ctx || (glim_amd_ctx*)sources[i]->ctx != ctx) return nullptr;
  }
  return ctx;
}

// what glim_amd_factor_set_add answers for each (voxel map, source) pair, then the empty source
int vgicp_pairs_ok(const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, int count) {
  for (int i = 0; i < count; i++) {
    if (!targets[i]->buckets || !sources[i]->has_covs) return GLIM_AMD_ERR_STATE;
    if (sources[i]->n == 0 || sources[i]->n > (int64_t)(1u << 28)) return GLIM_AMD_ERR_INVALID;
  }
  return GLIM_AMD_OK;
}

// a trace array: a cleared device buffer while the call runs and the copy back to the caller's, or nothing at all when the caller gave none
struct TraceBuffer {
  DeviceTemp d;
  void* host = nullptr;
  size_t bytes = 0;
  int open(void* host_array, size_t nbytes, hipStream_t st) {
    if (!host_array) return GLIM_AMD_OK;
    host = host_array;
    bytes = nbytes;
    GA_HIP(pool_malloc(&d.p, std::max<size_t>(8, bytes)));
    GA_HIP(hipMemsetAsync(d.p, 0, std::max<size_t>(8, bytes), st));
    return GLIM_AMD_OK;
  }
  int fetch(hipStream_t st) {
    if (host && bytes) GA_HIP(hipMemcpyAsync(host, d.p, bytes, hipMemcpyDeviceToHost, st));
    return GLIM_AMD_OK;
  }
};

void align_result(const lm::State& s, glim_amd_align_result* o) {
  memset(o, 0, sizeof(*o));
  memcpy(o->T_target_source, s.T, sizeof(o->T_target_source));
  memcpy(o->compact, s.rec, sizeof(o->compact));
  o->error = s.rec[1];
  o->num_inliers = (int64_t)llround(s.rec[0]);
  o->iterations = s.iterations;
  o->trials = s.trials;
  o->status = s.status;
  o->lambda = s.lambda;
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
  out->cost = state.sys[1];
  out->location_cost = state.cost_p;
  out->between_cost = state.cost_b;
  out->lambda = state.lambda;
  out->iterations = state.iterations;
  out->trials = state.trials;
  out->status = state.status;
  return GLIM_AMD_OK;
}

// the most rounds the ICP fine registration enqueues before it looks at the statuses: the most the other loops enqueue by default (1 + 2 x 20)
constexpr int ICP_ROUNDS_PER_CHUNK = 41;

// the batch over either kind of target: Handle = glim_amd_nn_index or glim_amd_ivox.  trace: count * (1 + max_trials) entries, or null.
// metric: the factor of the loop (the ICP factors: an index only).  chunk: rounds enqueued between two looks at the statuses; 0: all of them up
// front and ONE synchronisation.  The state lives on the device: the chunk length moves no bit of a result.
template <class Handle>
int run_align(const Handle* const* targets, const glim_amd_cloud* const* sources, const double* T_init12, const double* max_dists, int32_t count,
              const glim_amd_lm_params* params, glim_amd_align_result* out, glim_amd_align_trace_entry* trace_host, Metric metric = Metric::GICP,
              int chunk = 0, void (*defaults)(glim_amd_lm_params*) = lm_default_params) {
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
  if (trace_host.rounds) {  // (the entry point has seen to it that the four arrays come together)
    GA_TRY(trounds.open(trace_host.rounds, (size_t)count * rounds * sizeof(glim_amd_align_trace_entry), st));
    GA_TRY(tprior.open(trace_host.prior, (size_t)count * rounds * keyframe_lm::PRIOR * sizeof(double), st));
    GA_TRY(tTf.open(trace_host.Tf, (size_t)rounds * F * 12 * sizeof(double), st));
    GA_TRY(trec.open(trace_host.rec, (size_t)rounds * F * lm::RECORD * sizeof(double), st));
  }
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
  GA_TRY(trounds.fetch(st));
  GA_TRY(tprior.fetch(st));
  GA_TRY(tTf.fetch(st));
  GA_TRY(trec.fetch(st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  batch.seen_complete();
  if (factor_compact_out) memcpy(factor_compact_out, kept_host.data(), kept_bytes);
  for (int i = 0; i < count; i++) align_result(states[(size_t)i], out + i);
  return GLIM_AMD_OK;
}

// ---- the host scaffold of the two N-pose loops (the sub-map bundle, the global graph) ----
struct GraphCaps {
  int poses, factors, terms;
};

// the refusals of glim_amd_graph_align_nav's node kinds and new terms (the counts and the arrays have been looked at)
int check_nav_args(const glim_amd_nav_terms& nav, const int32_t* target_pose, const int32_t* source_pose, int F, const glim_amd_bundle_prior* priors, int P,
                   const glim_amd_bundle_between* betweens, int Q, const double* X, int N) {
  auto kind = [&](int k) { return nav.kinds ? nav.kinds[k] : GLIM_AMD_NODE_POSE; };
  auto is = [&](int k, int want) { return k >= 0 && k < N && kind(k) == want; };
  auto vector_kind = [&](int k) { return is(k, GLIM_AMD_NODE_BIAS) || is(k, GLIM_AMD_NODE_VELOCITY); };
  for (int k = 0; k < N; k++) {
    const int kd = kind(k);
    if (kd != GLIM_AMD_NODE_POSE && kd != GLIM_AMD_NODE_BIAS && kd != GLIM_AMD_NODE_VELOCITY) return GLIM_AMD_ERR_INVALID;
    for (int u = kd == GLIM_AMD_NODE_POSE ? 12 : nav::node_dim(kd); u < 12; u++)
      if (X[12 * k + u] != 0.0 || std::signbit(X[12 * k + u])) return GLIM_AMD_ERR_INVALID;
  }
  for (int f = 0; f < F; f++)
    if (!is(target_pose[f], GLIM_AMD_NODE_POSE) || !is(source_pose[f], GLIM_AMD_NODE_POSE)) return GLIM_AMD_ERR_INVALID;
  for (int p = 0; p < P; p++)
    if (!is(priors[p].pose, GLIM_AMD_NODE_POSE)) return GLIM_AMD_ERR_INVALID;
  for (int q = 0; q < Q; q++)
    if (!is(betweens[q].pose_i, GLIM_AMD_NODE_POSE) || !is(betweens[q].pose_j, GLIM_AMD_NODE_POSE)) return GLIM_AMD_ERR_INVALID;
  for (int p = 0; p < nav.num_vector_priors; p++) {
    const glim_amd_nav_vector_prior& e = nav.vector_priors[p];
    if (!vector_kind(e.node) || !all_finite_host(e.value, 6) || !all_finite_host(e.information, 36)) return GLIM_AMD_ERR_INVALID;
  }
  for (int q = 0; q < nav.num_vector_betweens; q++) {
    const glim_amd_nav_vector_between& e = nav.vector_betweens[q];
    if (!vector_kind(e.node_i) || !vector_kind(e.node_j) || e.node_i == e.node_j || kind(e.node_i) != kind(e.node_j)) return GLIM_AMD_ERR_INVALID;
    if (!all_finite_host(e.measurement, 6) || !all_finite_host(e.information, 36)) return GLIM_AMD_ERR_INVALID;
  }
  for (int q = 0; q < nav.num_imu_terms; q++) {
    const glim_amd_nav_imu_term& e = nav.imu_terms[q];
    if (e.mode != GLIM_AMD_IMU_TANGENT && e.mode != GLIM_AMD_IMU_MANIFOLD) return GLIM_AMD_ERR_INVALID;
    if (!is(e.pose_i, GLIM_AMD_NODE_POSE) || !is(e.pose_j, GLIM_AMD_NODE_POSE) || !is(e.velocity_i, GLIM_AMD_NODE_VELOCITY) || !is(e.velocity_j, GLIM_AMD_NODE_VELOCITY) ||
        !is(e.bias, GLIM_AMD_NODE_BIAS) || e.pose_i == e.pose_j || e.velocity_i == e.velocity_j)
      return GLIM_AMD_ERR_INVALID;
    if (!all_finite_host(&e.dt, nav::IMU_DATA) || !(e.dt > 0.0)) return GLIM_AMD_ERR_INVALID;
  }
  return GLIM_AMD_OK;
}
static_assert(offsetof(glim_amd_nav_imu_term, dt) == 24 && sizeof(glim_amd_nav_imu_term) == 24 + nav::IMU_DATA * sizeof(double), "a term's doubles are nav::IMU_DATA in a row");
static_assert(GLIM_AMD_NODE_POSE == nav::NODE_POSE && GLIM_AMD_NODE_BIAS == nav::NODE_BIAS && GLIM_AMD_NODE_VELOCITY == nav::NODE_VELOCITY &&
                  GLIM_AMD_IMU_TANGENT == nav::IMU_TANGENT && GLIM_AMD_IMU_MANIFOLD == nav::IMU_MANIFOLD,
              "the kinds and the modes");

// the refusals of glim_amd_bundle_align with a loop's caps: everything that is answered before a handle or the context is used, then the pairs.
// GLIM_AMD_OK with N == 0 is the caller's to answer first
int check_graph_args(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const int32_t* target_pose,
                     const int32_t* source_pose, int32_t F, uint32_t flags, const glim_amd_bundle_prior* priors, int32_t P, const glim_amd_bundle_between* betweens,
                     int32_t Q, const double* X_init12, int32_t N, const glim_amd_lm_params* params, const double* X_out12, const glim_amd_bundle_result* result,
                     const GraphCaps& caps, lm::Params* prm, int* rounds, const glim_amd_graph_terms* more, const glim_amd_nav_terms* nav = nullptr) {
  if (!ctx || !X_init12 || !X_out12 || !result) return GLIM_AMD_ERR_INVALID;
  if (F > 0 && (!targets || !sources || !target_pose || !source_pose)) return GLIM_AMD_ERR_INVALID;
  if ((P > 0 && !priors) || (Q > 0 && !betweens)) return GLIM_AMD_ERR_INVALID;
  const int D = more ? more->num_dampings : 0;
  if (D < 0 || (D > 0 && !more->dampings)) return GLIM_AMD_ERR_INVALID;
  const int VP = nav ? nav->num_vector_priors : 0, VB = nav ? nav->num_vector_betweens : 0, I = nav ? nav->num_imu_terms : 0;
  if (VP < 0 || VB < 0 || I < 0 || (VP > 0 && !nav->vector_priors) || (VB > 0 && !nav->vector_betweens) || (I > 0 && !nav->imu_terms)) return GLIM_AMD_ERR_INVALID;
  if (F + P + Q == 0 && VP == 0 && VB == 0 && I == 0) return GLIM_AMD_ERR_INVALID;  // (dampings alone too: there is nothing to optimise over)
  if (flags & ~(uint32_t)GLIM_AMD_FACTOR_SURFACE_VALIDATION) return GLIM_AMD_ERR_INVALID;  // GLIM_AMD_FACTOR_BINARY: every factor here is binary
  GA_TRY(resolve_params(params, bundle_default_params, prm, rounds));
  if (N > caps.poses || F > caps.factors || P > caps.terms || Q > caps.terms || D > caps.terms) return GLIM_AMD_ERR_UNSUPPORTED;
  if (VP > caps.terms || VB > caps.terms || I > caps.terms) return GLIM_AMD_ERR_UNSUPPORTED;
  if (!one_context(targets, sources, F, ctx)) return GLIM_AMD_ERR_INVALID;
  for (int f = 0; f < F; f++)
    if (target_pose[f] < 0 || target_pose[f] >= N || source_pose[f] < 0 || source_pose[f] >= N || target_pose[f] == source_pose[f]) return GLIM_AMD_ERR_INVALID;
  for (int p = 0; p < P; p++) {
    if (priors[p].pose < 0 || priors[p].pose >= N) return GLIM_AMD_ERR_INVALID;
    if (!all_finite_host(priors[p].T, 12) || !all_finite_host(priors[p].information, 36)) return GLIM_AMD_ERR_INVALID;
  }
  for (int q = 0; q < Q; q++) {
    const glim_amd_bundle_between& b = betweens[q];
    if (b.pose_i < 0 || b.pose_i >= N || b.pose_j < 0 || b.pose_j >= N || b.pose_i == b.pose_j) return GLIM_AMD_ERR_INVALID;
    if (!all_finite_host(b.T, 12) || !all_finite_host(b.information, 36)) return GLIM_AMD_ERR_INVALID;
  }
  for (int d = 0; d < D; d++) {
    const glim_amd_graph_damping& e = more->dampings[d];
    if (e.pose < 0 || e.pose >= N) return GLIM_AMD_ERR_INVALID;
    for (double v : e.diagonal)
      if (!(v >= 0.0) || !std::isfinite(v)) return GLIM_AMD_ERR_INVALID;
  }
  if (more && more->between_huber_width)
    for (int q = 0; q < Q; q++)
      if (!(more->between_huber_width[q] >= 0.0) || !std::isfinite(more->between_huber_width[q])) return GLIM_AMD_ERR_INVALID;
  if (!all_finite_host(X_init12, 12 * N)) return GLIM_AMD_ERR_INVALID;
  if (nav) GA_TRY(check_nav_args(*nav, target_pose, source_pose, F, priors, P, betweens, Q, X_init12, N));
  return vgicp_pairs_ok(targets, sources, F);
}

// One block of doubles and one of ints hold the graph, the state and the scratch of a problem, laid out the same on host and device: the
// offsets in doubles / ints, and the host's copy with the graph, its lists and the state before round 0.  `extra`: doubles of further
// scratch behind the problem's own (o_extra)
struct GraphBlocks {
  size_t o_X, o_cand, o_delta, o_rec, o_S, o_pT, o_pL, o_bT, o_bL, o_dd, o_bw, o_wk, o_scal, upload_doubles, o_pc, o_bc, o_wt, o_lin, o_Tf0, o_extra, total_doubles;
  size_t o_vpv, o_vpL, o_vbd, o_vbL, o_imd, o_vpc, o_vbc, o_ic;  // the node kinds' terms (glim_amd_graph_align_nav)
  size_t i_ft, i_fs, i_pk, i_bi, i_bj, i_dk, i_first, i_items, total_ints;
  size_t i_kind, i_vpk, i_vbi, i_vbj, i_imn, i_imm;
  int N, F, P, Q, D;
  int VP, VB, I;
  bool kinds;   // the nodes carry kinds
  bool widths;  // the betweens carry Huber widths
  std::vector<double> hd;
  std::vector<int> hi;

  bundle_lm::Problem problem_at(double* d, int* i, double* Tf) const {
    using namespace bundle_lm;
    Problem pr{};
    pr.g = Graph{N, F, P, Q, i + i_ft, i + i_fs, i + i_pk, d + o_pT, d + o_pL, i + i_bi, i + i_bj, d + o_bT, d + o_bL, i + i_first, i + i_items,
                 D, i + i_dk, d + o_dd, widths ? d + o_bw : nullptr};
    if (kinds) {
      nav::Terms& t = pr.g.nav;
      t.kind = i + i_kind;
      t.VP = VP, t.VB = VB, t.I = I;
      t.vpk = i + i_vpk, t.vpv = d + o_vpv, t.vpL = d + o_vpL;
      t.vbi = i + i_vbi, t.vbj = i + i_vbj, t.vbd = d + o_vbd, t.vbL = d + o_vbL;
      t.imn = i + i_imn, t.imm = i + i_imm, t.imd = d + o_imd;
      t.vpc = d + o_vpc, t.vbc = d + o_vbc, t.ic = d + o_ic;
    }
    pr.X = d + o_X;
    pr.cand = d + o_cand;
    pr.delta = d + o_delta;
    pr.rec = d + o_rec;
    pr.S = d + o_S;
    pr.Tf = Tf;
    pr.lin = reinterpret_cast<glim_amd_linearized6*>(d + o_lin);
    pr.pc = d + o_pc;
    pr.bc = d + o_bc;
    pr.W = nullptr;  // the bundle kernel's LDS; the graph's scratch
    pr.s = reinterpret_cast<Scalars*>(d + o_scal);
    pr.wt = d + o_wt;
    pr.wk = d + o_wk;
    return pr;
  }

  GraphBlocks(int N_, int F_, int P_, int Q_, const int32_t* target_pose, const int32_t* source_pose, const glim_amd_bundle_prior* priors,
              const glim_amd_bundle_between* betweens, const glim_amd_graph_terms* more, const double* X_init12, const lm::Params& prm, size_t extra,
              const glim_amd_nav_terms* nav = nullptr)
      : N(N_), F(F_), P(P_), Q(Q_), D(more ? more->num_dampings : 0), VP(nav ? nav->num_vector_priors : 0), VB(nav ? nav->num_vector_betweens : 0),
        I(nav ? nav->num_imu_terms : 0), kinds(nav && nav->kinds), widths(more && more->between_huber_width && Q_ > 0) {
    using namespace bundle_lm;
    const int n = 6 * N, nsys = system_doubles(n), nlist = list_items(F, P, Q, D) + VP + 3 * VB + 15 * I;
    size_t at = 0;
    auto take = [&](size_t count) {
      const size_t o = at;
      at += count;
      return o;
    };
    o_X = take(12 * (size_t)N), o_cand = take(12 * (size_t)N), o_delta = take(n), o_rec = take((size_t)lm::RECORD * F), o_S = take(nsys);
    o_pT = take(12 * (size_t)P), o_pL = take(36 * (size_t)P), o_bT = take(12 * (size_t)Q), o_bL = take(36 * (size_t)Q);
    o_dd = take(6 * (size_t)D), o_bw = take(widths ? (size_t)Q : 0), o_wk = take(Q);
    o_scal = take(sizeof(Scalars) / sizeof(double));
    o_vpv = take(6 * (size_t)VP), o_vpL = take(36 * (size_t)VP), o_vbd = take(6 * (size_t)VB), o_vbL = take(36 * (size_t)VB), o_imd = take((size_t)nav::IMU_DATA * I);
    upload_doubles = at;  // what the host fills; the scratch below is written before it is read
    o_pc = take((size_t)PRIOR_STRIDE * P), o_bc = take((size_t)BETWEEN_STRIDE * Q), o_wt = take(Q), o_lin = take(122 * (size_t)F), o_Tf0 = take(12 * (size_t)F);
    o_vpc = take((size_t)nav::VPRIOR_STRIDE * VP), o_vbc = take((size_t)nav::VBETWEEN_STRIDE * VB), o_ic = take((size_t)nav::IMU_STRIDE * I);
    o_extra = take(extra);
    total_doubles = at;
    at = 0;
    i_ft = take(F), i_fs = take(F), i_pk = take(P), i_bi = take(Q), i_bj = take(Q), i_dk = take(D), i_first = take(tri(N) + 1), i_items = take(nlist);
    i_kind = take(kinds ? N : 0), i_vpk = take(VP), i_vbi = take(VB), i_vbj = take(VB), i_imn = take(nav::IMU_SLOTS * (size_t)I), i_imm = take(I);
    total_ints = at;
    hd.assign(upload_doubles + (size_t)PRIOR_STRIDE * P + (size_t)BETWEEN_STRIDE * Q + (size_t)Q, 0.0);
    hi.assign(total_ints + (size_t)tri(N), 0);  // (the tail: build_lists' cursors)
    for (int f = 0; f < F; f++) {
      hi[i_ft + f] = target_pose[f];
      hi[i_fs + f] = source_pose[f];
    }
    for (int p = 0; p < P; p++) {
      hi[i_pk + p] = priors[p].pose;
      memcpy(&hd[o_pT + 12 * (size_t)p], priors[p].T, 12 * sizeof(double));
      memcpy(&hd[o_pL + 36 * (size_t)p], priors[p].information, 36 * sizeof(double));
    }
    for (int q = 0; q < Q; q++) {
      hi[i_bi + q] = betweens[q].pose_i;
      hi[i_bj + q] = betweens[q].pose_j;
      memcpy(&hd[o_bT + 12 * (size_t)q], betweens[q].T, 12 * sizeof(double));
      memcpy(&hd[o_bL + 36 * (size_t)q], betweens[q].information, 36 * sizeof(double));
      if (widths) hd[o_bw + q] = more->between_huber_width[q];
    }
    for (int d = 0; d < D; d++) {
      hi[i_dk + d] = more->dampings[d].pose;
      memcpy(&hd[o_dd + 6 * (size_t)d], more->dampings[d].diagonal, 6 * sizeof(double));
    }
    for (int k = 0; kinds && k < N; k++) hi[i_kind + k] = nav->kinds[k];
    for (int p = 0; p < VP; p++) {
      hi[i_vpk + p] = nav->vector_priors[p].node;
      memcpy(&hd[o_vpv + 6 * (size_t)p], nav->vector_priors[p].value, 6 * sizeof(double));
      memcpy(&hd[o_vpL + 36 * (size_t)p], nav->vector_priors[p].information, 36 * sizeof(double));
    }
    for (int q = 0; q < VB; q++) {
      hi[i_vbi + q] = nav->vector_betweens[q].node_i;
      hi[i_vbj + q] = nav->vector_betweens[q].node_j;
      memcpy(&hd[o_vbd + 6 * (size_t)q], nav->vector_betweens[q].measurement, 6 * sizeof(double));
      memcpy(&hd[o_vbL + 36 * (size_t)q], nav->vector_betweens[q].information, 36 * sizeof(double));
    }
    for (int q = 0; q < I; q++) {
      const glim_amd_nav_imu_term& e = nav->imu_terms[q];
      const int nodes[nav::IMU_SLOTS] = {e.pose_i, e.velocity_i, e.pose_j, e.velocity_j, e.bias};
      for (int u = 0; u < nav::IMU_SLOTS; u++) hi[i_imn + nav::IMU_SLOTS * (size_t)q + u] = nodes[u];
      hi[i_imm + q] = e.mode;
      memcpy(&hd[o_imd + (size_t)nav::IMU_DATA * q], &e.dt, nav::IMU_DATA * sizeof(double));
    }
    Problem host = problem_at(hd.data(), hi.data(), nullptr);
    build_lists(host.g, hi.data() + i_first, hi.data() + i_items, hi.data() + total_ints);
    init(prm, X_init12, host);
  }
};

void graph_result(const bundle_lm::Scalars& sc, glim_amd_bundle_result* result) {
  memset(result, 0, sizeof(*result));
  result->cost = sc.cost;
  result->factor_cost = sc.fcost;
  result->prior_cost = sc.pcost;
  result->between_cost = sc.bcost;
  result->num_inliers = (int64_t)llround(sc.inliers);
  result->iterations = sc.iterations;
  result->trials = sc.trials;
  result->status = sc.status;
  result->lambda = sc.lambda;
}

// The sub-map bundle optimisation and the global-graph optimisation: one host scaffold.  A round is vgicp_batch_round over the F factors, all
// behind the problem's ONE status word (stride 0), and then either the bundle decide kernel (one workgroup, the system in LDS) or the graph's
// launches (graph_round: the system in device memory); both leave the next round's T_f in the batch's pose buffer.  trace: the four arrays of
// the diag entry, or all null.  chunk: rounds enqueued between two looks at the status; 0: all of them up front and ONE synchronisation.  The
// state lives on the device: the chunk length moves no bit of a result.
int run_bundle_align(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const int32_t* target_pose,
                     const int32_t* source_pose, int32_t F, uint32_t flags, const glim_amd_bundle_prior* priors, int32_t P, const glim_amd_bundle_between* betweens,
                     int32_t Q, const double* X_init12, int32_t N, const glim_amd_lm_params* params, double* X_out12, double* compact_out,
                     glim_amd_bundle_result* result, int one_thread, const BundleTrace& trace_host, bool graph = false, int chunk = 0,
                     const glim_amd_graph_terms* more = nullptr, double* between_weight_out = nullptr, const glim_amd_nav_terms* nav = nullptr,
                     glim_amd_nav_result* nav_result = nullptr) {
  using namespace bundle_lm;
  if (N < 0 || F < 0 || P < 0 || Q < 0) return GLIM_AMD_ERR_INVALID;
  if (N == 0) return GLIM_AMD_OK;
  lm::Params prm;
  int rounds;
  const GraphCaps caps = graph ? GraphCaps{GLIM_AMD_GRAPH_MAX_POSES, GLIM_AMD_GRAPH_MAX_FACTORS, GLIM_AMD_GRAPH_MAX_TERMS} : GraphCaps{MAX_POSES, MAX_FACTORS, MAX_TERMS};
  GA_TRY(check_graph_args(ctx, targets, sources, target_pose, source_pose, F, flags, priors, P, betweens, Q, X_init12, N, params, X_out12, result, caps, &prm,
                          &rounds, more, nav));
  const GraphBlocks blk(N, F, P, Q, target_pose, source_pose, priors, betweens, more, X_init12, prm, graph ? graph_scratch_doubles(6 * N) : 0, nav);

  std::unique_lock<std::mutex> held(ctx->mu);  // once for the call
  GA_HIP(hipSetDevice(ctx->device));
  VgicpBatch batch;  // (destroyed last: its plan goes back after the stream has been waited for)
  DeviceTemp d_d, d_i;
  TraceBuffer tX, tTf, trec, trounds;
  hipStream_t st = ctx->stream();
  if (F > 0) {
    GA_TRY(vgicp_batch_open(ctx, targets, sources, flags, F, &batch));
    st = batch.stream();
  }
  SyncOnExit in_flight(st);  // an error exit after the launches waits for the stream before the scratch goes back to the pool
  GA_HIP(pool_malloc(&d_d.p, std::max<size_t>(1, blk.total_doubles) * sizeof(double)));
  GA_HIP(pool_malloc(&d_i.p, std::max<size_t>(1, blk.total_ints) * sizeof(int)));
  if (trace_host.rounds) {  // (the entry point has seen to it that the arrays the graph needs come together)
    GA_TRY(tX.open(trace_host.X, (size_t)rounds * 12 * N * sizeof(double), st));
    GA_TRY(tTf.open(trace_host.Tf, (size_t)rounds * 12 * F * sizeof(double), st));
    GA_TRY(trec.open(trace_host.rec, (size_t)rounds * lm::RECORD * F * sizeof(double), st));
    GA_TRY(trounds.open(trace_host.rounds, (size_t)rounds * sizeof(glim_amd_bundle_trace_round), st));
  }
  const BundleTrace tr{tX.d.as<double>(), tTf.d.as<double>(), trec.d.as<double>(), trounds.d.as<glim_amd_bundle_trace_round>()};
  GA_HIP(hipMemcpyAsync(d_d.p, blk.hd.data(), blk.upload_doubles * sizeof(double), hipMemcpyHostToDevice, st));
  if (blk.total_ints) GA_HIP(hipMemcpyAsync(d_i.p, blk.hi.data(), blk.total_ints * sizeof(int), hipMemcpyHostToDevice, st));
  Problem pr = blk.problem_at(d_d.as<double>(), d_i.as<int>(), F > 0 ? batch.poses() : d_d.as<double>() + blk.o_Tf0);
  const GraphScratch gs = graph_scratch_at(d_d.as<double>() + blk.o_extra, 6 * N);
  if (graph) {
    pr.W = gs.E;
    GA_HIP(hipMemsetAsync(gs.words, 0, sizeof(GraphWords), st));
  }
  const int* d_status = reinterpret_cast<const int*>(reinterpret_cast<const char*>(pr.s) + offsetof(Scalars, status));
  const double* d_recs = F > 0 ? batch.records() : pr.rec;
  if (F > 0) bundle_pose_kernel<<<1, 256, 0, st>>>(pr);
  Scalars sc;
  for (int r = 0;;) {
    for (const int end = chunk > 0 ? std::min(rounds, r + chunk) : rounds; r < end; r++) {
      if (F > 0) GA_TRY(vgicp_batch_round(&batch, d_status, 0));
      if (graph) GA_TRY(graph_round(pr, gs, prm, d_recs, d_status, tr, r, one_thread, st));
      else bundle_decide_kernel<<<1, BUNDLE_THREADS, 0, st>>>(pr, prm, d_recs, tr, r, one_thread);
    }
    GA_HIP(hipGetLastError());
    GA_HIP(hipMemcpyAsync(&sc, pr.s, sizeof(sc), hipMemcpyDeviceToHost, st));
    if (r == rounds) break;
    GA_HIP(hipStreamSynchronize(st));  // a chunk's end: the loop stops enqueueing when the problem has finished
    if (sc.status != lm::RUNNING) break;
  }
  std::vector<double> rec_host((size_t)lm::RECORD * F);
  GA_HIP(hipMemcpyAsync(X_out12, pr.X, 12 * (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
  if (F > 0) GA_HIP(hipMemcpyAsync(rec_host.data(), pr.rec, rec_host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  if (between_weight_out && Q > 0) GA_HIP(hipMemcpyAsync(between_weight_out, pr.wk, (size_t)Q * sizeof(double), hipMemcpyDeviceToHost, st));
  GA_TRY(tX.fetch(st));
  GA_TRY(tTf.fetch(st));  // (nothing without factors: no bytes)
  GA_TRY(trec.fetch(st));
  GA_TRY(trounds.fetch(st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  if (F > 0) batch.seen_complete();
  if (compact_out && F > 0) memcpy(compact_out, rec_host.data(), rec_host.size() * sizeof(double));
  graph_result(sc, result);
  if (nav_result) {
    memset(nav_result, 0, sizeof(*nav_result));
    nav_result->cost = sc.cost, nav_result->factor_cost = sc.fcost, nav_result->prior_cost = sc.pcost, nav_result->between_cost = sc.bcost;
    nav_result->vector_prior_cost = sc.vpcost, nav_result->vector_between_cost = sc.vbcost, nav_result->imu_cost = sc.icost;
    nav_result->num_inliers = result->num_inliers;
    nav_result->iterations = sc.iterations, nav_result->trials = sc.trials, nav_result->status = sc.status;
    nav_result->lambda = sc.lambda;
  }
  return GLIM_AMD_OK;
}

}  // namespace

extern "C" {

int glim_amd_bundle_align_default_params(glim_amd_lm_params* params) {
  if (!params) return GLIM_AMD_ERR_INVALID;
  bundle_default_params(params);
  return GLIM_AMD_OK;
}

int glim_amd_bundle_align(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const int32_t* target_pose,
                          const int32_t* source_pose, int32_t num_factors, uint32_t flags, const glim_amd_bundle_prior* priors, int32_t num_priors,
                          const glim_amd_bundle_between* betweens, int32_t num_betweens, const double* X_init12, int32_t num_poses,
                          const glim_amd_lm_params* params, double* X_out12, double* compact_out, glim_amd_bundle_result* result) {
  return run_bundle_align(ctx, targets, sources, target_pose, source_pose, num_factors, flags, priors, num_priors, betweens, num_betweens, X_init12, num_poses,
                          params, X_out12, compact_out, result, 0, BundleTrace{nullptr, nullptr, nullptr, nullptr});
}

int glim_amd_debug_bundle_align_trace(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources,
                                      const int32_t* target_pose, const int32_t* source_pose, int32_t num_factors, uint32_t flags,
                                      const glim_amd_bundle_prior* priors, int32_t num_priors, const glim_amd_bundle_between* betweens,
                                      int32_t num_betweens, const double* X_init12, int32_t num_poses, const glim_amd_lm_params* params,
                                      double* X_out12, double* compact_out, glim_amd_bundle_result* result, int32_t one_thread, double* X_trace,
                                      double* Tf_trace, double* compact_trace, glim_amd_bundle_trace_round* rounds) {
  const bool any = X_trace || Tf_trace || compact_trace || rounds;
  if (any && num_poses > 0 && (!X_trace || !rounds || (num_factors > 0 && (!Tf_trace || !compact_trace)))) return GLIM_AMD_ERR_INVALID;
  return run_bundle_align(ctx, targets, sources, target_pose, source_pose, num_factors, flags, priors, num_priors, betweens, num_betweens, X_init12, num_poses,
                          params, X_out12, compact_out, result, one_thread ? 1 : 0, BundleTrace{X_trace, Tf_trace, compact_trace, rounds});
}

int glim_amd_graph_align_default_params(glim_amd_lm_params* params) { return glim_amd_bundle_align_default_params(params); }

int glim_amd_graph_align(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const int32_t* target_pose,
                         const int32_t* source_pose, int32_t num_factors, uint32_t flags, const glim_amd_bundle_prior* priors, int32_t num_priors,
                         const glim_amd_bundle_between* betweens, int32_t num_betweens, const double* X_init12, int32_t num_poses,
                         const glim_amd_lm_params* params, double* X_out12, double* compact_out, glim_amd_bundle_result* result) {
  return run_bundle_align(ctx, targets, sources, target_pose, source_pose, num_factors, flags, priors, num_priors, betweens, num_betweens, X_init12, num_poses,
                          params, X_out12, compact_out, result, 0, BundleTrace{nullptr, nullptr, nullptr, nullptr}, true, GRAPH_ROUNDS_PER_CHUNK);
}

int glim_amd_debug_graph_align_trace(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources,
                                     const int32_t* target_pose, const int32_t* source_pose, int32_t num_factors, uint32_t flags,
                                     const glim_amd_bundle_prior* priors, int32_t num_priors, const glim_amd_bundle_between* betweens,
                                     int32_t num_betweens, const double* X_init12, int32_t num_poses, const glim_amd_lm_params* params,
                                     double* X_out12, double* compact_out, glim_amd_bundle_result* result, int32_t one_thread, double* X_trace,
                                     double* Tf_trace, double* compact_trace, glim_amd_bundle_trace_round* rounds, int32_t rounds_per_chunk) {
  const bool any = X_trace || Tf_trace || compact_trace || rounds;
  if (any && num_poses > 0 && (!X_trace || !rounds || (num_factors > 0 && (!Tf_trace || !compact_trace)))) return GLIM_AMD_ERR_INVALID;
  if (rounds_per_chunk < 0) return GLIM_AMD_ERR_INVALID;
  return run_bundle_align(ctx, targets, sources, target_pose, source_pose, num_factors, flags, priors, num_priors, betweens, num_betweens, X_init12, num_poses,
                          params, X_out12, compact_out, result, one_thread ? 1 : 0, BundleTrace{X_trace, Tf_trace, compact_trace, rounds}, true,
                          rounds_per_chunk > 0 ? rounds_per_chunk : GRAPH_ROUNDS_PER_CHUNK);
}

// the two loops with damping terms and Huber widths: the same scaffold, the terms behind the graph
int glim_amd_bundle_align_terms(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const int32_t* target_pose,
                                const int32_t* source_pose, int32_t num_factors, uint32_t flags, const glim_amd_bundle_prior* priors, int32_t num_priors,
                                const glim_amd_bundle_between* betweens, int32_t num_betweens, const double* X_init12, int32_t num_poses,
                                const glim_amd_lm_params* params, double* X_out12, double* compact_out, glim_amd_bundle_result* result,
                                const glim_amd_graph_terms* more, double* between_weight_out) {
  return run_bundle_align(ctx, targets, sources, target_pose, source_pose, num_factors, flags, priors, num_priors, betweens, num_betweens, X_init12, num_poses,
                          params, X_out12, compact_out, result, 0, BundleTrace{nullptr, nullptr, nullptr, nullptr}, false, 0, more, between_weight_out);
}

int glim_amd_debug_bundle_align_terms_trace(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources,
                                            const int32_t* target_pose, const int32_t* source_pose, int32_t num_factors, uint32_t flags,
                                            const glim_amd_bundle_prior* priors, int32_t num_priors, const glim_amd_bundle_between* betweens,
                                            int32_t num_betweens, const double* X_init12, int32_t num_poses, const glim_amd_lm_params* params,
                                            double* X_out12, double* compact_out, glim_amd_bundle_result* result, const glim_amd_graph_terms* more,
                                            double* between_weight_out, int32_t one_thread, double* X_trace, double* Tf_trace, double* compact_trace,
                                            glim_amd_bundle_trace_round* rounds) {
  const bool any = X_trace || Tf_trace || compact_trace || rounds;
  if (any && num_poses > 0 && (!X_trace || !rounds || (num_factors > 0 && (!Tf_trace || !compact_trace)))) return GLIM_AMD_ERR_INVALID;
  return run_bundle_align(ctx, targets, sources, target_pose, source_pose, num_factors, flags, priors, num_priors, betweens, num_betweens, X_init12, num_poses,
                          params, X_out12, compact_out, result, one_thread ? 1 : 0, BundleTrace{X_trace, Tf_trace, compact_trace, rounds}, false, 0, more,
                          between_weight_out);
}

int glim_amd_graph_align_terms(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const int32_t* target_pose,
                               const int32_t* source_pose, int32_t num_factors, uint32_t flags, const glim_amd_bundle_prior* priors, int32_t num_priors,
                               const glim_amd_bundle_between* betweens, int32_t num_betweens, const double* X_init12, int32_t num_poses,
                               const glim_amd_lm_params* params, double* X_out12, double* compact_out, glim_amd_bundle_result* result,
                               const glim_amd_graph_terms* more, double* between_weight_out) {
  return run_bundle_align(ctx, targets, sources, target_pose, source_pose, num_factors, flags, priors, num_priors, betweens, num_betweens, X_init12, num_poses,
                          params, X_out12, compact_out, result, 0, BundleTrace{nullptr, nullptr, nullptr, nullptr}, true, GRAPH_ROUNDS_PER_CHUNK, more,
                          between_weight_out);
}

int glim_amd_debug_graph_align_terms_trace(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources,
                                           const int32_t* target_pose, const int32_t* source_pose, int32_t num_factors, uint32_t flags,
                                           const glim_amd_bundle_prior* priors, int32_t num_priors, const glim_amd_bundle_between* betweens,
                                           int32_t num_betweens, const double* X_init12, int32_t num_poses, const glim_amd_lm_params* params,
                                           double* X_out12, double* compact_out, glim_amd_bundle_result* result, const glim_amd_graph_terms* more,
                                           double* between_weight_out, int32_t one_thread, double* X_trace, double* Tf_trace, double* compact_trace,
                                           glim_amd_bundle_trace_round* rounds, int32_t rounds_per_chunk) {
  const bool any = X_trace || Tf_trace || compact_trace || rounds;
  if (any && num_poses > 0 && (!X_trace || !rounds || (num_factors > 0 && (!Tf_trace || !compact_trace)))) return GLIM_AMD_ERR_INVALID;
  if (rounds_per_chunk < 0) return GLIM_AMD_ERR_INVALID;
  return run_bundle_align(ctx, targets, sources, target_pose, source_pose, num_factors, flags, priors, num_priors, betweens, num_betweens, X_init12, num_poses,
                          params, X_out12, compact_out, result, one_thread ? 1 : 0, BundleTrace{X_trace, Tf_trace, compact_trace, rounds}, true,
                          rounds_per_chunk > 0 ? rounds_per_chunk : GRAPH_ROUNDS_PER_CHUNK, more, between_weight_out);
}

// the global graph with node kinds, vector priors, vector betweens and IMU terms (sub_mapping.cpp:218-243, global_mapping.cpp:168-216, 976-1042,
// odometry_estimation_imu.cpp:218-220, 268-283, loose_initial_state_estimation.cpp:105-124, 174): the same scaffold, the terms behind the graph
int glim_amd_graph_align_nav(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const int32_t* target_pose,
                             const int32_t* source_pose, int32_t num_factors, uint32_t flags, const glim_amd_bundle_prior* priors, int32_t num_priors,
                             const glim_amd_bundle_between* betweens, int32_t num_betweens, const double* X_init12, int32_t num_poses,
                             const glim_amd_lm_params* params, double* X_out12, double* compact_out, glim_amd_nav_result* result,
                             const glim_amd_graph_terms* more, double* between_weight_out, const glim_amd_nav_terms* nav) {
  if (!result) return GLIM_AMD_ERR_INVALID;
  glim_amd_bundle_result base;
  return run_bundle_align(ctx, targets, sources, target_pose, source_pose, num_factors, flags, priors, num_priors, betweens, num_betweens, X_init12, num_poses,
                          params, X_out12, compact_out, &base, 0, BundleTrace{nullptr, nullptr, nullptr, nullptr}, true, GRAPH_ROUNDS_PER_CHUNK, more,
                          between_weight_out, nav, result);
}

int glim_amd_debug_graph_align_nav_trace(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources,
                                         const int32_t* target_pose, const int32_t* source_pose, int32_t num_factors, uint32_t flags,
                                         const glim_amd_bundle_prior* priors, int32_t num_priors, const glim_amd_bundle_between* betweens,
                                         int32_t num_betweens, const double* X_init12, int32_t num_poses, const glim_amd_lm_params* params,
                                         double* X_out12, double* compact_out, glim_amd_nav_result* result, const glim_amd_graph_terms* more,
                                         double* between_weight_out, const glim_amd_nav_terms* nav, int32_t one_thread, double* X_trace,
                                         double* Tf_trace, double* compact_trace, glim_amd_bundle_trace_round* rounds, int32_t rounds_per_chunk) {
  const bool any = X_trace || Tf_trace || compact_trace || rounds;
  if (any && num_poses > 0 && (!X_trace || !rounds || (num_factors > 0 && (!Tf_trace || !compact_trace)))) return GLIM_AMD_ERR_INVALID;
  if (rounds_per_chunk < 0 || !result) return GLIM_AMD_ERR_INVALID;
  glim_amd_bundle_result base;
  return run_bundle_align(ctx, targets, sources, target_pose, source_pose, num_factors, flags, priors, num_priors, betweens, num_betweens, X_init12, num_poses,
                          params, X_out12, compact_out, &base, one_thread ? 1 : 0, BundleTrace{X_trace, Tf_trace, compact_trace, rounds}, true,
                          rounds_per_chunk > 0 ? rounds_per_chunk : GRAPH_ROUNDS_PER_CHUNK, more, between_weight_out, nav, result);
}

int glim_amd_debug_graph_solve(glim_amd_ctx* ctx, const double* S, int32_t n, double lambda, double* delta_out, int32_t* ok_out) {
  if (!ctx || !S || !delta_out || !ok_out || n < 1 || n > graph_solve::MAX_DIM || !std::isfinite(lambda)) return GLIM_AMD_ERR_INVALID;
  const size_t nsys = (size_t)bundle_lm::system_doubles(n), nm = graph_solve::matrix_doubles(n);
  std::unique_lock<std::mutex> held(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  DeviceTemp d;  // the system, the matrix, delta, then the two words (fail, a status that stays 0)
  SyncOnExit in_flight(st);
  GA_HIP(pool_malloc(&d.p, (nsys + nm + n + 1) * sizeof(double)));
  double *d_S = d.as<double>(), *d_M = d_S + nsys, *d_delta = d_M + nm;
  int* d_words = reinterpret_cast<int*>(d_delta + n);
  GA_HIP(hipMemcpyAsync(d_S, S, nsys * sizeof(double), hipMemcpyHostToDevice, st));
  GA_HIP(hipMemsetAsync(d_words, 0, 2 * sizeof(int), st));
  graph_load_kernel<<<dim3((n + GRAPH_THREADS - 1) / GRAPH_THREADS, n + 1), GRAPH_THREADS, 0, st>>>(d_S, n, lambda, d_M);
  GA_HIP(graph_solve_enqueue(st, d_M, n, d_delta, d_words, d_words + 1));
  int fail = 0;
  GA_HIP(hipMemcpyAsync(delta_out, d_delta, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  GA_HIP(hipMemcpyAsync(&fail, d_words, sizeof(int), hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  *ok_out = fail ? 0 : 1;
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

int glim_amd_keyframe_align_default_params(glim_amd_lm_params* params) {
  if (!params) return GLIM_AMD_ERR_INVALID;
  lm_default_params(params);
  return GLIM_AMD_OK;
}

int glim_amd_keyframe_align_batch(const glim_amd_cloud* const* sources, const int32_t* first_target, const glim_amd_voxelmap* const* targets,
                                  const double* T_world_target12, const double* X_init12, const glim_amd_bundle_prior* priors, int32_t num_priors, uint32_t flags,
                                  int32_t count, const glim_amd_lm_params* params, glim_amd_align_result* out, double* factor_compact_out) {
  return run_keyframe_align(sources, first_target, targets, T_world_target12, X_init12, priors, num_priors, flags, count, params, out, factor_compact_out,
                            KeyframeTrace{nullptr, nullptr, nullptr, nullptr});
}

int glim_amd_debug_keyframe_align_trace(const glim_amd_cloud* const* sources, const int32_t* first_target, const glim_amd_voxelmap* const* targets,
                                        const double* T_world_target12, const double* X_init12, const glim_amd_bundle_prior* priors, int32_t num_priors,
                                        uint32_t flags, int32_t count, const glim_amd_lm_params* params, glim_amd_align_result* out, double* factor_compact_out,
                                        glim_amd_align_trace_entry* rounds, double* prior_trace, double* Tf_trace, double* compact_trace) {
  if (count > 0 && (!rounds || !prior_trace || !Tf_trace || !compact_trace)) return GLIM_AMD_ERR_INVALID;
  return run_keyframe_align(sources, first_target, targets, T_world_target12, X_init12, priors, num_priors, flags, count, params, out, factor_compact_out,
                            KeyframeTrace{rounds, prior_trace, Tf_trace, compact_trace});
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

int glim_amd_icp_align_default_params(glim_amd_lm_params* params) {
  if (!params) return GLIM_AMD_ERR_INVALID;
  icp_default_params(params);
  return GLIM_AMD_OK;
}

int glim_amd_icp_align_batch(const glim_amd_nn_index* const* targets, const glim_amd_cloud* const* sources, const double* T_init12,
                             const double* max_correspondence_distances, uint32_t flags, int32_t count, const glim_amd_lm_params* params,
                             glim_amd_align_result* out) {
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
