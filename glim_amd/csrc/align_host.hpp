// align_host.hpp -- what the on-device Levenberg-Marquardt loops share on the host (gicp_align.hip, vgicp_align.hip, ct_align.hip,
// bundle_align.hip): the parameters and their defaults, the refusals every loop answers alike, the trace arrays, the result of a six-parameter
// problem, and the one device function the six-parameter decide kernels share.  The scheme they all follow (problem table, block table, a round,
// the call, chunks) is stated once, in gicp_align.hip's opening comment.  Like gicp_factor.hpp and knn_common.hpp the shared part is in an
// unnamed namespace: each unit gets its own few lines, nothing of it is called across units.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "internal.hpp"
#include "lm_step.hpp"
#include "scope_sync.hpp"

namespace {

using namespace glim_amd;

static_assert(sizeof(lm::Params) == sizeof(glim_amd_lm_params), "lm::Params is the layout of glim_amd_lm_params");
static_assert(offsetof(lm::Params, error_scale) == offsetof(glim_amd_lm_params, error_scale), "lm::Params is the layout of glim_amd_lm_params");
static_assert(lm::RECORD == COMPACT, "the compact record");
static_assert(lm::CONVERGED == GLIM_AMD_ALIGN_CONVERGED && lm::MAX_ITERATIONS == GLIM_AMD_ALIGN_MAX_ITERATIONS && lm::MAX_TRIALS == GLIM_AMD_ALIGN_MAX_TRIALS &&
                  lm::LAMBDA_BOUND == GLIM_AMD_ALIGN_LAMBDA_BOUND && lm::NO_CORRESPONDENCES == GLIM_AMD_ALIGN_NO_CORRESPONDENCES &&
                  lm::NUMERIC == GLIM_AMD_ALIGN_NUMERIC,
              "status values");
constexpr int ALIGN_MAX_TRIALS = 4096;

// what the decide kernels of the six-parameter loops do with a problem's record, in one thread: the step rule on the state, and the round's
// trace entry when a trace was asked for (`entry`: the problem's entry of this round, or null).  s: the state after the round
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

bool lm_params_ok(const glim_amd_lm_params& p) {
  const double v[] = {p.lambda_initial, p.lambda_factor, p.lambda_upper_bound, p.lambda_lower_bound, p.relative_error_tol, p.absolute_error_tol, p.error_scale};
  for (double x : v)
    if (!std::isfinite(x)) return false;
  return p.lambda_factor > 1.0 && p.lambda_initial >= 0.0 && p.error_scale > 0.0 && p.max_iterations >= 0 && p.max_trials >= 0 && p.max_trials <= ALIGN_MAX_TRIALS &&
         p.max_iterations <= ALIGN_MAX_TRIALS;
}

void lm_default_params(glim_amd_lm_params* p) {
  memset(p, 0, sizeof(*p));
  p->lambda_initial = 1e-5, p->lambda_factor = 10.0, p->lambda_upper_bound = 1e5, p->lambda_lower_bound = 0.0;
  p->relative_error_tol = 1e-5, p->absolute_error_tol = 1e-5, p->error_scale = 1.0;
  p->max_iterations = 10, p->max_trials = 0;
}

// what every glim_amd_*_align_default_params answers, with its loop's defaults
int default_params_out(glim_amd_lm_params* params, void (*defaults)(glim_amd_lm_params*)) {
  if (!params) return GLIM_AMD_ERR_INVALID;
  defaults(params);
  return GLIM_AMD_OK;
}

bool all_finite_host(const double* v, int n) {
  for (int k = 0; k < n; k++)
    if (!std::isfinite(v[k])) return false;
  return true;
}

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
  o->error = s.rec[1], o->num_inliers = (int64_t)llround(s.rec[0]);
  o->iterations = s.iterations, o->trials = s.trials, o->status = s.status, o->lambda = s.lambda;
}

}  // namespace
