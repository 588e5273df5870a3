// registration_host.hpp -- the host scaffold the global-registration entries share (ransac.hip, gnc.hip): the argument checks, the two ways a
// correspondence list reaches the device (uploaded from the host, or matched there from two descriptor sets), the "nothing estimated" result and
// the HIP-event clock of the profile entries.  Host code only; with_matched_nearest uses fpfh.hip's descriptor object and matcher (fpfh.hpp).
#pragma once
#include <cstring>
#include <mutex>

#include "fpfh.hpp"
#include "internal.hpp"
#include "scope_sync.hpp"

namespace glim_amd {
namespace reg_detail {

constexpr int64_t MAX_POINTS = (int64_t)1 << 27;

// two clouds of one context and the correspondence list between them, on the device: what an estimator works on beside its own parameters
struct Pair {
  glim_amd_ctx* ctx;
  hipStream_t st;
  int n_src, n_tgt;
  const float4 *spts, *tpts;
  const int* d_nearest;  // n_src entries: a target index or -1
};

inline int check_pair(const glim_amd_cloud* target, const glim_amd_cloud* source) {
  if (!target || !source) return GLIM_AMD_ERR_INVALID;
  if ((glim_amd_ctx*)target->ctx != (glim_amd_ctx*)source->ctx) return GLIM_AMD_ERR_INVALID;
  if (target->n > MAX_POINTS || source->n > MAX_POINTS) return GLIM_AMD_ERR_INVALID;
  return GLIM_AMD_OK;
}
inline int check_nearest(const int32_t* nearest, int64_t n_src, int64_t n_tgt) {
  if (!nearest && n_src > 0) return GLIM_AMD_ERR_INVALID;
  for (int64_t i = 0; i < n_src; i++)
    if (nearest[i] < -1 || (int64_t)nearest[i] >= n_tgt) return GLIM_AMD_ERR_INVALID;
  return GLIM_AMD_OK;
}
// the arguments of a *_fpfh entry beside its parameter block: the handles, one context, the flags, one descriptor per point.  (Every refusal,
// here and in the entries' check_params, is GLIM_AMD_ERR_INVALID: which of them is looked at first cannot be seen from outside.)
inline int check_fpfh_pair(const glim_amd_cloud* target, const glim_amd_cloud* source, const glim_amd_fpfh* target_fpfh,
                           const glim_amd_fpfh* source_fpfh, uint32_t flags) {
  if (!target_fpfh || !source_fpfh) return GLIM_AMD_ERR_INVALID;
  GA_TRY(check_pair(target, source));
  glim_amd_ctx* ctx = source->ctx;
  if ((glim_amd_ctx*)target_fpfh->ctx != ctx || (glim_amd_ctx*)source_fpfh->ctx != ctx) return GLIM_AMD_ERR_INVALID;
  if (flags & ~(uint32_t)GLIM_AMD_FPFH_RECIPROCAL) return GLIM_AMD_ERR_INVALID;
  if (target_fpfh->n != target->n || source_fpfh->n != source->n) return GLIM_AMD_ERR_INVALID;
  return GLIM_AMD_OK;
}

// `nearest` from the host: locks the context, uploads the list (nothing to upload for an empty source), synchronises and returns fn(pair).
// The arguments have passed check_pair and check_nearest.
template <class Fn>
int with_host_nearest(const glim_amd_cloud* target, const glim_amd_cloud* source, const int32_t* nearest, Fn&& fn) {
  glim_amd_ctx* ctx = source->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  DeviceTemp d_nearest;
  if (source->n > 0) {
    GA_HIP(pool_malloc(&d_nearest.p, (size_t)source->n * sizeof(int)));
    GA_HIP(hipMemcpyAsync(d_nearest.p, nearest, (size_t)source->n * sizeof(int), hipMemcpyHostToDevice, st));
    GA_HIP(hipStreamSynchronize(st));
  }
  return fn(Pair{ctx, st, (int)source->n, (int)target->n, source->pts, target->pts, d_nearest.as<int>()});
}

// `nearest` matched on the device from the two descriptor sets (both non-empty): locks the context, runs the matcher, synchronises and returns
// fn(pair).  The match buffers outlive fn: its kernels read `nearest`.
template <class Fn>
int with_matched_nearest(const glim_amd_cloud* target, const glim_amd_cloud* source, const glim_amd_fpfh* target_fpfh,
                         const glim_amd_fpfh* source_fpfh, uint32_t flags, Fn&& fn) {
  glim_amd_ctx* ctx = source->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  GA_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream();
  fpfh_detail::MatchBuffers m;
  {
    SyncOnExit in_flight(st);
    GA_TRY(fpfh_detail::enqueue_match_both(ctx, st, target_fpfh, source_fpfh, flags, &m));
    GA_HIP(hipStreamSynchronize(st));
    in_flight.dismiss();
  }
  return fn(Pair{ctx, st, (int)source->n, (int)target->n, source->pts, target->pts, m.fwd_i.as<int>()});
}

// the result of a call that estimated nothing: the identity, no inliers, no best iteration
inline void identity_result(glim_amd_registration_result* r, int iterations_run) {
  const double I[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  std::memcpy(r->T_target_source, I, sizeof(I));
  r->inlier_rate = 0.0;
  r->num_inliers = 0;
  r->best_iteration = -1;
  r->iterations_run = iterations_run;
}

// HIP events at the N boundaries of N - 1 stages (the profile entries).  mark() does nothing before start(): a run that is not timed passes
// an idle clock.
template <int N>
struct StageClock {
  hipEvent_t ev[N] = {};
  bool on = false;
  int start() {
    for (auto& e : ev) GA_HIP(hipEventCreate(&e));
    on = true;
    return GLIM_AMD_OK;
  }
  void mark(int i, hipStream_t st) {
    if (on) (void)hipEventRecord(ev[i], st);
  }
  // microseconds of stage k of the last synchronised run, added to *sum
  hipError_t add_us(int k, double* sum) const {
    float ms = 0.0f;
    const hipError_t e = hipEventElapsedTime(&ms, ev[k], ev[k + 1]);
    *sum += (double)ms * 1e3;
    return e;
  }
  ~StageClock() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

}  // namespace reg_detail
}  // namespace glim_amd
