// bundle_align.hip -- the N-pose Levenberg-Marquardt loops on gfx950: the sub-map bundle optimisation and the global-graph optimisation.  The
// scheme is gicp_align.hip's, the host scaffold align_host.hpp's; the rule is bundle_lm_step.hpp's.  This is the only unit that includes the
// rule directly (vgicp_align.hip reaches it through the keyframe rule's header, for the prior's term products).
//
// The sub-map bundle optimisation (include/glim_amd.h "Sub-map bundle optimisation") is the scheme over N poses and F binary VGICP factors:
// a round is vgicp_batch_round over the F factors at the candidate's relative poses, all behind the problem's one status word, and the bundle
// decide kernel: one workgroup that expands the records, assembles the dense 6N x 6N system, factorises it in LDS, retracts the poses and
// writes the next round's relative poses, every value by the item functions of bundle_lm_step.hpp.
//
// The global-graph optimisation (include/glim_amd.h "Global-graph optimisation") is the bundle at up to 256 poses with the systems in device
// memory and the decide step as a sequence of launches (below).  Its rounds are enqueued a few at a time, as the ICP loop's are.  With node
// kinds it also carries velocity and bias nodes, vector terms and IMU terms (nav_terms.hpp).
//
// Both take damping terms and Huber widths of the between terms (include/glim_amd.h "Damping terms and Huber between terms") through the same
// item functions: the two arrays live in device memory beside the graph, and so do the betweens' weights -- those of a round's evaluation, and
// those of the kept evaluation, which the kernel that keeps a candidate's poses and records copies with them.
#include "align_host.hpp"
#include "bundle_lm_step.hpp"
#include "graph_solve.hpp"
#include "vgicp_batch.hpp"

namespace {

// ---- the sub-map bundle optimisation ----
static_assert(sizeof(glim_amd_linearized6) == 122 * sizeof(double), "a factor's blocks, in doubles");
static_assert(sizeof(bundle_lm::Scalars) % sizeof(double) == 0 && offsetof(bundle_lm::Scalars, status) % sizeof(int) == 0, "the scalars of a state");
static_assert(bundle_lm::MAX_POSES == GLIM_AMD_BUNDLE_MAX_POSES && bundle_lm::MAX_FACTORS == GLIM_AMD_BUNDLE_MAX_FACTORS &&
                  bundle_lm::MAX_TERMS == GLIM_AMD_BUNDLE_MAX_TERMS,
              "the caps");
constexpr int BUNDLE_THREADS = 512;
static_assert(BUNDLE_THREADS > bundle_lm::MAX_DIM, "a thread per row of the solve, the right-hand side included");
static_assert(2 * bundle_lm::MAX_FACTORS + 2 * bundle_lm::MAX_TERMS <= bundle_lm::MAX_SYSTEM, "the cost sums are staged where the system is assembled afterwards");

struct BundleTrace {  // the arrays of the diag entry (the caller's, or their device copies), or all null
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
// GraphWords.  The solve's matrix is graph_solve.hpp's and its launches are graph_solve.hip's.
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

void bundle_default_params(glim_amd_lm_params* p) {
  lm_default_params(p);
  p->max_iterations = 20;
}

// ---- the host scaffold of the two N-pose loops (the sub-map bundle, the global graph) ----
// The arguments of one call, under the names the C ABI gives them (include/glim_amd.h, include/glim_amd_diag.h): every entry point fills its
// own by name.  The first rows are what every entry point has; what only some have keeps its default here (result or nav_result takes the
// result; graph: the global graph, not the sub-map bundle; rounds_per_chunk: the graph's, 0 = GRAPH_ROUNDS_PER_CHUNK)
struct BundleCall {
  glim_amd_ctx* ctx;
  const glim_amd_voxelmap* const* targets;
  const glim_amd_cloud* const* sources;
  const int32_t *target_pose, *source_pose;
  int32_t num_factors, num_priors, num_betweens, num_poses;
  uint32_t flags;
  const glim_amd_bundle_prior* priors;
  const glim_amd_bundle_between* betweens;
  const double* X_init12;
  const glim_amd_lm_params* params;
  double *X_out12, *compact_out, *between_weight_out = nullptr;
  glim_amd_bundle_result* result = nullptr;
  glim_amd_nav_result* nav_result = nullptr;
  BundleTrace trace{};
  int32_t one_thread = 0, rounds_per_chunk = 0;
  bool graph = false;
  const glim_amd_graph_terms* more = nullptr;
  const glim_amd_nav_terms* nav = nullptr;
};

// the trace arrays come together: none, or all that the problem fills
bool trace_arrays_ok(const BundleCall& c) {
  const BundleTrace& t = c.trace;
  return !((t.X || t.Tf || t.rec || t.rounds) && c.num_poses > 0 && (!t.X || !t.rounds || (c.num_factors > 0 && (!t.Tf || !t.rec))));
}

// rounds enqueued between two looks at the status: the bundle's 0 (all of them up front and ONE synchronisation), the graph's own or its
// default; -1: rounds_per_chunk is negative
int chunk_rounds(const BundleCall& c) {
  return c.rounds_per_chunk < 0 ? -1 : !c.graph ? 0 : c.rounds_per_chunk > 0 ? c.rounds_per_chunk : GRAPH_ROUNDS_PER_CHUNK;
}

// the refusals of glim_amd_graph_align_nav's node kinds and new terms (the counts and the arrays have been looked at)
int check_nav_args(const BundleCall& c) {
  const glim_amd_nav_terms& nav = *c.nav;
  const int N = c.num_poses;
  const double* X = c.X_init12;
  auto kind = [&](int k) { return nav.kinds ? nav.kinds[k] : GLIM_AMD_NODE_POSE; };
  auto is = [&](int k, int want) { return k >= 0 && k < N && kind(k) == want; };
  auto vector_kind = [&](int k) { return is(k, GLIM_AMD_NODE_BIAS) || is(k, GLIM_AMD_NODE_VELOCITY); };
  for (int k = 0; k < N; k++) {
    const int kd = kind(k);
    if (kd != GLIM_AMD_NODE_POSE && kd != GLIM_AMD_NODE_BIAS && kd != GLIM_AMD_NODE_VELOCITY) return GLIM_AMD_ERR_INVALID;
    for (int u = kd == GLIM_AMD_NODE_POSE ? 12 : nav::node_dim(kd); u < 12; u++)
      if (X[12 * k + u] != 0.0 || std::signbit(X[12 * k + u])) return GLIM_AMD_ERR_INVALID;
  }
  for (int f = 0; f < c.num_factors; f++)
    if (!is(c.target_pose[f], GLIM_AMD_NODE_POSE) || !is(c.source_pose[f], GLIM_AMD_NODE_POSE)) return GLIM_AMD_ERR_INVALID;
  for (int p = 0; p < c.num_priors; p++)
    if (!is(c.priors[p].pose, GLIM_AMD_NODE_POSE)) return GLIM_AMD_ERR_INVALID;
  for (int q = 0; q < c.num_betweens; q++)
    if (!is(c.betweens[q].pose_i, GLIM_AMD_NODE_POSE) || !is(c.betweens[q].pose_j, GLIM_AMD_NODE_POSE)) return GLIM_AMD_ERR_INVALID;
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

// the refusals of glim_amd_bundle_align with the loop's caps: everything that is answered before a handle or the context is used, then the
// pairs.  GLIM_AMD_OK with N == 0 is the caller's to answer first
int check_graph_args(const BundleCall& c, lm::Params* prm, int* rounds) {
  const int N = c.num_poses, F = c.num_factors, P = c.num_priors, Q = c.num_betweens;
  const int max_poses = c.graph ? GLIM_AMD_GRAPH_MAX_POSES : bundle_lm::MAX_POSES, max_factors = c.graph ? GLIM_AMD_GRAPH_MAX_FACTORS : bundle_lm::MAX_FACTORS,
            max_terms = c.graph ? GLIM_AMD_GRAPH_MAX_TERMS : bundle_lm::MAX_TERMS;
  const glim_amd_graph_terms* more = c.more;
  const glim_amd_nav_terms* nav = c.nav;
  if (!c.ctx || !c.X_init12 || !c.X_out12 || (!c.result && !c.nav_result)) return GLIM_AMD_ERR_INVALID;
  if (F > 0 && (!c.targets || !c.sources || !c.target_pose || !c.source_pose)) return GLIM_AMD_ERR_INVALID;
  if ((P > 0 && !c.priors) || (Q > 0 && !c.betweens)) return GLIM_AMD_ERR_INVALID;
  const int D = more ? more->num_dampings : 0;
  if (D < 0 || (D > 0 && !more->dampings)) return GLIM_AMD_ERR_INVALID;
  const int VP = nav ? nav->num_vector_priors : 0, VB = nav ? nav->num_vector_betweens : 0, I = nav ? nav->num_imu_terms : 0;
  if (VP < 0 || VB < 0 || I < 0 || (VP > 0 && !nav->vector_priors) || (VB > 0 && !nav->vector_betweens) || (I > 0 && !nav->imu_terms)) return GLIM_AMD_ERR_INVALID;
  if (F + P + Q == 0 && VP == 0 && VB == 0 && I == 0) return GLIM_AMD_ERR_INVALID;  // (dampings alone too: there is nothing to optimise over)
  if (c.flags & ~(uint32_t)GLIM_AMD_FACTOR_SURFACE_VALIDATION) return GLIM_AMD_ERR_INVALID;  // GLIM_AMD_FACTOR_BINARY: every factor here is binary
  GA_TRY(resolve_params(c.params, bundle_default_params, prm, rounds));
  if (N > max_poses || F > max_factors || P > max_terms || Q > max_terms || D > max_terms) return GLIM_AMD_ERR_UNSUPPORTED;
  if (VP > max_terms || VB > max_terms || I > max_terms) return GLIM_AMD_ERR_UNSUPPORTED;
  if (!one_context(c.targets, c.sources, F, c.ctx)) return GLIM_AMD_ERR_INVALID;
  for (int f = 0; f < F; f++)
    if (c.target_pose[f] < 0 || c.target_pose[f] >= N || c.source_pose[f] < 0 || c.source_pose[f] >= N || c.target_pose[f] == c.source_pose[f])
      return GLIM_AMD_ERR_INVALID;
  for (int p = 0; p < P; p++) {
    if (c.priors[p].pose < 0 || c.priors[p].pose >= N) return GLIM_AMD_ERR_INVALID;
    if (!all_finite_host(c.priors[p].T, 12) || !all_finite_host(c.priors[p].information, 36)) return GLIM_AMD_ERR_INVALID;
  }
  for (int q = 0; q < Q; q++) {
    const glim_amd_bundle_between& b = c.betweens[q];
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
  if (!all_finite_host(c.X_init12, 12 * N)) return GLIM_AMD_ERR_INVALID;
  if (nav) GA_TRY(check_nav_args(c));
  return vgicp_pairs_ok(c.targets, c.sources, F);
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

  GraphBlocks(const BundleCall& c, const lm::Params& prm, size_t extra)
      : N(c.num_poses), F(c.num_factors), P(c.num_priors), Q(c.num_betweens), D(c.more ? c.more->num_dampings : 0), VP(c.nav ? c.nav->num_vector_priors : 0),
        VB(c.nav ? c.nav->num_vector_betweens : 0), I(c.nav ? c.nav->num_imu_terms : 0), kinds(c.nav && c.nav->kinds),
        widths(c.more && c.more->between_huber_width && c.num_betweens > 0) {
    using namespace bundle_lm;
    const glim_amd_graph_terms* more = c.more;
    const glim_amd_nav_terms* nav = c.nav;
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
      hi[i_ft + f] = c.target_pose[f];
      hi[i_fs + f] = c.source_pose[f];
    }
    for (int p = 0; p < P; p++) {
      hi[i_pk + p] = c.priors[p].pose;
      memcpy(&hd[o_pT + 12 * (size_t)p], c.priors[p].T, 12 * sizeof(double));
      memcpy(&hd[o_pL + 36 * (size_t)p], c.priors[p].information, 36 * sizeof(double));
    }
    for (int q = 0; q < Q; q++) {
      hi[i_bi + q] = c.betweens[q].pose_i;
      hi[i_bj + q] = c.betweens[q].pose_j;
      memcpy(&hd[o_bT + 12 * (size_t)q], c.betweens[q].T, 12 * sizeof(double));
      memcpy(&hd[o_bL + 36 * (size_t)q], c.betweens[q].information, 36 * sizeof(double));
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
    init(prm, c.X_init12, host);
  }
};

// what glim_amd_bundle_result and glim_amd_nav_result have in common
template <class Result>
void graph_result(const bundle_lm::Scalars& sc, Result* result) {
  memset(result, 0, sizeof(*result));
  result->cost = sc.cost, result->factor_cost = sc.fcost, result->prior_cost = sc.pcost, result->between_cost = sc.bcost;
  result->num_inliers = (int64_t)llround(sc.inliers);
  result->iterations = sc.iterations, result->trials = sc.trials, result->status = sc.status, result->lambda = sc.lambda;
}

// Both loops: a round is vgicp_batch_round over the F factors, all behind the problem's ONE status word (stride 0), and then either the bundle
// decide kernel or the graph's launches (graph_round); both leave the next round's T_f in the batch's pose buffer.
int run_bundle_align(const BundleCall& c) {
  using namespace bundle_lm;
  const int chunk = chunk_rounds(c), N = c.num_poses, F = c.num_factors, Q = c.num_betweens;
  if (!trace_arrays_ok(c) || chunk < 0) return GLIM_AMD_ERR_INVALID;
  if (N < 0 || F < 0 || c.num_priors < 0 || Q < 0) return GLIM_AMD_ERR_INVALID;
  if (N == 0) return GLIM_AMD_OK;
  lm::Params prm;
  int rounds;
  GA_TRY(check_graph_args(c, &prm, &rounds));
  const GraphBlocks blk(c, prm, c.graph ? graph_scratch_doubles(6 * N) : 0);

  glim_amd_ctx* ctx = c.ctx;
  std::unique_lock<std::mutex> held(ctx->mu);  // once for the call
  GA_HIP(hipSetDevice(ctx->device));
  VgicpBatch batch;  // (destroyed last: its plan goes back after the stream has been waited for)
  DeviceTemp d_d, d_i;
  TraceBuffer tX, tTf, trec, trounds;
  hipStream_t st = ctx->stream();
  if (F > 0) {
    GA_TRY(vgicp_batch_open(ctx, c.targets, c.sources, c.flags, F, &batch));
    st = batch.stream();
  }
  SyncOnExit in_flight(st);  // an error exit after the launches waits for the stream before the scratch goes back to the pool
  GA_HIP(pool_malloc(&d_d.p, std::max<size_t>(1, blk.total_doubles) * sizeof(double)));
  GA_HIP(pool_malloc(&d_i.p, std::max<size_t>(1, blk.total_ints) * sizeof(int)));
  GA_TRY(tX.open(c.trace.X, (size_t)rounds * 12 * N * sizeof(double), st));  // (an array the caller did not give opens nothing)
  GA_TRY(tTf.open(c.trace.Tf, (size_t)rounds * 12 * F * sizeof(double), st));
  GA_TRY(trec.open(c.trace.rec, (size_t)rounds * lm::RECORD * F * sizeof(double), st));
  GA_TRY(trounds.open(c.trace.rounds, (size_t)rounds * sizeof(glim_amd_bundle_trace_round), st));
  const BundleTrace tr{tX.d.as<double>(), tTf.d.as<double>(), trec.d.as<double>(), trounds.d.as<glim_amd_bundle_trace_round>()};
  GA_HIP(hipMemcpyAsync(d_d.p, blk.hd.data(), blk.upload_doubles * sizeof(double), hipMemcpyHostToDevice, st));
  if (blk.total_ints) GA_HIP(hipMemcpyAsync(d_i.p, blk.hi.data(), blk.total_ints * sizeof(int), hipMemcpyHostToDevice, st));
  Problem pr = blk.problem_at(d_d.as<double>(), d_i.as<int>(), F > 0 ? batch.poses() : d_d.as<double>() + blk.o_Tf0);
  const GraphScratch gs = graph_scratch_at(d_d.as<double>() + blk.o_extra, 6 * N);
  if (c.graph) {
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
      if (c.graph) GA_TRY(graph_round(pr, gs, prm, d_recs, d_status, tr, r, c.one_thread, st));
      else bundle_decide_kernel<<<1, BUNDLE_THREADS, 0, st>>>(pr, prm, d_recs, tr, r, c.one_thread);
    }
    GA_HIP(hipGetLastError());
    GA_HIP(hipMemcpyAsync(&sc, pr.s, sizeof(sc), hipMemcpyDeviceToHost, st));
    if (r == rounds) break;
    GA_HIP(hipStreamSynchronize(st));  // a chunk's end: the loop stops enqueueing when the problem has finished
    if (sc.status != lm::RUNNING) break;
  }
  std::vector<double> rec_host((size_t)lm::RECORD * F);
  GA_HIP(hipMemcpyAsync(c.X_out12, pr.X, 12 * (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
  if (F > 0) GA_HIP(hipMemcpyAsync(rec_host.data(), pr.rec, rec_host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  if (c.between_weight_out && Q > 0) GA_HIP(hipMemcpyAsync(c.between_weight_out, pr.wk, (size_t)Q * sizeof(double), hipMemcpyDeviceToHost, st));
  for (TraceBuffer* t : {&tX, &tTf, &trec, &trounds}) GA_TRY(t->fetch(st));  // (Tf, rec: nothing without factors, no bytes)
  GA_HIP(hipStreamSynchronize(st));
  in_flight.dismiss();
  if (F > 0) batch.seen_complete();
  if (c.compact_out && F > 0) memcpy(c.compact_out, rec_host.data(), rec_host.size() * sizeof(double));
  if (c.result) graph_result(sc, c.result);
  if (c.nav_result) {
    graph_result(sc, c.nav_result);
    c.nav_result->vector_prior_cost = sc.vpcost, c.nav_result->vector_between_cost = sc.vbcost, c.nav_result->imu_cost = sc.icost;
  }
  return GLIM_AMD_OK;
}

}  // namespace

// The sixteen parameters every entry point of the two loops begins with and the five of a trace entry, and the statements that fill a
// BundleCall's fields from them BY NAME.  (The two public headers declare each entry point in full: a definition that disagrees does not compile.)
#define BUNDLE_ARGS                                                                                                                                                 \
  glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const int32_t* target_pose, const int32_t* source_pose,         \
      int32_t num_factors, uint32_t flags, const glim_amd_bundle_prior* priors, int32_t num_priors, const glim_amd_bundle_between* betweens, int32_t num_betweens, \
      const double* X_init12, int32_t num_poses, const glim_amd_lm_params* params, double* X_out12, double* compact_out
#define BUNDLE_TRACE_ARGS int32_t one_thread, double* X_trace, double* Tf_trace, double* compact_trace, glim_amd_bundle_trace_round* rounds
#define BUNDLE_CALL(c)                                                                                                                            \
  BundleCall c;                                                                                                                                   \
  c.ctx = ctx, c.targets = targets, c.sources = sources, c.target_pose = target_pose, c.source_pose = source_pose, c.num_factors = num_factors;   \
  c.flags = flags, c.priors = priors, c.num_priors = num_priors, c.betweens = betweens, c.num_betweens = num_betweens, c.X_init12 = X_init12;     \
  c.num_poses = num_poses, c.params = params, c.X_out12 = X_out12, c.compact_out = compact_out
#define BUNDLE_CALL_TRACE(c) \
  c.one_thread = one_thread ? 1 : 0, c.trace.X = X_trace, c.trace.Tf = Tf_trace, c.trace.rec = compact_trace, c.trace.rounds = rounds

extern "C" {

int glim_amd_bundle_align_default_params(glim_amd_lm_params* params) { return default_params_out(params, bundle_default_params); }

int glim_amd_bundle_align(BUNDLE_ARGS, glim_amd_bundle_result* result) {
  BUNDLE_CALL(c);
  c.result = result;
  return run_bundle_align(c);
}

int glim_amd_debug_bundle_align_trace(BUNDLE_ARGS, glim_amd_bundle_result* result, BUNDLE_TRACE_ARGS) {
  BUNDLE_CALL(c);
  BUNDLE_CALL_TRACE(c);
  c.result = result;
  return run_bundle_align(c);
}

int glim_amd_graph_align_default_params(glim_amd_lm_params* params) { return glim_amd_bundle_align_default_params(params); }

int glim_amd_graph_align(BUNDLE_ARGS, glim_amd_bundle_result* result) {
  BUNDLE_CALL(c);
  c.result = result, c.graph = true;
  return run_bundle_align(c);
}

int glim_amd_debug_graph_align_trace(BUNDLE_ARGS, glim_amd_bundle_result* result, BUNDLE_TRACE_ARGS, int32_t rounds_per_chunk) {
  BUNDLE_CALL(c);
  BUNDLE_CALL_TRACE(c);
  c.result = result, c.graph = true, c.rounds_per_chunk = rounds_per_chunk;
  return run_bundle_align(c);
}

// the two loops with damping terms and Huber widths: the same scaffold, the terms behind the graph
int glim_amd_bundle_align_terms(BUNDLE_ARGS, glim_amd_bundle_result* result, const glim_amd_graph_terms* more, double* between_weight_out) {
  BUNDLE_CALL(c);
  c.result = result, c.more = more, c.between_weight_out = between_weight_out;
  return run_bundle_align(c);
}

int glim_amd_debug_bundle_align_terms_trace(BUNDLE_ARGS, glim_amd_bundle_result* result, const glim_amd_graph_terms* more, double* between_weight_out,
                                            BUNDLE_TRACE_ARGS) {
  BUNDLE_CALL(c);
  BUNDLE_CALL_TRACE(c);
  c.result = result, c.more = more, c.between_weight_out = between_weight_out;
  return run_bundle_align(c);
}

int glim_amd_graph_align_terms(BUNDLE_ARGS, glim_amd_bundle_result* result, const glim_amd_graph_terms* more, double* between_weight_out) {
  BUNDLE_CALL(c);
  c.result = result, c.graph = true, c.more = more, c.between_weight_out = between_weight_out;
  return run_bundle_align(c);
}

int glim_amd_debug_graph_align_terms_trace(BUNDLE_ARGS, glim_amd_bundle_result* result, const glim_amd_graph_terms* more, double* between_weight_out, BUNDLE_TRACE_ARGS,
                                           int32_t rounds_per_chunk) {
  BUNDLE_CALL(c);
  BUNDLE_CALL_TRACE(c);
  c.result = result, c.graph = true, c.rounds_per_chunk = rounds_per_chunk, c.more = more, c.between_weight_out = between_weight_out;
  return run_bundle_align(c);
}

// the global graph with node kinds, vector priors, vector betweens and IMU terms (sub_mapping.cpp:218-243, global_mapping.cpp:168-216, 976-1042,
// odometry_estimation_imu.cpp:218-220, 268-283, loose_initial_state_estimation.cpp:105-124, 174): the same scaffold, the terms behind the graph
int glim_amd_graph_align_nav(BUNDLE_ARGS, glim_amd_nav_result* result, const glim_amd_graph_terms* more, double* between_weight_out, const glim_amd_nav_terms* nav) {
  if (!result) return GLIM_AMD_ERR_INVALID;
  BUNDLE_CALL(c);
  c.nav_result = result, c.graph = true, c.more = more, c.between_weight_out = between_weight_out, c.nav = nav;
  return run_bundle_align(c);
}

int glim_amd_debug_graph_align_nav_trace(BUNDLE_ARGS, glim_amd_nav_result* result, const glim_amd_graph_terms* more, double* between_weight_out,
                                         const glim_amd_nav_terms* nav, BUNDLE_TRACE_ARGS, int32_t rounds_per_chunk) {
  if (!result) return GLIM_AMD_ERR_INVALID;
  BUNDLE_CALL(c);
  BUNDLE_CALL_TRACE(c);
  c.nav_result = result, c.graph = true, c.rounds_per_chunk = rounds_per_chunk, c.more = more, c.between_weight_out = between_weight_out, c.nav = nav;
  return run_bundle_align(c);
}

#undef BUNDLE_ARGS
#undef BUNDLE_TRACE_ARGS
#undef BUNDLE_CALL
#undef BUNDLE_CALL_TRACE

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

}  // extern "C"
