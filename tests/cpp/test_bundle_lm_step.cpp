// glim_amd/csrc/bundle_lm_step.hpp under a plain C++ compiler: the statements bundle_align.hip's bundle decide kernel runs, fed from a file.
// A graph is, in doubles: N, F, P, Q, F x (t, s), P x (pose, 12 of P, 36 of the information), Q x (i, j, 12 of D, 36 of the information).
//   expand    in : n, then n x (29 of a record, 12 of a pose)
//             out: n x 122, the bytes of glim_amd_linearized6
//   assemble  in : a graph, N x 12 poses, F x 29 records (evaluated at X_t^-1 X_s)
//             out: the packed system (lower triangle of H by rows, then b), then cost, factor cost, prior cost, between cost, inliers
//   solve     in : n, lambda, the packed system
//             out: ok, then n of delta
//   step      in : 9 parameters in glim_amd_lm_params order (max_trials resolved), a graph, N x 12 initial poses, R, then R x F x 29 records
//             out: per round the state after it: kept poses (12 N), next candidates (12 N), delta (6 N), lambda, solve_ok, iterations, trials,
//                  status, accepted, the kept cost
// tests/test_bundle_align.py writes the inputs and compares with tests/bundle_lm_restatement.py, numpy.linalg and glim_amd_expand_compact.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../glim_amd/csrc/bundle_lm_step.hpp"

using namespace glim_amd;

static bool read_all(const char* path, std::vector<double>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  double buf[256];
  size_t n;
  while ((n = fread(buf, sizeof(double), 256, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return true;
}

static bool write_all(const char* path, const std::vector<double>& v) {
  FILE* g = fopen(path, "wb");
  if (!g) return false;
  const bool ok = fwrite(v.data(), sizeof(double), v.size(), g) == v.size();
  fclose(g);
  return ok;
}

// a problem over host vectors
struct Host {
  std::vector<int> ft, fs, pk, bi, bj, first, items, cursor;
  std::vector<double> pT, pL, bT, bL, X, cand, delta, rec, S, Tf, pc, bc, W;
  std::vector<glim_amd_linearized6> lin;
  bundle_lm::Scalars sc;
  bundle_lm::Problem pr;
  // reads a graph at h; returns the doubles read, or 0
  size_t read(const double* h, size_t left) {
    if (left < 4) return 0;
    const int N = (int)h[0], F = (int)h[1], P = (int)h[2], Q = (int)h[3];
    const size_t need = 4 + 2 * (size_t)F + 49 * (size_t)P + 50 * (size_t)Q;
    if (N < 0 || F < 0 || P < 0 || Q < 0 || N > bundle_lm::MAX_POSES || left < need) return 0;
    const double* c = h + 4;
    for (int f = 0; f < F; f++, c += 2) {
      ft.push_back((int)c[0]);
      fs.push_back((int)c[1]);
    }
    for (int p = 0; p < P; p++, c += 49) {
      pk.push_back((int)c[0]);
      pT.insert(pT.end(), c + 1, c + 13);
      pL.insert(pL.end(), c + 13, c + 49);
    }
    for (int q = 0; q < Q; q++, c += 50) {
      bi.push_back((int)c[0]);
      bj.push_back((int)c[1]);
      bT.insert(bT.end(), c + 2, c + 14);
      bL.insert(bL.end(), c + 14, c + 50);
    }
    const int n = 6 * N, nsys = bundle_lm::system_doubles(n);
    first.resize(bundle_lm::tri(N) + 1);
    cursor.resize(bundle_lm::tri(N) + 1);
    items.resize(bundle_lm::list_items(F, P, Q) + 1);
    X.resize(12 * N + 1), cand.resize(12 * N + 1), delta.resize(n + 1), rec.resize(29 * F + 1), S.resize(nsys + 1), Tf.resize(12 * F + 1);
    pc.resize(bundle_lm::PRIOR_STRIDE * P + 1), bc.resize(bundle_lm::BETWEEN_STRIDE * Q + 1), W.resize(nsys + 1), lin.resize(F + 1);
    ft.push_back(0), fs.push_back(0), pk.push_back(0), bi.push_back(0), bj.push_back(0);  // (no empty vector's data())
    pT.push_back(0), pL.push_back(0), bT.push_back(0), bL.push_back(0);
    pr.g = bundle_lm::Graph{N, F, P, Q, ft.data(), fs.data(), pk.data(), pT.data(), pL.data(), bi.data(), bj.data(), bT.data(), bL.data(), first.data(), items.data()};
    bundle_lm::build_lists(pr.g, first.data(), items.data(), cursor.data());
    pr.X = X.data(), pr.cand = cand.data(), pr.delta = delta.data(), pr.rec = rec.data(), pr.S = S.data(), pr.Tf = Tf.data();
    pr.lin = lin.data(), pr.pc = pc.data(), pr.bc = bc.data(), pr.W = W.data(), pr.s = &sc;
    return need;
  }
};

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  std::vector<double> in, out;
  if (!read_all(argv[2], in)) return 2;
  const double* h = in.data();
  if (!strcmp(argv[1], "expand")) {
    if (in.empty()) return 2;
    const size_t n = (size_t)h[0];
    if (in.size() != 1 + 41 * n) return 2;
    static_assert(sizeof(glim_amd_linearized6) == 122 * sizeof(double), "a factor's blocks, in doubles");
    out.resize(122 * n);
    std::vector<glim_amd_linearized6> lin(n + 1);
    for (size_t k = 0; k < n; k++) {
      // the record and the pose as arrays of F = k + 1 factors, so that the index arithmetic runs too
      bundle_lm::expand_factor(h + 1 + 41 * k - 29 * k, h + 1 + 41 * k + 29 - 12 * k, (int)k, lin.data());
      memcpy(out.data() + 122 * k, &lin[k], sizeof(glim_amd_linearized6));
    }
  } else if (!strcmp(argv[1], "solve")) {
    if (in.size() < 2) return 2;
    const int n = (int)h[0];
    if (n < 0 || n > bundle_lm::MAX_DIM || in.size() != 2 + (size_t)bundle_lm::system_doubles(n)) return 2;
    std::vector<double> W(bundle_lm::system_doubles(n) + 1), delta(n + 1);
    for (int i = 0; i <= n; i++)
      for (int j = 0; j < (i < n ? i + 1 : n); j++) W[bundle_lm::tri(i) + j] = bundle_lm::solve_load(h + 2, n, h[1], bundle_lm::tri(i) + j, i, j);
    out.push_back(bundle_lm::solve(W.data(), n, delta.data()) ? 1.0 : 0.0);
    out.insert(out.end(), delta.begin(), delta.begin() + n);
  } else if (!strcmp(argv[1], "assemble")) {
    Host H;
    const size_t used = H.read(h, in.size());
    if (!used) return 2;
    const bundle_lm::Graph& g = H.pr.g;
    if (in.size() != used + 12 * (size_t)g.N + 29 * (size_t)g.F) return 2;
    const double *X = h + used, *recs = X + 12 * g.N;
    for (int f = 0; f < g.F; f++) {
      bundle_lm::relative_pose(X, g.ft, g.fs, f, H.pr.Tf);
      bundle_lm::expand_factor(recs, H.pr.Tf, f, H.pr.lin);
    }
    for (int p = 0; p < g.P; p++) bundle_lm::prior_term(g, X, p, H.pr.pc);
    for (int q = 0; q < g.Q; q++) bundle_lm::between_term(g, X, q, H.pr.bc);
    const int n = 6 * g.N;
    for (int r = 0; r < n; r++)
      for (int c = 0; c <= r; c++) out.push_back(bundle_lm::assemble_entry(g, H.pr.lin, H.pr.pc, H.pr.bc, r, c));
    for (int r = 0; r < n; r++) out.push_back(bundle_lm::assemble_rhs(g, H.pr.lin, H.pr.pc, H.pr.bc, r));
    const double fc = bundle_lm::sum_ascending(recs + 1, g.F, 29), pcs = bundle_lm::sum_ascending(H.pr.pc + 42, g.P, bundle_lm::PRIOR_STRIDE),
                 bcs = bundle_lm::sum_ascending(H.pr.bc + 156, g.Q, bundle_lm::BETWEEN_STRIDE);
    const double tail[5] = {(fc + pcs) + bcs, fc, pcs, bcs, bundle_lm::sum_ascending(recs, g.F, 29)};
    out.insert(out.end(), tail, tail + 5);
  } else if (!strcmp(argv[1], "step")) {
    if (in.size() < 13) return 2;
    lm::Params p{h[0], h[1], h[2], h[3], h[4], h[5], (int)h[6], (int)h[7], h[8]};
    Host H;
    const size_t used = H.read(h + 9, in.size() - 9);
    if (!used) return 2;
    const bundle_lm::Graph& g = H.pr.g;
    const size_t at = 9 + used + 12 * (size_t)g.N;
    if (in.size() < at + 1) return 2;
    const size_t R = (size_t)h[at];
    if (in.size() != at + 1 + R * 29 * (size_t)g.F) return 2;
    bundle_lm::init(p, h + 9 + used, H.pr);
    for (int f = 0; f < g.F; f++) bundle_lm::relative_pose(H.pr.cand, g.ft, g.fs, f, H.pr.Tf);
    for (size_t k = 0; k < R; k++) {
      bundle_lm::step(p, H.pr, h + at + 1 + k * 29 * (size_t)g.F);
      out.insert(out.end(), H.X.begin(), H.X.begin() + 12 * g.N);
      out.insert(out.end(), H.cand.begin(), H.cand.begin() + 12 * g.N);
      out.insert(out.end(), H.delta.begin(), H.delta.begin() + 6 * g.N);
      const double tail[7] = {H.sc.lambda, (double)H.sc.solve_ok, (double)H.sc.iterations, (double)H.sc.trials, (double)H.sc.status, (double)H.sc.accepted, H.sc.cost};
      out.insert(out.end(), tail, tail + 7);
    }
  } else {
    return 2;
  }
  if (!write_all(argv[3], out)) return 2;
  printf("test_bundle_lm_step OK (%s, %zu doubles)\n", argv[1], out.size());
  return 0;
}
