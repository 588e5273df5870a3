// glim_amd/csrc/graph_solve.hpp under a plain C++ compiler, beside the rule it walks (bundle_lm_step.hpp), fed from a file.
//   solve   in : n, lambda, tile, then the packed system (lower triangle of H by rows, then b)
//           out: ok of bundle_lm::solve, ok of the blocked solve, then 1.0 / 0.0 for "the same bytes" of L, of y and of delta (L and y are
//                compared only when both solves succeeded: after a failed pivot nothing of them is used), then n of the blocked delta
//   step    in : 9 parameters in glim_amd_lm_params order (max_trials resolved), a graph (the format of test_bundle_lm_step.cpp, any N up to
//                the graph cap), N x 12 initial poses, R, then R x F x 29 records
//           out: per round the state after it, as test_bundle_lm_step.cpp writes it
// tests/test_graph_align.py writes the inputs.  The program has a main of its own, so it runs under the sanitizers as it stands.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../glim_amd/csrc/bundle_lm_step.hpp"
#include "../../glim_amd/csrc/graph_solve.hpp"

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

// a problem over host vectors, sized by the graph
struct Host {
  std::vector<int> ft, fs, pk, bi, bj, first, items, cursor;
  std::vector<double> pT, pL, bT, bL, X, cand, delta, rec, S, Tf, pc, bc, W;
  std::vector<glim_amd_linearized6> lin;
  bundle_lm::Scalars sc;
  bundle_lm::Problem pr;
  size_t read(const double* h, size_t left) {
    if (left < 4) return 0;
    const int N = (int)h[0], F = (int)h[1], P = (int)h[2], Q = (int)h[3];
    const size_t need = 4 + 2 * (size_t)F + 49 * (size_t)P + 50 * (size_t)Q;
    if (N < 0 || F < 0 || P < 0 || Q < 0 || 6 * N > graph_solve::MAX_DIM || left < need) return 0;
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
  if (!strcmp(argv[1], "solve")) {
    if (in.size() < 3) return 2;
    const int n = (int)h[0], tile = (int)h[2];
    if (n < 1 || n > graph_solve::MAX_DIM || !graph_solve::tile_ok(tile) || in.size() != 3 + (size_t)bundle_lm::system_doubles(n)) return 2;
    const double *S = h + 3, lambda = h[1];
    const int ld = graph_solve::leading(n);
    // the rule: the packed rows, first the factorisation alone (the statements of bundle_lm::solve), then solve() itself on a fresh copy
    std::vector<double> P(bundle_lm::system_doubles(n)), P2, ref_delta(n), W(graph_solve::matrix_doubles(n), 0.0), delta(n, -1.0);
    for (int i = 0; i <= n; i++)
      for (int j = 0; j < (i < n ? i + 1 : n); j++) {
        P[bundle_lm::tri(i) + j] = bundle_lm::solve_load(S, n, lambda, bundle_lm::tri(i) + j, i, j);
        W[(size_t)j * ld + i] = P[bundle_lm::tri(i) + j];
      }
    P2 = P;
    const bool ref_ok = bundle_lm::solve(P2.data(), n, ref_delta.data());
    bool chol_ok = true;
    for (int j = 0; j < n && chol_ok; j++) {
      const double d = bundle_lm::chol_pivot(P.data(), j);
      if (!(d > 0.0)) {
        chol_ok = false;
        break;
      }
      P[bundle_lm::tri(j) + j] = d;
      for (int i = j + 1; i <= n; i++) P[bundle_lm::tri(i) + j] = bundle_lm::chol_entry(P.data(), i, j);
    }
    if (chol_ok != ref_ok) return 3;
    const bool ok = graph_solve::factor_blocked(W.data(), n, tile);
    bool same_L = true, same_y = true;
    if (ok && ref_ok) {
      for (int i = 0; i <= n; i++)
        for (int j = 0; j < (i < n ? i + 1 : n); j++) {
          const double got = graph_solve::factor_entry(W.data(), n, tile, i, j);
          const bool same = !memcmp(&got, &P[bundle_lm::tri(i) + j], sizeof(double));
          if (i < n) same_L = same_L && same;
          else same_y = same_y && same;
        }
    }
    graph_solve::back_blocked(W.data(), n, tile, !ok, delta.data());
    const bool same_delta = !memcmp(delta.data(), ref_delta.data(), n * sizeof(double));
    const double head[5] = {ref_ok ? 1.0 : 0.0, ok ? 1.0 : 0.0, same_L ? 1.0 : 0.0, same_y ? 1.0 : 0.0, same_delta ? 1.0 : 0.0};
    out.insert(out.end(), head, head + 5);
    out.insert(out.end(), delta.begin(), delta.end());
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
  printf("test_graph_solve OK (%s, %zu doubles)\n", argv[1], out.size());
  return 0;
}
