// glim_amd/csrc/bundle_lm_step.hpp under a plain C++ compiler once more, with the damping terms and the Huber widths of the betweens, at any
// number of poses.  A graph is test_bundle_lm_step.cpp's, in doubles, followed by: D, D x (pose, 6 of the diagonal), then 1 and Q widths, or 0
// (no width array).
//   assemble        in : a graph, N x 12 poses, F x 29 records
//                   out: what test_bundle_lm_step.cpp's `assemble` writes: the packed system, then cost, factor cost, prior cost, between cost,
//                        inliers
//   assemble_terms  the same in; out: that, then Q weights, then Q x 157 of the betweens' stored contributions (H 12 x 12, b 12, cost)
//   step            in : 9 parameters, a graph, N x 12 initial poses, R, then R x F x 29 records
//                   out: what test_bundle_lm_step.cpp's `step` writes per round
//   step_terms      the same in; out: per round that, then the Q kept weights
// tests/test_graph_terms.py writes the inputs and compares with tests/graph_terms_restatement.py and with test_bundle_lm_step.cpp's bytes.
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
  std::vector<int> ft, fs, pk, bi, bj, dk, first, items, cursor;
  std::vector<double> pT, pL, bT, bL, dd, bw, X, cand, delta, rec, S, Tf, pc, bc, W, wt, wk;
  std::vector<glim_amd_linearized6> lin;
  bundle_lm::Scalars sc;
  bundle_lm::Problem pr;
  // reads a graph at h; returns the doubles read, or 0
  size_t read(const double* h, size_t left) {
    if (left < 4) return 0;
    const int N = (int)h[0], F = (int)h[1], P = (int)h[2], Q = (int)h[3];
    if (N < 0 || F < 0 || P < 0 || Q < 0) return 0;
    size_t need = 4 + 2 * (size_t)F + 49 * (size_t)P + 50 * (size_t)Q + 1;
    if (left < need) return 0;
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
    const int D = (int)*c++;
    need += 7 * (size_t)D + 1;
    if (D < 0 || left < need) return 0;
    for (int d = 0; d < D; d++, c += 7) {
      dk.push_back((int)c[0]);
      dd.insert(dd.end(), c + 1, c + 7);
    }
    const bool widths = *c++ != 0.0;
    if (widths) {
      need += (size_t)Q;
      if (left < need) return 0;
      bw.insert(bw.end(), c, c + Q);
    }
    const int n = 6 * N, nsys = bundle_lm::system_doubles(n);
    first.resize(bundle_lm::tri(N) + 1);
    cursor.resize(bundle_lm::tri(N) + 1);
    items.resize(bundle_lm::list_items(F, P, Q, D) + 1);
    X.resize(12 * N + 1), cand.resize(12 * N + 1), delta.resize(n + 1), rec.resize(29 * F + 1), S.resize(nsys + 1), Tf.resize(12 * F + 1);
    pc.resize(bundle_lm::PRIOR_STRIDE * P + 1), bc.resize(bundle_lm::BETWEEN_STRIDE * Q + 1), W.resize(nsys + 1), lin.resize(F + 1);
    wt.resize(Q + 1), wk.resize(Q + 1);
    ft.push_back(0), fs.push_back(0), pk.push_back(0), bi.push_back(0), bj.push_back(0), dk.push_back(0);  // (no empty vector's data())
    pT.push_back(0), pL.push_back(0), bT.push_back(0), bL.push_back(0), dd.push_back(0), bw.push_back(0);
    pr.g = bundle_lm::Graph{N, F, P, Q, ft.data(), fs.data(), pk.data(), pT.data(), pL.data(), bi.data(), bj.data(), bT.data(), bL.data(), first.data(), items.data(),
                            D, dk.data(), dd.data(), widths ? bw.data() : nullptr};
    bundle_lm::build_lists(pr.g, first.data(), items.data(), cursor.data());
    pr.X = X.data(), pr.cand = cand.data(), pr.delta = delta.data(), pr.rec = rec.data(), pr.S = S.data(), pr.Tf = Tf.data();
    pr.lin = lin.data(), pr.pc = pc.data(), pr.bc = bc.data(), pr.W = W.data(), pr.s = &sc, pr.wt = wt.data(), pr.wk = wk.data();
    return need;
  }
};

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  std::vector<double> in, out;
  if (!read_all(argv[2], in)) return 2;
  const double* h = in.data();
  const bool terms = strstr(argv[1], "_terms") != nullptr;
  if (!strcmp(argv[1], "assemble") || !strcmp(argv[1], "assemble_terms")) {
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
    for (int q = 0; q < g.Q; q++) bundle_lm::between_term(g, X, q, H.pr.bc, H.pr.wt);
    const int n = 6 * g.N;
    for (int r = 0; r < n; r++)
      for (int c = 0; c <= r; c++) out.push_back(bundle_lm::assemble_entry(g, H.pr.lin, H.pr.pc, H.pr.bc, r, c));
    for (int r = 0; r < n; r++) out.push_back(bundle_lm::assemble_rhs(g, H.pr.lin, H.pr.pc, H.pr.bc, r));
    const double fc = bundle_lm::sum_ascending(recs + 1, g.F, 29), pcs = bundle_lm::sum_ascending(H.pr.pc + 42, g.P, bundle_lm::PRIOR_STRIDE),
                 bcs = bundle_lm::sum_ascending(H.pr.bc + 156, g.Q, bundle_lm::BETWEEN_STRIDE);
    const double tail[5] = {(fc + pcs) + bcs, fc, pcs, bcs, bundle_lm::sum_ascending(recs, g.F, 29)};
    out.insert(out.end(), tail, tail + 5);
    if (terms) {
      out.insert(out.end(), H.wt.begin(), H.wt.begin() + g.Q);
      out.insert(out.end(), H.bc.begin(), H.bc.begin() + bundle_lm::BETWEEN_STRIDE * g.Q);
    }
  } else if (!strcmp(argv[1], "step") || !strcmp(argv[1], "step_terms")) {
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
      if (terms) out.insert(out.end(), H.wk.begin(), H.wk.begin() + g.Q);
    }
  } else {
    return 2;
  }
  if (!write_all(argv[3], out)) return 2;
  printf("test_graph_terms_step OK (%s, %zu doubles)\n", argv[1], out.size());
  return 0;
}
