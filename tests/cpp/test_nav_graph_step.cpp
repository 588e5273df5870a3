// glim_amd/csrc/bundle_lm_step.hpp and nav_terms.hpp under a plain C++ compiler: the rule with node kinds, vector priors, vector betweens and
// IMU terms, at any number of nodes.  A graph is test_graph_terms_step.cpp's, in doubles, followed by: N kinds; VP, VP x (node, 6 of the value,
// 36 of the information); VB, VB x (node i, node j, 6 of the measurement, 36); I, I x (5 nodes, mode, 154 of nav::IMU_DATA).
//   imu       in : K, then K x nav::IMU_EVAL_IN;  out: K x (r 9, J 9 x 24)
//   assemble  in : a graph, N x 12 node values, F x 29 records
//             out: the packed system, then cost, factor cost, prior cost, between cost, inliers, vector prior cost, vector between cost, IMU cost
//   step      in : 9 parameters, a graph, N x 12 initial values, R, then R x F x 29 records
//             out: what test_bundle_lm_step.cpp's `step` writes per round
// tests/test_nav_graph.py writes the inputs and compares with tests/nav_graph_restatement.py, with a 200-bit reference and with
// test_graph_terms_step.cpp's bytes.
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
  std::vector<int> ft, fs, pk, bi, bj, dk, first, items, cursor, kind, vpk, vbi, vbj, imn, imm;
  std::vector<double> pT, pL, bT, bL, dd, bw, X, cand, delta, rec, S, Tf, pc, bc, W, wt, wk, vpv, vpL, vbd, vbL, imd, vpc, vbc, ic;
  std::vector<glim_amd_linearized6> lin;
  bundle_lm::Scalars sc;
  bundle_lm::Problem pr;
  // reads a graph at h; returns the doubles read, or 0
  size_t read(const double* h, size_t left) {
    const double* c = h;
    const double* end = h + left;
    auto have = [&](size_t k) { return (size_t)(end - c) >= k; };
    if (!have(4)) return 0;
    const int N = (int)c[0], F = (int)c[1], P = (int)c[2], Q = (int)c[3];
    c += 4;
    if (N < 0 || F < 0 || P < 0 || Q < 0 || !have(2 * (size_t)F + 49 * (size_t)P + 50 * (size_t)Q + 1)) return 0;
    for (int f = 0; f < F; f++, c += 2) ft.push_back((int)c[0]), fs.push_back((int)c[1]);
    for (int p = 0; p < P; p++, c += 49) {
      pk.push_back((int)c[0]);
      pT.insert(pT.end(), c + 1, c + 13);
      pL.insert(pL.end(), c + 13, c + 49);
    }
    for (int q = 0; q < Q; q++, c += 50) {
      bi.push_back((int)c[0]), bj.push_back((int)c[1]);
      bT.insert(bT.end(), c + 2, c + 14);
      bL.insert(bL.end(), c + 14, c + 50);
    }
    const int D = (int)*c++;
    if (D < 0 || !have(7 * (size_t)D + 1)) return 0;
    for (int d = 0; d < D; d++, c += 7) {
      dk.push_back((int)c[0]);
      dd.insert(dd.end(), c + 1, c + 7);
    }
    const bool widths = *c++ != 0.0;
    if (widths) {
      if (!have(Q)) return 0;
      bw.insert(bw.end(), c, c + Q);
      c += Q;
    }
    if (!have((size_t)N + 1)) return 0;
    for (int k = 0; k < N; k++) kind.push_back((int)*c++);
    const int VP = (int)*c++;
    if (VP < 0 || !have(43 * (size_t)VP + 1)) return 0;
    for (int p = 0; p < VP; p++, c += 43) {
      vpk.push_back((int)c[0]);
      vpv.insert(vpv.end(), c + 1, c + 7);
      vpL.insert(vpL.end(), c + 7, c + 43);
    }
    const int VB = (int)*c++;
    if (VB < 0 || !have(44 * (size_t)VB + 1)) return 0;
    for (int q = 0; q < VB; q++, c += 44) {
      vbi.push_back((int)c[0]), vbj.push_back((int)c[1]);
      vbd.insert(vbd.end(), c + 2, c + 8);
      vbL.insert(vbL.end(), c + 8, c + 44);
    }
    const int I = (int)*c++;
    const size_t per = 6 + nav::IMU_DATA;
    if (I < 0 || !have(per * (size_t)I)) return 0;
    for (int q = 0; q < I; q++, c += per) {
      for (int u = 0; u < 5; u++) imn.push_back((int)c[u]);
      imm.push_back((int)c[5]);
      imd.insert(imd.end(), c + 6, c + per);
    }
    const int n = 6 * N, nsys = bundle_lm::system_doubles(n);
    nav::Terms t;
    t.VP = VP, t.VB = VB, t.I = I;
    first.resize(bundle_lm::tri(N) + 1);
    cursor.resize(bundle_lm::tri(N) + 1);
    items.resize(bundle_lm::list_items(F, P, Q, D, t) + 1);
    X.resize(12 * N + 1), cand.resize(12 * N + 1), delta.resize(n + 1), rec.resize(29 * F + 1), S.resize(nsys + 1), Tf.resize(12 * F + 1);
    pc.resize(bundle_lm::PRIOR_STRIDE * P + 1), bc.resize(bundle_lm::BETWEEN_STRIDE * Q + 1), W.resize(nsys + 1), lin.resize(F + 1);
    wt.resize(Q + 1), wk.resize(Q + 1);
    vpc.resize(nav::VPRIOR_STRIDE * VP + 1), vbc.resize(nav::VBETWEEN_STRIDE * VB + 1), ic.resize((size_t)nav::IMU_STRIDE * I + 1);
    ft.push_back(0), fs.push_back(0), pk.push_back(0), bi.push_back(0), bj.push_back(0), dk.push_back(0);  // (no empty vector's data())
    pT.push_back(0), pL.push_back(0), bT.push_back(0), bL.push_back(0), dd.push_back(0), bw.push_back(0);
    kind.push_back(0), vpk.push_back(0), vbi.push_back(0), vbj.push_back(0), imn.push_back(0), imm.push_back(0);
    vpv.push_back(0), vpL.push_back(0), vbd.push_back(0), vbL.push_back(0), imd.push_back(0);
    pr.g = bundle_lm::Graph{N, F, P, Q, ft.data(), fs.data(), pk.data(), pT.data(), pL.data(), bi.data(), bj.data(), bT.data(), bL.data(), first.data(), items.data(),
                            D, dk.data(), dd.data(), widths ? bw.data() : nullptr};
    t.kind = kind.data();
    t.vpk = vpk.data(), t.vpv = vpv.data(), t.vpL = vpL.data();
    t.vbi = vbi.data(), t.vbj = vbj.data(), t.vbd = vbd.data(), t.vbL = vbL.data();
    t.imn = imn.data(), t.imm = imm.data(), t.imd = imd.data();
    t.vpc = vpc.data(), t.vbc = vbc.data(), t.ic = ic.data();
    pr.g.nav = t;
    bundle_lm::build_lists(pr.g, first.data(), items.data(), cursor.data());
    pr.X = X.data(), pr.cand = cand.data(), pr.delta = delta.data(), pr.rec = rec.data(), pr.S = S.data(), pr.Tf = Tf.data();
    pr.lin = lin.data(), pr.pc = pc.data(), pr.bc = bc.data(), pr.W = W.data(), pr.s = &sc, pr.wt = wt.data(), pr.wk = wk.data();
    return (size_t)(c - h);
  }
};

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  std::vector<double> in, out;
  if (!read_all(argv[2], in)) return 2;
  const double* h = in.data();
  if (!strcmp(argv[1], "imu")) {
    if (in.empty()) return 2;
    const size_t K = (size_t)h[0];
    if (in.size() != 1 + K * nav::IMU_EVAL_IN) return 2;
    out.resize(K * nav::IMU_EVAL_OUT);
    for (size_t k = 0; k < K; k++) nav::imu_eval(h + 1 + k * nav::IMU_EVAL_IN, out.data() + k * nav::IMU_EVAL_OUT);
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
    for (int q = 0; q < g.Q; q++) bundle_lm::between_term(g, X, q, H.pr.bc, H.pr.wt);
    for (int p = 0; p < g.nav.VP; p++) nav::vector_prior_term(g.nav, X, p);
    for (int q = 0; q < g.nav.VB; q++) nav::vector_between_term(g.nav, X, q);
    for (int q = 0; q < g.nav.I; q++) nav::imu_term(g.nav, X, q);
    const int n = 6 * g.N;
    for (int r = 0; r < n; r++)
      for (int c = 0; c <= r; c++) out.push_back(bundle_lm::assemble_entry(g, H.pr.lin, H.pr.pc, H.pr.bc, r, c));
    for (int r = 0; r < n; r++) out.push_back(bundle_lm::assemble_rhs(g, H.pr.lin, H.pr.pc, H.pr.bc, r));
    const double fc = bundle_lm::sum_ascending(recs + 1, g.F, 29), pcs = bundle_lm::sum_ascending(H.pr.pc + 42, g.P, bundle_lm::PRIOR_STRIDE),
                 bcs = bundle_lm::sum_ascending(H.pr.bc + 156, g.Q, bundle_lm::BETWEEN_STRIDE),
                 vps = bundle_lm::sum_ascending(H.vpc.data() + 42, g.nav.VP, nav::VPRIOR_STRIDE),
                 vbs = bundle_lm::sum_ascending(H.vbc.data() + 156, g.nav.VB, nav::VBETWEEN_STRIDE),
                 ims = bundle_lm::sum_ascending(H.ic.data() + nav::IMU_STRIDE - 1, g.nav.I, nav::IMU_STRIDE);
    const double tail[8] = {bundle_lm::total_cost(fc, pcs, bcs, vps, vbs, ims), fc, pcs, bcs, bundle_lm::sum_ascending(recs, g.F, 29), vps, vbs, ims};
    out.insert(out.end(), tail, tail + 8);
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
  printf("test_nav_graph_step OK (%s, %zu doubles)\n", argv[1], out.size());
  return 0;
}
