// Stand-alone host program over the plain-C++ side of glim_amd/csrc/plane_ba.hpp and eig3_direct.hpp: the moment form of the plane / edge
// eigenvalue factor, through the very functions the kernels of plane_ba.hip call.  tests/test_plane_ba.py writes the input, builds this
// file plain and with -fsanitize=address,undefined, runs it directly and compares the output with tests/plane_ba_restatement.py.
//
//   input : kind K n, then n lines "frame x y z" (frame-local points), then K lines of 12 pose entries (3x4 row-major)
//   output: status, cost, 6 K gradient entries, 36 K^2 Hessian entries, then the eigenvalues and eigenvectors of the first 3x3 block of
//           H + H^T by eig3::direct (9 + 3 numbers: a second, unrelated matrix through the solver)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../glim_amd/csrc/plane_ba.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "r");
  if (!in) return 2;
  int kind = 0, K = 0;
  long n = 0;
  if (fscanf(in, "%d %d %ld", &kind, &K, &n) != 3 || K < 1 || K > glim_amd::ba::BA_MAX_FRAMES || n < 1) return 2;
  std::vector<double> pts(3 * (size_t)n), poses(12 * (size_t)K);
  std::vector<int> frame((size_t)n);
  for (long i = 0; i < n; i++)
    if (fscanf(in, "%d %lf %lf %lf", &frame[(size_t)i], &pts[3 * (size_t)i], &pts[3 * (size_t)i + 1], &pts[3 * (size_t)i + 2]) != 4) return 2;
  for (size_t i = 0; i < poses.size(); i++)
    if (fscanf(in, "%lf", &poses[i]) != 1) return 2;
  fclose(in);

  using namespace glim_amd::ba;
  std::vector<double> mom((size_t)BA_MOM * K), ws(ba_workspace_doubles(K)), g(6 * (size_t)K), H(36 * (size_t)K * K);
  ba_moments_host(n, pts.data(), frame.data(), K, mom.data());
  double cost = 0.0;
  const unsigned int status = ba_linearize_host(K, kind, mom.data(), poses.data(), ws.data(), &cost, g.data(), H.data());
  double cost_only = 0.0;
  const unsigned int status2 = ba_linearize_host(K, kind, mom.data(), poses.data(), ws.data(), &cost_only, nullptr, nullptr);
  if (status2 != status || (status != ~0u && cost_only != cost)) return 3;

  FILE* out = fopen(argv[2], "w");
  if (!out) return 2;
  fprintf(out, "%u\n%.17g\n", status, cost);
  if (status != ~0u) {
    for (double v : g) fprintf(out, "%.17g\n", v);
    for (double v : H) fprintf(out, "%.17g\n", v);
    double M[9], lam[3], U[9];
    const int ld = 6 * K;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) M[3 * r + c] = H[(size_t)r * ld + c] + H[(size_t)c * ld + r];
    glim_amd::eig3::direct(M, lam, U);
    for (double v : lam) fprintf(out, "%.17g\n", v);
    for (double v : U) fprintf(out, "%.17g\n", v);
  }
  fclose(out);
  return 0;
}
