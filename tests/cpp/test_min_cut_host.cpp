// Stand-alone host program over the plain-C++ side of glim_amd/csrc/map_edit.hpp, min-cut part: the edge weights and their integer
// capacities, through the very functions the kernels of map_edit.hip call.  tests/test_min_cut.py writes the input, builds this file plain
// and with -fsanitize=address,undefined, runs it directly and compares the output with tests/min_cut_restatement.py.
//
//   input : sigma_d sigma_a n | n lines "ax ay az bx by bz nax nay naz nbx nby nbz" | w weights, one per line after their count
//   output: n lines "capacity_without_normals capacity_with_normals", then per weight "fits quantised"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../glim_amd/csrc/map_edit.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "r");
  if (!in) return 2;
  using namespace glim_amd::edit;
  double sigma_d = 0, sigma_a = 0;
  long n = 0, nw = 0;
  if (fscanf(in, "%lf %lf %ld", &sigma_d, &sigma_a, &n) != 3 || n < 0) return 2;
  std::vector<double> e(12 * (size_t)n);
  for (double& x : e)
    if (fscanf(in, "%lf", &x) != 1) return 2;
  if (fscanf(in, "%ld", &nw) != 1 || nw < 0) return 2;
  std::vector<double> weights((size_t)nw);
  for (double& x : weights)
    if (fscanf(in, "%lf", &x) != 1) return 2;
  fclose(in);
  FILE* out = fopen(argv[2], "w");
  if (!out) return 2;
  for (long i = 0; i < n; i++) {
    const double* r = &e[12 * (size_t)i];
    fprintf(out, "%d %d\n", (int)min_cut_edge_capacity(r, r + 3, sigma_d, nullptr, nullptr, 0.0), (int)min_cut_edge_capacity(r, r + 3, sigma_d, r + 6, r + 9, sigma_a));
  }
  for (double w : weights) fprintf(out, "%d %d\n", capacity_fits(w) ? 1 : 0, capacity_fits(w) ? (int)quantize_capacity(w) : -1);
  fclose(out);
  return CAP_SCALE == 65536.0 ? 0 : 3;
}
