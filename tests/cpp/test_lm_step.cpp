// glim_amd/csrc/lm_step.hpp under a plain C++ compiler: the statements the decide kernels of gicp_align.hip and vgicp_align.hip run, fed the records of a file.
//   in  (doubles): 9 parameters in glim_amd_lm_params order (max_trials resolved), 12 of the initial pose, N, then N records of 29
//   out (doubles): per record, the state after the round: 12 kept pose, 12 next candidate, 6 delta, lambda, solve_ok, iterations, trials,
//                  status, accepted (36 per round)
// tests/test_gicp_align.py writes the records (the oracle's, at the restatement's poses) and compares every round with tests/lm_restatement.py.
#include <cstdio>
#include <vector>

#include "../../glim_amd/csrc/lm_step.hpp"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  double head[22];
  if (fread(head, sizeof(double), 22, f) != 22) return 2;
  glim_amd::lm::Params p{head[0], head[1], head[2], head[3], head[4], head[5], (int)head[6], (int)head[7], head[8]};
  const int n = (int)head[21];
  std::vector<double> recs((size_t)n * 29);
  if (fread(recs.data(), sizeof(double), recs.size(), f) != recs.size()) return 2;
  fclose(f);
  glim_amd::lm::State s;
  glim_amd::lm::init(p, head + 9, s);
  std::vector<double> out;
  for (int k = 0; k < n; k++) {
    glim_amd::lm::step(p, s, recs.data() + 29 * (size_t)k);
    out.insert(out.end(), s.T, s.T + 12);
    out.insert(out.end(), s.cand, s.cand + 12);
    out.insert(out.end(), s.delta, s.delta + 6);
    const double tail[6] = {s.lambda, (double)s.solve_ok, (double)s.iterations, (double)s.trials, (double)s.status, (double)s.accepted};
    out.insert(out.end(), tail, tail + 6);
  }
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 2;
  fwrite(out.data(), sizeof(double), out.size(), g);
  fclose(g);
  printf("test_lm_step OK (%d rounds, status %d)\n", n, s.status);
  return 0;
}
