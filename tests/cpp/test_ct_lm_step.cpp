// glim_amd/csrc/ct_lm_step.hpp and ct_se3.hpp under a plain C++ compiler: the statements ct_align.hip's kernels run, fed from a file.
//   step  in  (doubles): 9 parameters in glim_amd_lm_params order (max_trials resolved), 12 + 12 of the initial pair, 26 of the terms
//                        (T_location, location_precision, T_between, between_precision), N, then N records of 92
//         out (doubles): per record, the state after the round: kept X, Y (24), next candidate X, Y (24), delta (12), lambda, solve_ok,
//                        iterations, trials, status, accepted, the kept total cost (67 per round)
//   poses in  (doubles): 12 + 12 of the pair, N, then N bucket times
//         out (doubles): the pose table, 84 per bucket (T_k | D0_k | D1_k)
// tests/test_ct_align.py writes the inputs and compares with tests/ct_lm_restatement.py and tests/ct_restatement.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../glim_amd/csrc/ct_lm_step.hpp"

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

int main(int argc, char** argv) {
  using namespace glim_amd;
  if (argc < 4) return 2;
  std::vector<double> in, out;
  if (!read_all(argv[2], in)) return 2;
  if (!strcmp(argv[1], "poses")) {
    if (in.size() < 25) return 2;
    const size_t n = (size_t)in[24];
    if (in.size() != 25 + n) return 2;
    out.resize(n * ct_se3::CT_POSE_STRIDE);
    ct_se3::ct_pose_table(in.data() + 25, n, in.data(), in.data() + 12, out.data());
    if (!write_all(argv[3], out)) return 2;
    printf("test_ct_lm_step OK (%zu buckets)\n", n);
    return 0;
  }
  if (strcmp(argv[1], "step") || in.size() < 60) return 2;
  const double* h = in.data();
  lm::Params p{h[0], h[1], h[2], h[3], h[4], h[5], (int)h[6], (int)h[7], h[8]};
  ct_lm::Terms t;
  static_assert(sizeof(t) == 26 * sizeof(double), "the terms are 26 doubles");
  memcpy(&t, h + 33, sizeof(t));
  const size_t n = (size_t)h[59];
  if (in.size() != 60 + n * ct_lm::RECORD) return 2;
  ct_lm::State s;
  ct_lm::init(p, h + 9, h + 21, s);
  double work[ct_lm::WORK];
  for (size_t k = 0; k < n; k++) {
    ct_lm::step(p, t, s, h + 60 + ct_lm::RECORD * k, work);
    out.insert(out.end(), s.X, s.X + 12);
    out.insert(out.end(), s.Y, s.Y + 12);
    out.insert(out.end(), s.candX, s.candX + 12);
    out.insert(out.end(), s.candY, s.candY + 12);
    out.insert(out.end(), s.delta, s.delta + 12);
    const double tail[7] = {s.lambda, (double)s.solve_ok, (double)s.iterations, (double)s.trials, (double)s.status, (double)s.accepted, s.sys[1]};
    out.insert(out.end(), tail, tail + 7);
  }
  if (!write_all(argv[3], out)) return 2;
  printf("test_ct_lm_step OK (%zu rounds, status %d)\n", n, s.status);
  return 0;
}
