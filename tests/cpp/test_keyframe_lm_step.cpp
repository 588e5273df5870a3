// glim_amd/csrc/keyframe_lm_step.hpp under a plain C++ compiler, as the only include: the statements vgicp_align.hip's keyframe decide kernel
// runs, fed from a file.
//   step      in : 9 parameters in glim_amd_lm_params order (max_trials resolved), M, has_prior, M x 12 target poses P_f, [12 of the prior's
//                  pose, 36 of its information], 12 of X_init, R, then R x M x 29 records (round r's: evaluated at the T_f round r reports)
//             out: per round: the T_f the round evaluated (12 M), the summed record (29), the prior's contribution (28), then the state after
//                  it: kept pose (12), next candidate (12), delta (6), lambda, solve_ok, iterations, trials, status, accepted
// tests/test_keyframe_align.py writes the inputs and compares with tests/keyframe_restatement.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../glim_amd/csrc/keyframe_lm_step.hpp"

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

int main(int argc, char** argv) {
  if (argc != 4 || strcmp(argv[1], "step") != 0) {
    fprintf(stderr, "usage: %s step <in> <out>\n", argv[0]);
    return 2;
  }
  std::vector<double> in, out;
  if (!read_all(argv[2], in) || in.size() < 11) return 3;
  lm::Params p;
  p.lambda_initial = in[0];
  p.lambda_factor = in[1];
  p.lambda_upper_bound = in[2];
  p.lambda_lower_bound = in[3];
  p.relative_error_tol = in[4];
  p.absolute_error_tol = in[5];
  p.max_iterations = (int)in[6];
  p.max_trials = (int)in[7];
  p.error_scale = in[8];
  const int M = (int)in[9], has_prior = (int)in[10];
  if (M < 1 || M > keyframe_lm::MAX_TARGETS) return 3;
  size_t at = 11;
  const size_t head = at + 12 * (size_t)M + (has_prior ? keyframe_lm::PRIOR_TERM : 0) + 12 + 1;
  if (in.size() < head) return 3;
  std::vector<double> Pinv(12 * (size_t)M), Tf(12 * (size_t)M);
  for (int f = 0; f < M; f++, at += 12) keyframe_lm::target_inverse(&in[at], &Pinv[12 * (size_t)f]);
  const double* term = nullptr;
  if (has_prior) {
    term = &in[at];
    at += keyframe_lm::PRIOR_TERM;
  }
  lm::State s;
  lm::init(p, &in[at], s);
  at += 12;
  const int R = (int)in[at++];
  if (R < 0 || in.size() != head + (size_t)R * M * lm::RECORD) return 3;
  for (int f = 0; f < M; f++) keyframe_lm::factor_pose(&Pinv[12 * (size_t)f], s.cand, &Tf[12 * (size_t)f]);
  for (int r = 0; r < R; r++, at += (size_t)M * lm::RECORD) {
    double sum[lm::RECORD] = {0.0}, pc[keyframe_lm::PRIOR] = {0.0};
    out.insert(out.end(), Tf.begin(), Tf.end());
    keyframe_lm::step(p, s, M, Pinv.data(), term, &in[at], Tf.data(), sum, pc);
    out.insert(out.end(), sum, sum + lm::RECORD);
    out.insert(out.end(), pc, pc + keyframe_lm::PRIOR);
    out.insert(out.end(), s.T, s.T + 12);
    out.insert(out.end(), s.cand, s.cand + 12);
    out.insert(out.end(), s.delta, s.delta + 6);
    const double tail[6] = {s.lambda, (double)s.solve_ok, (double)s.iterations, (double)s.trials, (double)s.status, (double)s.accepted};
    out.insert(out.end(), tail, tail + 6);
  }
  if (!write_all(argv[3], out)) return 4;
  printf("test_keyframe_lm_step OK (%d targets, %d rounds)\n", M, R);
  return 0;
}
