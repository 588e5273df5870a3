// glim_amd/csrc/ct_se3.hpp under a plain C++ compiler, one routine at a time, fed from a file: what tests/test_se3_range.py compares with the
// multiprecision table tests/golden/se3_range.npz.  Usage: test_se3_range <op> <in> <out>; in: cases x IN doubles, out: cases x OUT doubles.
//   op              IN                         OUT
//   exp             6  xi                      12 T
//   log             12 T                       6  xi
//   jr              6  xi                      36 J_r(xi)
//   jr_inv          6  xi                      36 J_r(xi)^-1
//   ad              12 T                       36 Ad(T)
//   prior           24 P | X                   42 r | d r / d X
//   between         36 D | X | Y               78 r | J (6 x 12)
//   ct              25 X | Y | t_k             84 T_k | D0_k | D1_k
// The same table as glim_amd_debug_se3_eval (include/glim_amd_diag.h), which runs it on the device.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../glim_amd/csrc/ct_se3.hpp"

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
  using namespace glim_amd::ct_se3;
  if (argc < 4) return 2;
  static const char* names[SE3_EVAL_OPS] = {"exp", "log", "jr", "jr_inv", "ad", "prior", "between", "ct"};
  int op = -1;
  for (int k = 0; k < SE3_EVAL_OPS; k++)
    if (!strcmp(argv[1], names[k])) op = k;
  if (op < 0) return 2;
  std::vector<double> in;
  if (!read_all(argv[2], in)) return 2;
  const size_t ni = (size_t)se3_eval_in(op), no = (size_t)se3_eval_out(op);
  if (in.size() % ni) return 2;
  const size_t n = in.size() / ni;
  std::vector<double> out(n * no);
  for (size_t k = 0; k < n; k++) se3_eval(op, in.data() + k * ni, out.data() + k * no);
  if (!write_all(argv[3], out)) return 2;
  printf("test_se3_range OK (%s, %zu cases)\n", argv[1], n);
  return 0;
}
