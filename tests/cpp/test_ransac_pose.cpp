// The three-point pose solver of the RANSAC global registration (glim_amd/csrc/ransac_pose.hpp) on the CPU: the statements the hypothesis kernel
// runs, compiled by a plain C++ compiler (and once more under -fsanitize=address,undefined).
//   test_ransac_pose <in.txt> <out.txt>
// in : one case per line: dof thresh s0x s0y s0z s1x .. s2z t0x .. t2z   (hexadecimal floating point: exact)
// out: one line per case: status T[0] .. T[11]                            (likewise; the identity where status != 0)
#include <cstdio>

#include "../../glim_amd/csrc/ransac_pose.hpp"

int main(int argc, char** argv) {
  if (argc < 3) {
    std::printf("usage: test_ransac_pose <in.txt> <out.txt>\n");
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "r");
  std::FILE* out = std::fopen(argv[2], "w");
  if (!in || !out) return 1;
  int cases = 0;
  for (;;) {
    int dof = 0;
    double thresh = 0.0, s[9], t[9];
    if (std::fscanf(in, "%d %la", &dof, &thresh) != 2) break;
    bool ok = true;
    for (int i = 0; i < 9; i++) ok = ok && std::fscanf(in, "%la", &s[i]) == 1;
    for (int i = 0; i < 9; i++) ok = ok && std::fscanf(in, "%la", &t[i]) == 1;
    if (!ok) return 1;
    double T[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    const int status = glim_amd::ransac_pose::solve_pose(s, t, thresh, dof, T);
    std::fprintf(out, "%d", status);
    for (int i = 0; i < 12; i++) std::fprintf(out, " %a", T[i]);
    std::fprintf(out, "\n");
    cases++;
  }
  std::fclose(in);
  std::fclose(out);
  std::printf("test_ransac_pose OK (%d cases)\n", cases);
  return 0;
}
