// The pose step of the GNC global registration (glim_amd/csrc/gnc_pose.hpp) on the CPU: the statements the solve kernel runs once per iteration,
// compiled by a plain C++ compiler (and once more under -fsanitize=address,undefined).
//   test_gnc_pose <in.txt> <out.txt>
// in : one case per line: dof W a0 a1 a2 b0 b1 b2 M00 .. M22 cs0 cs1 cs2 ct0 ct1 ct2   (hexadecimal floating point: exact)
// out: one line per case: ok T[0] .. T[11]                                             (likewise)
#include <cstdio>

#include "../../glim_amd/csrc/gnc_pose.hpp"

int main(int argc, char** argv) {
  if (argc < 3) {
    std::printf("usage: test_gnc_pose <in.txt> <out.txt>\n");
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "r");
  std::FILE* out = std::fopen(argv[2], "w");
  if (!in || !out) return 1;
  int cases = 0;
  for (;;) {
    int dof = 0;
    double v[22];  // W | a | b | M | cs | ct
    if (std::fscanf(in, "%d", &dof) != 1) break;
    bool ok = true;
    for (int i = 0; i < 22; i++) ok = ok && std::fscanf(in, "%la", &v[i]) == 1;
    if (!ok) return 1;
    double T[12];
    const bool fine = glim_amd::gnc_pose::pose_from_moments(v[0], v + 1, v + 4, v + 7, v + 16, v + 19, dof, T);
    std::fprintf(out, "%d", fine ? 1 : 0);
    for (int i = 0; i < 12; i++) std::fprintf(out, " %a", T[i]);
    std::fprintf(out, "\n");
    cases++;
  }
  std::fclose(in);
  std::fclose(out);
  std::printf("test_gnc_pose OK (%d cases)\n", cases);
  return 0;
}
