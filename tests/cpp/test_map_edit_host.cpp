// Stand-alone host program over the plain-C++ side of glim_amd/csrc/map_edit.hpp: the four selection predicates, the edge test and the packed
// point ids, through the very functions the kernels of map_edit.hip call.  tests/test_map_edit.py writes the input, builds this file plain
// and with -fsanitize=address,undefined, runs it directly and compares the output with tests/map_edit_restatement.py.
//
//   input : resolution window radius cx cy cz | 12 matrix entries (3x4 row-major) | threshold cos_angle | n | n lines "x y z nx ny nz"
//   output: four lines of n flags (BOX, SPHERE, WINDOW, WINDOW_BALL of the transformed points), then n lines of n flags: edge(i, j) with normals
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../glim_amd/csrc/map_edit.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "r");
  if (!in) return 2;
  using namespace glim_amd::edit;
  double resolution = 0, radius = 0, c[3], M[12], thr = 0, cosang = 0;
  int window = 0;
  long n = 0;
  if (fscanf(in, "%lf %d %lf %lf %lf %lf", &resolution, &window, &radius, &c[0], &c[1], &c[2]) != 6) return 2;
  for (double& m : M)
    if (fscanf(in, "%lf", &m) != 1) return 2;
  if (fscanf(in, "%lf %lf %ld", &thr, &cosang, &n) != 3 || n < 0) return 2;
  std::vector<double> p(6 * (size_t)n), v(3 * (size_t)n), nw(3 * (size_t)n);
  for (double& x : p)
    if (fscanf(in, "%lf", &x) != 1) return 2;
  fclose(in);

  for (long i = 0; i < n; i++) {
    transform(M, p[6 * i], p[6 * i + 1], p[6 * i + 2], &v[3 * (size_t)i]);
    rotate(M, p[6 * i + 3], p[6 * i + 4], p[6 * i + 5], &nw[3 * (size_t)i]);
  }
  FILE* out = fopen(argv[2], "w");
  if (!out) return 2;
  for (int mode = MODE_BOX; mode <= MODE_WINDOW_BALL; mode++) {
    Predicate pred = Predicate();
    pred.mode = mode;
    window_bounds(c, resolution, window, &pred);
    pred.r2 = radius * radius;
    for (long i = 0; i < n; i++) fprintf(out, "%d ", selected(pred, &v[3 * (size_t)i]) ? 1 : 0);
    fprintf(out, "\n");
  }
  for (long i = 0; i < n; i++) {
    for (long j = 0; j < n; j++) fprintf(out, "%d ", edge(&v[3 * (size_t)i], &v[3 * (size_t)j], thr * thr, &nw[3 * (size_t)i], &nw[3 * (size_t)j], cosang) ? 1 : 0);
    fprintf(out, "\n");
  }
  fclose(out);
  // the packed ids: a round trip at the ends of both fields
  const int32_t subs[3] = {0, 1, 0x7fffffff}, pts[3] = {0, 5, 0x7fffffff};
  for (int32_t s : subs)
    for (int32_t q : pts) {
      const uint64_t id = pack_id(s, q);
      if (id_submap(id) != s || id_point(id) != q || (id >> 32) != (uint64_t)s) return 3;
    }
  return 0;
}
