// Stand-alone host program of tests/test_record_expand.py: the expansion of a compact record into the caller's dense blocks
// (glim_amd/csrc/record_expand.hpp) on seeded finite records, unary and binary.
//   hash_old   the six-term products over the full 6x6 adjoint, as the library computed them before the zero block was skipped (kept here)
//   hash_new   glim_amd::binary_adjoint + glim_amd::expand_compact_record
// Both are FNV-1a hashes over the bit patterns of every glim_amd_linearized6.  The inputs are made with integer arithmetic and exact scalings
// only, so two builds of this program (-O0 / -O3 -march=native) see the same records.
// With `time` as the second argument the program reports nanoseconds per call of both forms instead (binary records).
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "record_expand.hpp"

namespace {

constexpr int COMPACT_DOUBLES = 29;

uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint64_t next_u64() {  // splitmix64
  uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// uniform in (-1, 1) times 2^e, e in [-max_exp, max_exp]: a 53-bit integer scaled by powers of two (exact)
double next_double(int max_exp) {
  const uint64_t u = next_u64();
  const double m = std::ldexp((double)(int64_t)(u >> 11), -52) - 1.0;
  const int e = max_exp ? (int)(next_u64() % (uint64_t)(2 * max_exp + 1)) - max_exp : 0;
  return std::ldexp(m, e);
}

// the expansion as it was: full six-term sums over a 6x6 Ad with its zero block stored
void expand_old(const double* c, const double* T, bool binary, glim_amd_linearized6* out) {
#pragma clang fp contract(off)
  memset(out, 0, sizeof(*out));
  out->num_inliers = (int64_t)llround(c[0]);
  out->error = c[1];
  int k = 2;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++) {
      out->H_ss[6 * i + j] = c[k];
      out->H_ss[6 * j + i] = c[k];
      k++;
    }
  for (int i = 0; i < 6; i++) out->b_s[i] = c[k++];
  if (!binary) return;
  double Rt[9], Ht[9], Ad[36];
  for (int r = 0; r < 3; r++)
    for (int cc = 0; cc < 3; cc++) Rt[3 * r + cc] = T[4 * cc + r];
  const double t[3] = {T[3], T[7], T[11]};
  Ht[0] = 0; Ht[1] = -t[2]; Ht[2] = t[1];
  Ht[3] = t[2]; Ht[4] = 0; Ht[5] = -t[0];
  Ht[6] = -t[1]; Ht[7] = t[0]; Ht[8] = 0;
  memset(Ad, 0, sizeof(Ad));
  for (int r = 0; r < 3; r++)
    for (int cc = 0; cc < 3; cc++) {
      Ad[6 * r + cc] = Rt[3 * r + cc];
      Ad[6 * (r + 3) + cc + 3] = Rt[3 * r + cc];
      double s = 0.0;
      for (int m = 0; m < 3; m++) s += Rt[3 * r + m] * Ht[3 * m + cc];
      Ad[6 * (r + 3) + cc] = -s;
    }
  double AtH[36];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double s = 0.0;
      for (int m = 0; m < 6; m++) s += Ad[6 * m + i] * out->H_ss[6 * m + j];
      AtH[6 * i + j] = s;
    }
  for (int i = 0; i < 6; i++) {
    for (int j = 0; j < 6; j++) {
      double s = 0.0;
      for (int m = 0; m < 6; m++) s += AtH[6 * i + m] * Ad[6 * m + j];
      out->H_tt[6 * i + j] = s;
      out->H_ts[6 * i + j] = -AtH[6 * i + j];
    }
    double s = 0.0;
    for (int m = 0; m < 6; m++) s += Ad[6 * m + i] * out->b_s[m];
    out->b_t[i] = -s;
  }
  for (int i = 0; i < 6; i++)
    for (int j = i + 1; j < 6; j++) {
      const double s = 0.5 * (out->H_tt[6 * i + j] + out->H_tt[6 * j + i]);
      out->H_tt[6 * i + j] = out->H_tt[6 * j + i] = s;
    }
}

void expand_new(const double* c, const double* T, bool binary, glim_amd_linearized6* out) {
  double adj[glim_amd::ADJOINT_DOUBLES];
  if (binary) glim_amd::binary_adjoint(T, adj);
  glim_amd::expand_compact_record(c, binary ? adj : nullptr, out);
}

uint64_t g_hash[2] = {0xcbf29ce484222325ull, 0xcbf29ce484222325ull};
void hash_bytes(int which, const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; i++) {
    g_hash[which] ^= b[i];
    g_hash[which] *= 0x100000001b3ull;
  }
}
void hash_out(int which, const glim_amd_linearized6& o) {
  hash_bytes(which, &o.num_inliers, sizeof(o.num_inliers));
  hash_bytes(which, &o.error, sizeof(o.error));
  hash_bytes(which, o.H_tt, sizeof(o.H_tt));
  hash_bytes(which, o.H_ts, sizeof(o.H_ts));
  hash_bytes(which, o.H_ss, sizeof(o.H_ss));
  hash_bytes(which, o.b_t, sizeof(o.b_t));
  hash_bytes(which, o.b_s, sizeof(o.b_s));
}
long count_mismatch(const double* a, const double* b, int n) {
  long m = 0;
  for (int i = 0; i < n; i++) m += memcmp(&a[i], &b[i], 8) != 0;
  return m;
}

void make_record(long k, double* c, double* T) {
  const int max_exp = (int)(k % 4) * 10;  // every fourth record on one scale, the others spread over up to 2^+-30
  c[0] = (double)(next_u64() % 200000ull);
  for (int i = 1; i < COMPACT_DOUBLES; i++) c[i] = next_double(max_exp);
  for (int i = 0; i < 12; i++) T[i] = next_double(k % 8 == 7 ? 4 : 0);
  if (k % 16 == 3) c[1 + next_u64() % 28] = 0.0;
  if (k % 16 == 5) c[1 + next_u64() % 28] = -0.0;
  if (k % 64 == 9) T[next_u64() % 12] = 0.0;
  if (k % 64 == 11) T[next_u64() % 12] = -0.0;
}

}  // namespace

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 100000;
  double c[COMPACT_DOUBLES], T[12];
  if (argc > 2 && strcmp(argv[2], "time") == 0) {
    make_record(1, c, T);
    glim_amd_linearized6 o;
    double sink = 0.0, adj[glim_amd::ADJOINT_DOUBLES];
    glim_amd::binary_adjoint(T, adj);
    for (int which = 0; which < 3; which++) {
      const auto t0 = std::chrono::steady_clock::now();
      for (long k = 0; k < n; k++) {
        c[1] = (double)k;  // (keeps the call inside the loop)
        if (which == 0) expand_old(c, T, true, &o);
        else if (which == 1) expand_new(c, T, true, &o);
        else glim_amd::expand_compact_record(c, adj, &o);  // the synchronous call's share once the record has arrived: the adjoint was ready
        __asm__ volatile("" : : "r"(&o) : "memory");
        sink += o.H_tt[7];
      }
      const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / (double)n;
      printf("%s_ns %.1f\n", which == 0 ? "expand_old" : (which == 1 ? "expand_new" : "expand_given_adjoint"), ns);
    }
    printf("sink %g\n", sink);
    return 0;
  }
  long mismatch = 0;
  glim_amd_linearized6 a, b;
  for (long k = 0; k < n; k++) {
    make_record(k, c, T);
    const bool binary = k % 3 != 0;
    expand_old(c, T, binary, &a);
    expand_new(c, T, binary, &b);
    hash_out(0, a);
    hash_out(1, b);
    mismatch += a.num_inliers != b.num_inliers;
    mismatch += count_mismatch(&a.error, &b.error, 1) + count_mismatch(a.H_tt, b.H_tt, 36) + count_mismatch(a.H_ts, b.H_ts, 36) + count_mismatch(a.H_ss, b.H_ss, 36) +
                count_mismatch(a.b_t, b.b_t, 6) + count_mismatch(a.b_s, b.b_s, 6);
  }
  printf("records %ld\n", n);
  printf("hash_old %016llx\n", (unsigned long long)g_hash[0]);
  printf("hash_new %016llx\n", (unsigned long long)g_hash[1]);
  printf("mismatching_values %ld\n", mismatch);
  return 0;
}
