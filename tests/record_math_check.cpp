// Stand-alone host program of tests/test_record_math.py: the record math of glim_amd/csrc/device_math.hpp on seeded random records.
//   hash_finish   the host's finish of a raw record (rotate_part + the slot mapping: finish_raw_record)
//   hash_element  the device finalisers' form (the single-path rotate_element per slot + the same mapping)
// Both are FNV-1a hashes over the bit patterns of every compact record.  The inputs are made with integer arithmetic and exact scalings only, so
// two builds of this program (-O0 / -O3 -march=native) see the same records and any difference between their hashes is the compiler's: a
// contracted multiply-add in the record math.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "device_math.hpp"

namespace {

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
  const double m = std::ldexp((double)(int64_t)(u >> 11), -52) - 1.0;  // (exact: a 53-bit integer / 2^52, minus one)
  const int e = max_exp ? (int)(next_u64() % (uint64_t)(2 * max_exp + 1)) - max_exp : 0;
  return std::ldexp(m, e);
}

uint64_t g_hash[2] = {0xcbf29ce484222325ull, 0xcbf29ce484222325ull};
void hash_record(int which, const double* rec) {
  for (int i = 0; i < glim_amd::RECORD_SLOTS; i++) {
    uint64_t bits;
    memcpy(&bits, &rec[i], 8);
    if (std::isnan(rec[i])) bits = 0x7ff8000000000000ull;  // (which NaN an operation returns is the hardware's choice, not the record math's)
    for (int b = 0; b < 8; b++) {
      g_hash[which] ^= (bits >> (8 * b)) & 0xffull;
      g_hash[which] *= 0x100000001b3ull;
    }
  }
}

// the device finalisers' form: one rotate_element per rotated slot, then the slot select of finalize_tail
void finish_by_element(const double* raw, const double* T, double* compact) {
  double rot[glim_amd::RECORD_ROTATED];
  for (int j = 0; j < glim_amd::RECORD_ROTATED; j++) rot[j] = glim_amd::rotate_element(j, raw, T);
  compact[0] = raw[28];
  compact[1] = raw[27];
  for (int t = 2; t < glim_amd::RECORD_SLOTS; t++) compact[t] = glim_amd::compact_from_rot(t, rot);
}

long g_mismatch = 0;
void run(const double* raw, const double* T, double* a) {
  double b[glim_amd::RECORD_SLOTS];
  glim_amd::finish_raw_record(raw, T, a);
  finish_by_element(raw, T, b);
  hash_record(0, a);
  hash_record(1, b);
  for (int i = 0; i < glim_amd::RECORD_SLOTS; i++) {
    const bool same = std::isnan(a[i]) ? std::isnan(b[i]) : memcmp(&a[i], &b[i], 8) == 0;
    if (!same) g_mismatch++;
  }
}

}  // namespace

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 100000;
  double raw[32], T[12], out[glim_amd::RECORD_SLOTS];
  for (long k = 0; k < n; k++) {
    const int max_exp = (int)(k % 4) * 10;  // every fourth record on one scale, the others spread over up to 2^+-30
    for (int i = 0; i < 32; i++) raw[i] = next_double(max_exp);
    for (int i = 0; i < 12; i++) T[i] = next_double(k % 8 == 7 ? 4 : 0);
    if (k % 16 == 3) raw[next_u64() % 27] = 0.0;
    if (k % 16 == 5) raw[next_u64() % 27] = -0.0;
    if (k % 64 == 9) T[next_u64() % 12] = 0.0;
    run(raw, T, out);
  }
  // an empty factor (nothing but zeros), its negative-zero twin, and a record whose finaliser lost a row (NaN in every raw slot)
  for (int i = 0; i < 12; i++) T[i] = next_double(0);
  for (int i = 0; i < 32; i++) raw[i] = 0.0;
  run(raw, T, out);
  for (int i = 0; i < 32; i++) raw[i] = -0.0;
  run(raw, T, out);
  for (int i = 0; i < 32; i++) raw[i] = std::nan("");
  run(raw, T, out);
  printf("records %ld\n", n + 3);
  printf("hash_finish %016llx\n", (unsigned long long)g_hash[0]);
  printf("hash_element %016llx\n", (unsigned long long)g_hash[1]);
  printf("mismatching_values %ld\n", g_mismatch);
  printf("nan_count_in_slot0 %d\n", std::isnan(out[0]) ? 1 : 0);
  return 0;
}
