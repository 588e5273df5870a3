// Stand-alone host program of tests/test_pose_granule.py: the pose granule {lo32, tag, hi32, tag} of a resident session
// (glim_amd/csrc/pose_granule.hpp).  Packs seeded 64-bit patterns under seeded tags into the two 8-byte halves the host stores, reads them back
// as the four 32-bit words a block loads, and checks that
//   * a granule whose halves were written under one tag unpacks to that tag and the same 64 bits        (round_trip_failures)
//   * a granule with one half of another request -- either half, any other tag -- is not whole          (foreign_halves_accepted)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pose_granule.hpp"

namespace {
uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint64_t next_u64() {  // splitmix64
  uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
bool load(const uint64_t half[2], uint32_t* tag, uint64_t* bits) {
  uint32_t w[4];
  memcpy(w, half, 16);  // (the words as a 16-byte load returns them)
  return glim_amd::unpack_pose_granule(w[0], w[1], w[2], w[3], tag, bits);
}
}  // namespace

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 100000;
  long round_trip_failures = 0, foreign_halves_accepted = 0;
  for (long k = 0; k < n; k++) {
    uint64_t bits = next_u64();
    if (k % 16 == 1) bits = 0ull;
    if (k % 16 == 2) bits = ~0ull;
    if (k % 16 == 3) bits = 0xffffffff00000000ull | (uint32_t)next_u64();  // (a value word that looks like the exit tag)
    uint32_t tag = 0x80000000u | (uint32_t)next_u64();
    if (k % 32 == 5) tag = 0xffffffffu;  // the exit tag
    uint32_t other = 0x80000000u | (uint32_t)next_u64();
    if (k % 8 == 0) other = tag + 1u;  // the neighbouring request
    if (k % 8 == 1) other = 0u;        // a cleared granule
    if (k % 8 == 2) other = 0xffffffffu;
    if (other == tag) other = tag ^ 1u;
    uint64_t mine[2], theirs[2];
    glim_amd::pack_pose_granule(bits, tag, &mine[0], &mine[1]);
    glim_amd::pack_pose_granule(next_u64(), other, &theirs[0], &theirs[1]);
    uint32_t t = 0;
    uint64_t b = 0;
    if (!load(mine, &t, &b) || t != tag || b != bits) round_trip_failures++;
    const uint64_t mixed_a[2] = {mine[0], theirs[1]}, mixed_b[2] = {theirs[0], mine[1]};
    if (load(mixed_a, &t, &b)) foreign_halves_accepted++;
    if (load(mixed_b, &t, &b)) foreign_halves_accepted++;
  }
  printf("granules %ld\n", n);
  printf("round_trip_failures %ld\n", round_trip_failures);
  printf("foreign_halves_accepted %ld\n", foreign_halves_accepted);
  return 0;
}
