// sample_hash.hpp -- the counter-based generator of every random draw on the device: splitmix64 of seed + (index + 1) * golden.
// preprocess.hip (random-grid sampling; oracle/preprocess_oracle.c states it as orc_sample_hash), ransac.hip (the three draws of a hypothesis),
// gnc.hip (candidate marks, tuple trials) and resample.hip (the draw of a random sample, through resample.hpp) use it;
// tests/ransac_restatement.py restates it.  Plain C++ as well as HIP, so that a stand-alone host program can run it.
#pragma once

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define GLIM_AMD_HASH_HD __host__ __device__
#else
#define GLIM_AMD_HASH_HD
#endif

namespace glim_amd {
GLIM_AMD_HASH_HD inline unsigned long long sample_hash(unsigned long long seed, unsigned long long index) {
  unsigned long long z = seed + (index + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
}  // namespace glim_amd
