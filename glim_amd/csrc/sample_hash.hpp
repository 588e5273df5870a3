// sample_hash.hpp -- the counter-based generator of every random draw on the device: splitmix64 of seed + (index + 1) * golden.
// preprocess.hip (random-grid sampling; oracle/preprocess_oracle.c states it as orc_sample_hash), ransac.hip (the three draws of a hypothesis) and
// gnc.hip (candidate marks, tuple trials) use it; tests/ransac_restatement.py restates it.
#pragma once
#include <hip/hip_runtime.h>

namespace glim_amd {
__host__ __device__ inline unsigned long long sample_hash(unsigned long long seed, unsigned long long index) {
  unsigned long long z = seed + (index + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
}  // namespace glim_amd
