// pose_granule.hpp -- the 16-byte granule one pose value of a resident session travels in (vgicp.hip ResidentArgs::pose16): four 32-bit words
// {lo32, tag, hi32, tag}.  Whoever writes it -- the session's leader with one 16-byte store, or the host with two aligned 8-byte stores through
// the large BAR -- a reader takes it only when BOTH tags agree: an 8-byte half arrives as a unit, so a half that carries a tag carries that
// request's 32 bits, while nothing is assumed about the two halves arriving together or in order.
// Plain C++ as well as HIP: tests/test_pose_granule.py compiles a stand-alone host program against it.
#pragma once

#include <cstdint>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define GLIM_AMD_GRANULE_HD __host__ __device__
#else
#define GLIM_AMD_GRANULE_HD
#endif

namespace glim_amd {

// the two 8-byte halves (little endian: words {lo32, tag} and {hi32, tag}) of the granule of `bits` under `tag`
GLIM_AMD_GRANULE_HD inline void pack_pose_granule(uint64_t bits, uint32_t tag, uint64_t* half0, uint64_t* half1) {
  *half0 = (bits & 0xffffffffull) | ((uint64_t)tag << 32);
  *half1 = (bits >> 32) | ((uint64_t)tag << 32);
}

// words w0..w3 of a granule as loaded: its tag and value; false when the halves carry different tags (one of them is another request's, or
// not written yet) -- the granule is not whole and nothing of it may be used
GLIM_AMD_GRANULE_HD inline bool unpack_pose_granule(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t* tag, uint64_t* bits) {
  *tag = w1;
  *bits = ((uint64_t)w2 << 32) | (uint64_t)w0;
  return w1 == w3;
}

}  // namespace glim_amd
