// Host build of taichi_mpm_amd/csrc/poisson_tile.h with D = 2 for tests/test_seed2d_cpu.py: the header alone, no HIP, no library.
#include "../../taichi_mpm_amd/csrc/poisson_tile.h"

#include <cstring>

// a fresh generation on every call (the library caches one per process): min(count, capacity) points to out, returns the count
extern "C" long long pt2_generate(float *out, long long capacity) {
  const std::vector<float> t = poisson_tile::generate<2>();
  const long long n = (long long)(t.size() / 2);
  if (out && capacity > 0) std::memcpy(out, t.data(), sizeof(float) * 2 * (size_t)(n < capacity ? n : capacity));
  return n;
}
