// tests/cpp/sdf_lattice_host.cpp — taichi_mpm_amd/csrc/sdf_lattice.h alone, compiled for the host (tests/test_sdf_lattice_cpu.py runs it
// under AddressSanitizer and UBSan): the accepting and the refusing cases of both dimensions, with the words every entry point puts
// behind its own name.
#include <cstdio>
#include <limits>
#include <string>

#include "../../taichi_mpm_amd/csrc/sdf_lattice.h"

static int failures = 0;

template <int D>
static void expect(int line, const int32_t (&res)[D], const float (&origin)[D], float spacing, size_t count, const char *why) {
  std::string got = "untouched";
  const size_t n = sdf_lattice::check<D>(res, origin, spacing, got);
  if (n != count || (count == 0 && got != why) || (count != 0 && got != "untouched")) {
    printf("line %d: count %zu (expected %zu), reason '%s' (expected '%s')\n", line, n, count, got.c_str(), why);
    failures++;
  }
}
#define EXPECT(D, res, origin, spacing, count, why)  \
  do {                                                \
    const int32_t r_[D] = res;                        \
    const float o_[D] = origin;                       \
    expect<D>(__LINE__, r_, o_, spacing, count, why); \
  } while (0)
#define A(...) {__VA_ARGS__}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  EXPECT(3, A(4, 5, 6), A(0, -1, 2.5f), 0.1f, 120, "");
  EXPECT(2, A(2, 2), A(0, 0), 1e-30f, 4, "");
  EXPECT(3, A(2048, 1024, 1024), A(0, 0, 0), 1.0f, (size_t)1 << 31, "");  // 2^31 samples are allowed
  EXPECT(2, A(65536, 32768), A(0, 0), 1.0f, (size_t)1 << 31, "");
  EXPECT(3, A(2048, 2048, 1024), A(0, 0, 0), 1.0f, 0, "more than 2^31 samples");
  EXPECT(3, A(2147483647, 2147483647, 2147483647), A(0, 0, 0), 1.0f, 0, "more than 2^31 samples");  // (2^93: the count must not wrap)
  EXPECT(3, A(65536, 65536, 65536), A(0, 0, 0), 1.0f, 0, "more than 2^31 samples");  // (2^48)
  EXPECT(2, A(65536, 32769), A(0, 0), 1.0f, 0, "more than 2^31 samples");
  EXPECT(3, A(1, 4, 4), A(0, 0, 0), 0.1f, 0, "res[0] = 1, at least 2 samples per axis are needed");
  EXPECT(3, A(4, 4, -7), A(0, 0, 0), 0.1f, 0, "res[2] = -7, at least 2 samples per axis are needed");
  EXPECT(2, A(4, 0), A(0, 0), 0.1f, 0, "res[1] = 0, at least 2 samples per axis are needed");
  EXPECT(3, A(4, 4, 4), A(0, inf, 0), 0.1f, 0, "origin[1] is not finite");
  EXPECT(2, A(4, 4), A(nan, 0), 0.1f, 0, "origin[0] is not finite");
  EXPECT(3, A(4, 1, 4), A(-inf, 0, 0), 0.1f, 0, "origin[0] is not finite");  // axis by axis: res[k], then origin[k]
  EXPECT(3, A(4, 1, 4), A(0, nan, 0), 0.0f, 0, "res[1] = 1, at least 2 samples per axis are needed");
  EXPECT(2, A(4, 4), A(0, 0), 0.0f, 0, "spacing must be a finite number > 0");
  EXPECT(3, A(4, 4, 4), A(0, 0, 0), -1.0f, 0, "spacing must be a finite number > 0");
  EXPECT(3, A(4, 4, 4), A(0, 0, 0), nan, 0, "spacing must be a finite number > 0");
  EXPECT(2, A(4, 4), A(0, 0), inf, 0, "spacing must be a finite number > 0");
  EXPECT(2, A(65536, 65536), A(0, 0), nan, 0, "spacing must be a finite number > 0");  // the spacing before the count
  printf(failures ? "%d cases failed\n" : "cases ok\n", failures);
  return failures != 0;
}
