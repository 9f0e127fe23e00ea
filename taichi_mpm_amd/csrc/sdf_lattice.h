// taichi_mpm_amd/csrc/sdf_lattice.h — what every entry point that takes a sampled field's lattice demands of it (host only: no HIP
// header, no ctx; rules: include/mpmhip.h).  Its callers are mpmhip_set_levelset_sdf, mpmhip2d_set_levelset_sdf, the seeding of
// either dimension (seed_api.h) and the mesh voxeliser's two entries (mesh_sdf_api.h); each puts its own name in front of the reason.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

namespace sdf_lattice {

// the number of samples of a lattice of D axes; 0: the lattice is refused and `why` says what is wrong with it
template <int D>
size_t check(const int32_t *res, const float *origin, float spacing, std::string &why) {
  const size_t limit = (size_t)1 << 31;
  size_t count = 1;
  for (int k = 0; k < D; k++) {
    const std::string ax = "[" + std::to_string(k) + "]";
    if (res[k] < 2) { why = "res" + ax + " = " + std::to_string(res[k]) + ", at least 2 samples per axis are needed"; return 0; }
    if (!std::isfinite(origin[k])) { why = "origin" + ax + " is not finite"; return 0; }
    if (count <= limit) count *= (size_t)res[k];  // (beyond the limit it stays there: three axes of 2^31 would wrap 64 bits)
  }
  if (!(spacing > 0.0f) || !std::isfinite(spacing)) { why = "spacing must be a finite number > 0"; return 0; }
  if (count > limit) { why = "more than 2^31 samples"; return 0; }
  return count;
}

}  // namespace sdf_lattice
