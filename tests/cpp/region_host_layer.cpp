// add_particles_region(config, mpmhip_region_desc) of the C++ host layer (include/mpm_amd/mpm.h, mpm2d.h) for tests/test_gpu_region.py:
// seeds the clipped shell — (sphere r = 12 dx minus sphere r = 8 dx) below y = 0.5 + 2 dx — in 3D and the same annulus in 2D on
// contexts created for 1024 particles, and prints per dimension what the test compares with the numpy model: the count, the
// number of particles of the ctx, the first 16 particles in creation order.
#include <cstdio>

#include "mpm_amd/mpm.h"
#include "mpm_amd/mpm2d.h"

using namespace mpm_amd;

static mpmhip_region_desc clipped_shell(int dim) {
  mpmhip_region_desc r{};
  const float dx = 1.0f / 64;
  r.n_leaves = 3;
  for (int i = 0; i < 2; i++) {  // the two balls about the centre
    mpmhip_shape &s = r.leaves[i].shape;
    s.type = 1;
    s.p[0] = s.p[1] = 0.5f;
    s.p[2] = dim == 3 ? 0.5f : 0.0f;
    s.p[3] = (i == 0 ? 12.0f : 8.0f) * dx;
  }
  mpmhip_shape &cut = r.leaves[2].shape;  // y - (0.5 + 2 dx) < 0
  cut.type = 0;
  cut.p[1] = 1.0f;
  cut.p[3] = -(0.5f + 2.0f * dx);
  const mpmhip_region_op ops[6] = {{MPMHIP_REGION_PUSH, 0}, {MPMHIP_REGION_PUSH, 1}, {MPMHIP_REGION_NEG, 0},
                                   {MPMHIP_REGION_INTERSECT, 0}, {MPMHIP_REGION_PUSH, 2}, {MPMHIP_REGION_INTERSECT, 0}};
  r.n_ops = 6;
  for (int i = 0; i < 6; i++) r.ops[i] = ops[i];
  return r;
}

int main() {
  try {
    {
      MPM<3> sim;
      sim.initialize(Config().set("res", Vector3i(64, 64, 64)).set("base_delta_t", 1e-4).set("max_particles", 1024.0));
      const int64_t n = sim.add_particles_region(Config().set("type", "sand").set("ppc", 8.0), clipped_shell(3));
      const auto p = sim.get_render_particles();
      std::printf("%lld %lld", (long long)n, (long long)sim.get_num_particles());
      for (int i = 0; i < 16; i++) std::printf(" %.9g %.9g %.9g", p[i].position[0], p[i].position[1], p[i].position[2]);
      std::printf("\n");
    }
    {
      MPM<2> sim;
      sim.initialize(Config().set("res", "64,64").set("base_delta_t", 1e-4).set("max_particles", 1024.0));
      const int64_t n = sim.add_particles_region(Config().set("type", "sand").set("ppc", 4.0), clipped_shell(2));
      const auto p = sim.get_particles();  // ordered by creation id
      std::printf("%lld %lld", (long long)n, (long long)sim.get_num_particles());
      for (int i = 0; i < 16; i++) std::printf(" %.9g %.9g", p[i].position[0], p[i].position[1]);
      std::printf("\n");
    }
  } catch (const std::exception &e) {
    std::printf("error: %s\n", e.what());
    return 1;
  }
  return 0;
}
