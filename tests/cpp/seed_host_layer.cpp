// MPM<3>::add_particles_region of the C++ host layer (include/mpm_amd/mpm.h) for tests/test_gpu_seed.py: seeds the r = 12 dx sphere
// of the tests through shapes and prints what the test compares with the numpy model.
#include <cstdio>

#include "mpm_amd/mpm.h"

using namespace mpm_amd;

int main() {
  try {
    MPM<3> sim;
    sim.initialize(Config().set("res", Vector3i(64, 64, 64)).set("base_delta_t", 1e-4).set("max_particles", 1024.0));
    mpmhip_shape s{};
    s.type = 1;
    s.p[0] = s.p[1] = s.p[2] = 0.5f;
    s.p[3] = 12.0f / 64;
    const int64_t n = sim.add_particles_region(Config().set("type", "sand").set("ppc", 8.0), {s});
    const auto p = sim.get_render_particles();
    std::printf("%lld %lld %.9g %.9g %.9g\n", (long long)n, (long long)sim.get_num_particles(), p[0].position[0], p[0].position[1],
                p[0].position[2]);
  } catch (const std::exception &e) {
    std::printf("error: %s\n", e.what());
    return 1;
  }
  return 0;
}
