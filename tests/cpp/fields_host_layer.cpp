// MPM<3>::download_device / upload_device of the C++ host layer (include/mpm_amd/mpm.h) for tests/test_gpu_fields_host_layer.py: the
// sphere of seed_host_layer.cpp; x, v and id come out into device arrays in id order and must be what get_render_particles() returns
// (the host path, sorted by id); v goes back doubled and must be read back doubled.  Prints "ok <particles>" or what differed.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <stdexcept>
#include <vector>

#include "mpm_amd/mpm.h"

using namespace mpm_amd;

static void hip(hipError_t e, const char *what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

int main() {
  float *d_x = nullptr, *d_v = nullptr;
  int32_t *d_id = nullptr;
  int rc = 1;
  try {
    MPM<3> sim;
    sim.initialize(Config().set("res", Vector3i(64, 64, 64)).set("base_delta_t", 1e-4).set("max_particles", 16384.0));
    mpmhip_shape s{};
    s.type = 1;
    s.p[0] = s.p[1] = s.p[2] = 0.5f;
    s.p[3] = 12.0f / 64;
    sim.add_particles_region(Config().set("type", "sand").set("ppc", 8.0).set("initial_velocity", Vector3(0.25f, -1.0f, 0.5f)), {s});
    sim.substep();
    sim.substep();  // (the sort has moved the slots: id order is no longer slot order)
    const int64_t n = sim.get_num_particles();
    const auto ref = sim.get_render_particles();
    hip(hipMalloc(reinterpret_cast<void **>(&d_x), sizeof(float) * 3 * n), "hipMalloc");
    hip(hipMalloc(reinterpret_cast<void **>(&d_v), sizeof(float) * 3 * n), "hipMalloc");
    hip(hipMalloc(reinterpret_cast<void **>(&d_id), sizeof(int32_t) * n), "hipMalloc");
    void *dst[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    dst[MPMHIP_F_X] = d_x; dst[MPMHIP_F_V] = d_v; dst[MPMHIP_F_ID] = d_id;
    if (sim.download_device(dst, n, true) != n) throw std::runtime_error("download_device: another row count than get_num_particles()");
    std::vector<float> x(3 * n), v(3 * n);
    std::vector<int32_t> id(n);
    hip(hipMemcpy(x.data(), d_x, sizeof(float) * 3 * n, hipMemcpyDeviceToHost), "hipMemcpy");
    hip(hipMemcpy(v.data(), d_v, sizeof(float) * 3 * n, hipMemcpyDeviceToHost), "hipMemcpy");
    hip(hipMemcpy(id.data(), d_id, sizeof(int32_t) * n, hipMemcpyDeviceToHost), "hipMemcpy");
    for (int64_t i = 0; i < n; i++) {
      if (id[i] != ref[i].id) throw std::runtime_error("download_device: ids differ from get_render_particles()");
      for (int k = 0; k < 3; k++)
        if (x[3 * i + k] != ref[i].position[k] || v[3 * i + k] != ref[i].velocity[k])
          throw std::runtime_error("download_device: x or v differ from get_render_particles()");
    }
    try {
      sim.download_device(dst, n - 1, true);
      throw std::logic_error("download_device: a short capacity was accepted");
    } catch (const std::runtime_error &) {  // (check() throws what mpmhip_last_error says)
    }
    for (auto &c : v) c *= 2.0f;
    hip(hipMemcpy(d_v, v.data(), sizeof(float) * 3 * n, hipMemcpyHostToDevice), "hipMemcpy");
    const void *src[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    src[MPMHIP_F_V] = d_v;
    sim.upload_device(src, n, true);
    const auto now = sim.get_render_particles();
    for (int64_t i = 0; i < n; i++)
      for (int k = 0; k < 3; k++)
        if (now[i].velocity[k] != v[3 * i + k] || now[i].position[k] != ref[i].position[k])
          throw std::runtime_error("upload_device: v was not doubled, or x moved");
    std::printf("ok %lld\n", (long long)n);
    rc = 0;
  } catch (const std::exception &e) {
    std::printf("error: %s\n", e.what());
  }
  (void)hipFree(d_x); (void)hipFree(d_v); (void)hipFree(d_id);
  return rc;
}
