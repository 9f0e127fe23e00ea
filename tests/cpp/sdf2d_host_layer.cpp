// MPM<2>::set_levelset_sdf and the delete_particles_inside_level_set action of the C++ host layer (include/mpm_amd/mpm2d.h) for
// tests/test_gpu_sdf2d.py: a sand square over a baked floor, a few substeps, a deletion inside a baked disc, two key frames — once
// through the C++ layer and once through the C ABI directly; the two runs (deterministic mode) must agree bit for bit.
// argv[1]: a file of fp32 words — origin[2], spacing, then two 65 x 65 fields (floor, disc; the last axis fastest).
// argv[2]: where the positions before the deletion are written (fp32 pairs, by creation id).
// stdout: particles before the deletion, deleted, particles after, 1 if the two runs agree.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mpm_amd/mpm2d.h"

using namespace mpm_amd;

namespace {
constexpr int N_SIDE = 65, LO = 22, HI = 38;

void must(int rc, mpmhip2d_ctx *m, const char *what) {
  if (rc < 0) throw std::runtime_error(std::string(what) + ": " + mpmhip2d_last_error(m));
}

struct Rows {
  std::vector<float> x, v, F, aux;
  std::vector<int32_t> id;
  bool operator==(const Rows &o) const {
    auto same = [](const std::vector<float> &a, const std::vector<float> &b) {
      return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
    };
    return same(x, o.x) && same(v, o.v) && same(F, o.F) && same(aux, o.aux) && id == o.id;
  }
};

Rows rows_of(const std::vector<Particle2D> &p) {
  Rows r;
  for (const Particle2D &q : p) {
    for (int k = 0; k < 2; k++) { r.x.push_back(q.position[k]); r.v.push_back(q.velocity[k]); }
    for (int k = 0; k < 4; k++) r.F.push_back(q.F[k]);
    r.aux.push_back(q.aux);
    r.id.push_back(q.id);
  }
  return r;
}
}  // namespace

int main(int argc, char **argv) {
  try {
    if (argc < 3) throw std::runtime_error("usage: sdf2d_host_layer <fields file> <positions out>");
    const size_t count = (size_t)N_SIDE * N_SIDE;
    std::vector<float> words(3 + 2 * count);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(words.data(), sizeof(float), words.size(), f) != words.size()) throw std::runtime_error("cannot read the fields");
    std::fclose(f);
    const std::vector<float> floor(words.begin() + 3, words.begin() + 3 + count), disc(words.begin() + 3 + count, words.end());
    const Vector2 origin(words[0], words[1]);
    const float spacing = words[2], friction = 0.4f;
    const Config sand = Config().set("type", "sand").set("square_lo", LO).set("square_hi", HI);

    // ---- through the C++ layer
    MPM<2> sim;
    // (the deterministic mode: the default path scatters with float atomics, whose order differs from run to run)
    sim.initialize(Config().set("res", "64,64").set("base_delta_t", 1e-4).set("max_particles", 8192.0).set("deterministic", true));
    sim.set_levelset_sdf(Vector2i(N_SIDE, N_SIDE), origin, spacing, floor, friction);
    sim.add_particles(sand);
    for (int i = 0; i < 5; i++) sim.substep();
    sim.set_levelset_sdf(Vector2i(N_SIDE, N_SIDE), origin, spacing, disc, friction);
    const Rows before = rows_of(sim.get_particles());
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(before.x.data(), sizeof(float), before.x.size(), f) != before.x.size()) throw std::runtime_error("cannot write the positions");
    std::fclose(f);
    const int64_t n0 = sim.get_num_particles();
    if (sim.general_action(Config().set("action", "delete_particles_inside_level_set")) != "") throw std::runtime_error("the action returns \"\"");
    const int64_t n1 = sim.get_num_particles();
    sim.set_levelset_sdf(Vector2i(N_SIDE, N_SIDE), origin, spacing, 0.0f, 1.0f, floor, disc, friction);  // two key frames
    for (int i = 0; i < 2; i++) sim.substep();
    const Rows a = rows_of(sim.get_particles());

    // ---- through the C ABI
    mpmhip2d_config c{};
    c.res[0] = c.res[1] = 64;
    c.dx = 1.0f / 64; c.dt = 1e-4f;
    c.gravity[1] = -10.0f;
    c.particle_gravity = 1; c.clean_boundary = 1;
    c.max_particles = 8192;
    c.deterministic = 1;
    mpmhip2d_ctx *m = nullptr;
    must(mpmhip2d_create(&c, &m), nullptr, "create");
    mpmhip2d_sdf_desc d;
    d.res[0] = d.res[1] = N_SIDE;
    d.origin[0] = origin[0]; d.origin[1] = origin[1];
    d.spacing = spacing;
    must(mpmhip2d_set_levelset_sdf(m, &d, floor.data(), nullptr, 0.0f, 1.0f, friction), m, "set_levelset_sdf");
    const float vol = c.dx * c.dx / 4.0f;
    const ParticleType t = create_particle_type("sand", sand, vol * 400.0f, vol);
    const int gid = mpmhip2d_add_group(m, t.material, t.params);
    must(gid, m, "add_group");
    std::vector<float> x, F, aux;
    for (int i = LO; i < HI; i++)
      for (int j = LO; j < HI; j++)
        for (int s = 0; s < 4; s++) {
          x.push_back((i + 0.5f + ((s & 1) ? 0.25f : -0.25f)) * c.dx);
          x.push_back((j + 0.5f + ((s & 2) ? 0.25f : -0.25f)) * c.dx);
          for (int k = 0; k < 4; k++) F.push_back(k % 3 == 0 ? t.initial_dg : 0.0f);
          aux.push_back(t.initial_aux);
        }
    const std::vector<float> v(x.size(), 0.0f);
    must(mpmhip2d_add_particles(m, gid, (int64_t)aux.size(), x.data(), v.data(), F.data(), nullptr, aux.data()), m, "add_particles");
    for (int i = 0; i < 5; i++) must(mpmhip2d_substep(m), m, "substep");
    must(mpmhip2d_set_levelset_sdf(m, &d, disc.data(), nullptr, 0.0f, 1.0f, friction), m, "set_levelset_sdf");
    int64_t deleted = -1;
    must(mpmhip2d_delete_particles_inside_level_set(m, &deleted), m, "delete_particles_inside_level_set");
    must(mpmhip2d_set_levelset_sdf(m, &d, floor.data(), disc.data(), 0.0f, 1.0f, friction), m, "set_levelset_sdf");
    for (int i = 0; i < 2; i++) must(mpmhip2d_substep(m), m, "substep");
    const int64_t n = mpmhip2d_num_particles(m);
    Rows b;
    b.x.resize(2 * n); b.v.resize(2 * n); b.F.resize(4 * n); b.aux.resize(n); b.id.resize(n);
    const int64_t got = mpmhip2d_download(m, n, b.x.data(), b.v.data(), b.F.data(), nullptr, b.aux.data(), nullptr, b.id.data());
    must((int)std::min<int64_t>(got, 0), m, "download");
    mpmhip2d_destroy(m);
    const bool same = got == n && a == b && n0 - deleted == n1;
    std::printf("%lld %lld %lld %d\n", (long long)n0, (long long)deleted, (long long)n1, same ? 1 : 0);
    if (!same)  // what differs, for the test's message
      std::printf("rows %lld / %lld, ids %d, x %d, v %d, F %d, aux %d\n", (long long)a.id.size(), (long long)got, a.id == b.id, a.x == b.x, a.v == b.v,
                  a.F == b.F, a.aux == b.aux);
  } catch (const std::exception &e) {
    std::printf("error: %s\n", e.what());
    return 1;
  }
  return 0;
}
