// tests/cpp/rigid_setup_host.cpp — host build of the rigid-body set-up (taichi_mpm_amd/csrc/rigid_setup.h: creation, scripted steps,
// anchor kinematics, boundary rows of a frame) for tests/test_rigid_setup_cpu.py: the header alone, compiled by g++ into a small shared
// library, no HIP header, no GPU.  The same source is a program of its own: main() runs every scenario with fixed inputs, which
// is how the sampling loops run under AddressSanitizer and UBSan.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../taichi_mpm_amd/csrc/rigid_setup.h"

namespace rs = rigid_setup;

// what a ctx holds of its bodies: the store, the device records (here on the host) and the particles' id counter
template <int D> struct Scene {
  rs::Store<D> S;
  std::vector<typename rs::Dim<D>::Body> dev;
  int32_t next_pid = 0;
  std::string why;
  Scene() {
    S.bodies.emplace_back();  // the background
    dev.emplace_back();
    memset(&dev[0], 0, sizeof dev[0]);
  }
};
template <int D> static int add(Scene<D> *h, const typename rs::Dim<D>::Config *cfg, int64_t n, const float *elems, float dx, const int32_t *res, float t) {
  typename rs::Dim<D>::Body B;
  int32_t used = 0;
  const int body = (int)h->S.bodies.size();
  if (const char *why = rs::add_body<D>(*cfg, n, elems, dx, 1.0f / dx, res, t, h->next_pid, h->S, B, used)) { h->why = why; return -1; }
  h->next_pid += used;
  h->dev.push_back(B);
  return body;
}
// per boundary particle: offset D, world position D, world velocity D | body, element, creation id
template <int D> static int64_t samples(const Scene<D> *h, float *f, int32_t *i) {
  for (size_t s = 0; s < h->S.h_smp.size(); s++) {
    const auto &P = h->S.h_smp[s];
    if (f) {
      for (int k = 0; k < D; k++) f[3 * D * s + k] = P.off[k];
      rs::anchor(h->dev[P.body], P.off, f + 3 * D * s + D, f + 3 * D * s + 2 * D);
    }
    if (i) { i[3 * s] = P.body; i[3 * s + 1] = P.elem; i[3 * s + 2] = h->S.h_smp_id[s]; }
  }
  return (int64_t)h->S.h_smp.size();
}
// per body b >= 1: has_pos, has_rot, p0 D, p1 D, rotation at t, at t + dt (quaternion 4 / radians 1)
template <int D> static void steps(const Scene<D> *h, float t, float dt, float *out) {
  const auto st = rs::scripted_steps<D>(h->S, t, dt);
  constexpr int RW = D == 3 ? 4 : 1, W = 2 + 2 * D + 2 * RW;
  for (size_t b = 1; b < h->S.bodies.size(); b++) {
    float *o = out + W * (b - 1);
    const auto &s = st.s[b];
    o[0] = (float)s.has_pos; o[1] = (float)s.has_rot;
    for (int k = 0; k < D; k++) { o[2 + k] = s.p0[k]; o[2 + D + k] = s.p1[k]; }
    if constexpr (D == 3) { for (int k = 0; k < 4; k++) { o[8 + k] = s.q0[k]; o[12 + k] = s.q1[k]; } }
    else { o[6] = s.a0; o[7] = s.a1; }
  }
}
// every row of a frame whose material rows are `mat_ids` (ascending) and hold 0xAB bytes with the id's low byte in front
template <int D> static void frame_rows(const Scene<D> *h, int verbose, int64_t nm, const int32_t *mat_ids, uint8_t *out) {
  const size_t rb = verbose ? 92 : 48;
  rs::merge_rows_by_id(out, rb, (size_t)nm, [&](size_t im) { return mat_ids[im]; }, h->S.h_smp_id,
                       [&](size_t im, uint8_t *row) { memset(row, 0xAB, rb); row[0] = (uint8_t)mat_ids[im]; },
                       [&](size_t ir, uint8_t *row) { rs::bgeo_boundary_row<D>(h->S, h->dev.data(), ir, row, rb); });
}

extern "C" {
int rs_sizeof(int what) {
  const size_t s[] = {sizeof(mpmhip_rigid_config), sizeof(mpmhip2d_rigid_config), sizeof(mpm::RigidBodyDev), sizeof(mpm2d::Rigid2)};
  return (int)s[what];
}
void *rs3_new() { return new Scene<3>; }
void *rs2_new() { return new Scene<2>; }
void rs3_free(void *h) { delete (Scene<3> *)h; }
void rs2_free(void *h) { delete (Scene<2> *)h; }
int rs3_add(void *h, const mpmhip_rigid_config *c, int64_t n, const float *e, float dx, const int32_t *res, float t) { return add((Scene<3> *)h, c, n, e, dx, res, t); }
int rs2_add(void *h, const mpmhip2d_rigid_config *c, int64_t n, const float *e, float dx, const int32_t *res, float t) { return add((Scene<2> *)h, c, n, e, dx, res, t); }
const char *rs3_why(void *h) { return ((Scene<3> *)h)->why.c_str(); }
const char *rs2_why(void *h) { return ((Scene<2> *)h)->why.c_str(); }
int32_t rs3_next_pid(void *h, int32_t add) { return ((Scene<3> *)h)->next_pid += add; }  // (add > 0: material particles take ids)
int32_t rs2_next_pid(void *h, int32_t add) { return ((Scene<2> *)h)->next_pid += add; }
int64_t rs3_samples(void *h, float *f, int32_t *i) { return samples((Scene<3> *)h, f, i); }
int64_t rs2_samples(void *h, float *f, int32_t *i) { return samples((Scene<2> *)h, f, i); }
// the layouts of mpmhip_rigid_get_state (33 floats) and mpmhip2d_rigid_get_state (10)
void rs3_state(void *h, int id, float *out) {
  const auto &D = ((Scene<3> *)h)->dev[id];
  int k = 0;
  for (int i = 0; i < 3; i++) out[k++] = D.pos[i];
  for (int i = 0; i < 4; i++) out[k++] = D.q[i];
  for (int i = 0; i < 3; i++) out[k++] = D.vel[i];
  for (int i = 0; i < 3; i++) out[k++] = D.omega[i];
  out[k++] = D.mass; out[k++] = D.inv_mass;
  for (int i = 0; i < 9; i++) out[k++] = ((Scene<3> *)h)->S.bodies[id].inertia[i];
  for (int i = 0; i < 9; i++) out[k++] = D.inv_I[i];
}
void rs2_state(void *h, int id, float *out) {
  const auto &D = ((Scene<2> *)h)->dev[id];
  out[0] = D.pos[0]; out[1] = D.pos[1]; out[2] = D.angle; out[3] = D.vel[0]; out[4] = D.vel[1]; out[5] = D.omega;
  out[6] = D.mass; out[7] = D.inv_mass; out[8] = ((Scene<2> *)h)->S.bodies[id].inertia[0]; out[9] = D.inv_I;
}
// the rest of the device record: R 9, fric 2, damping 2, axis 3, scripted / fric 2, damping 2, scripted
void rs3_record(void *h, int id, float *out) {
  const auto &D = ((Scene<3> *)h)->dev[id];
  for (int i = 0; i < 9; i++) out[i] = D.R[i];
  out[9] = D.fric[0]; out[10] = D.fric[1]; out[11] = D.lin_damp; out[12] = D.ang_damp;
  for (int i = 0; i < 3; i++) out[13 + i] = D.axis[i];
  out[16] = (float)D.scripted;
}
void rs2_record(void *h, int id, float *out) {
  const auto &D = ((Scene<2> *)h)->dev[id];
  out[0] = D.fric[0]; out[1] = D.fric[1]; out[2] = D.lin_damp; out[3] = D.ang_damp; out[4] = (float)D.scripted;
}
void rs3_set_motion(void *h, int id, const float *v, const float *w) { auto &D = ((Scene<3> *)h)->dev[id]; for (int k = 0; k < 3; k++) { D.vel[k] = v[k]; D.omega[k] = w[k]; } }
void rs2_set_motion(void *h, int id, const float *v, const float *w) { auto &D = ((Scene<2> *)h)->dev[id]; D.vel[0] = v[0]; D.vel[1] = v[1]; D.omega = w[0]; }
int64_t rs3_mesh(void *h, int id, int64_t cap, float *out) { auto *s = (Scene<3> *)h; return rs::world_elements<3>(s->S, id, s->dev[id], cap, out); }
int64_t rs2_mesh(void *h, int id, int64_t cap, float *out) { auto *s = (Scene<2> *)h; return rs::world_elements<2>(s->S, id, s->dev[id], cap, out); }
void rs3_steps(void *h, float t, float dt, float *out) { steps((Scene<3> *)h, t, dt, out); }
void rs2_steps(void *h, float t, float dt, float *out) { steps((Scene<2> *)h, t, dt, out); }
void rs3_frame_rows(void *h, int verbose, int64_t nm, const int32_t *ids, uint8_t *out) { frame_rows((Scene<3> *)h, verbose, nm, ids, out); }
void rs2_frame_rows(void *h, int verbose, int64_t nm, const int32_t *ids, uint8_t *out) { frame_rows((Scene<2> *)h, verbose, nm, ids, out); }
}

// ---------------------------------------------------------------------------------------------- the stand-alone program
#define CHECK(x) do { if (!(x)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #x); return __LINE__; } } while (0)
static void script_pos(void *u, float t, float out[3]) { const float *p = (const float *)u; for (int k = 0; k < 3; k++) out[k] = p[k] + 0.25f * t; }
static void script_rot(void *u, float t, float out[3]) { const float *p = (const float *)u; for (int k = 0; k < 3; k++) out[k] = p[3 + k] + 90.0f * t; }
static std::vector<float> box(float hx, float hy, float hz, bool inward) {
  float c[8][3];
  for (int i = 0; i < 8; i++) { c[i][0] = i & 4 ? hx : -hx; c[i][1] = i & 2 ? hy : -hy; c[i][2] = i & 1 ? hz : -hz; }
  const int q[6][4] = {{0, 1, 3, 2}, {4, 6, 7, 5}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 2, 6, 4}, {1, 5, 7, 3}};
  std::vector<float> t;
  for (int pass = 0; pass < 2; pass++)
    for (const auto &f : q) {
      const int v[3] = {f[0], pass ? f[2] : f[1], pass ? f[3] : f[2]};
      for (int k = 0; k < 3; k++) t.insert(t.end(), c[v[inward ? 2 - k : k]], c[v[inward ? 2 - k : k]] + 3);
    }
  return t;
}
template <int D> static int frames(Scene<D> &s) {  // plain and verbose, the bodies between two particle groups / first / alone
  const int64_t nb = samples<D>(&s, nullptr, nullptr);
  const int32_t lo[3] = {0, 1, 2}, hi[2] = {s.next_pid, s.next_pid + 1}, both[5] = {0, 1, 2, s.next_pid, s.next_pid + 1};
  for (int verbose = 0; verbose < 2; verbose++) {
    std::vector<uint8_t> rows((size_t)(nb + 5) * (verbose ? 92 : 48));  // (exactly the frame's rows: a row too many is a heap overflow)
    frame_rows<D>(&s, verbose, 5, both, rows.data());
    rows.resize((size_t)(nb + 3) * (verbose ? 92 : 48)); rows.shrink_to_fit();
    frame_rows<D>(&s, verbose, 3, lo, rows.data());
    rows.resize((size_t)(nb + 2) * (verbose ? 92 : 48)); rows.shrink_to_fit();
    frame_rows<D>(&s, verbose, 2, hi, rows.data());
    rows.resize((size_t)nb * (verbose ? 92 : 48)); rows.shrink_to_fit();
    frame_rows<D>(&s, verbose, 0, nullptr, rows.data());
  }
  return 0;
}
static int scenarios3() {
  const float dx = 1.0f / 32;
  const int32_t res[3] = {32, 32, 32};
  float script[6] = {0.5f, 0.55f, 0.5f, 10.0f, 0.0f, 5.0f};
  Scene<3> s;
  s.next_pid = 3;  // (a particle group before the bodies)
  mpmhip_rigid_config c{};
  c.codimensional = 1; c.recenter = 1; c.density = 40.0f;
  c.initial_position[0] = c.initial_position[1] = c.initial_position[2] = 0.5f;
  c.initial_rotation[0] = 20.0f; c.initial_rotation[2] = 10.0f;
  // edges shorter than dx / 2, just under and just over a multiple of dx; a triangle without area between two good ones
  const float h = 0.2f, e0 = 0.4f * dx, e1 = 3.0f * dx - 1e-6f, e2 = 3.0f * dx + 1e-6f;
  const std::vector<float> tris = {0, 0, 0, e0, 0, 0, 0, 0, e0,      0.1f, 0, 0.1f, 0.1f, 0, 0.1f, 0.2f, 0, 0.2f,   0, 0, 0, e1, 0, 0, 0, 0, e2,
                                   -h, 0, -h, h, 0, -h, h, 0, h};
  CHECK(add<3>(&s, &c, 4, tris.data(), dx, res, 0.0f) == 1);
  CHECK(s.S.bodies[1].n_samples > 0 && s.S.h_smp_id.front() == 3 && s.next_pid >= 3 + s.S.bodies[1].n_samples);
  for (const auto &p : s.S.h_smp) CHECK(p.elem != 1);
  // a solid box, outward and inward; scaled with a zero component; reversed; near the wall
  for (int inward = 0; inward < 2; inward++) {
    mpmhip_rigid_config b = c;
    b.codimensional = 0; b.density = 400.0f; b.reverse_vertices = inward; b.scale[0] = 0.0f; b.scale[1] = 0.5f; b.scale[2] = 2.0f;
    b.initial_position[0] = inward ? 0.2f : 0.5f;
    const std::vector<float> t = box(0.1f, 0.06f, 0.12f, inward != 0);
    const int32_t before = s.next_pid;
    const size_t kept = s.S.h_smp.size();
    CHECK(add<3>(&s, &b, (int64_t)t.size() / 9, t.data(), dx, res, 0.0f) == 2 + inward);
    CHECK(s.dev.back().mass > 0.0f && s.next_pid - before >= (int32_t)(s.S.h_smp.size() - kept));
  }
  // scripted, recenter = 0; the refusals
  mpmhip_rigid_config sc = c;
  sc.recenter = 0; sc.scripted_position = script_pos; sc.position_user = script; sc.scripted_rotation = script_rot; sc.rotation_user = script;
  CHECK(add<3>(&s, &sc, 1, tris.data() + 27, dx, res, 0.125f) == 4);
  CHECK(s.dev[4].scripted == 3 && s.dev[4].inv_mass == 0.0f && s.dev[4].pos[0] == 0.5f + 0.25f * 0.125f);
  sc.scripted_rotation = nullptr;
  CHECK(add<3>(&s, &sc, 1, tris.data() + 27, dx, res, 0.0f) == -1 && s.why.find("recenter = 0 needs") == 0);
  CHECK(add<3>(&s, &c, 1, tris.data() + 9, dx, res, 0.0f) == -1 && s.why.find("no mass") != std::string::npos);
  CHECK(s.S.bodies.size() == 5 && s.dev.size() == 5);
  const auto st = rs::scripted_steps<3>(s.S, 0.5f, 0.25f);
  CHECK(st.s[4].has_pos == 1 && st.s[4].has_rot == 1 && st.s[1].has_pos == 0 && st.s[4].p1[1] == 0.55f + 0.25f * 0.75f);
  std::vector<float> mesh(9 * 12);
  CHECK(rs::world_elements<3>(s.S, 2, s.dev[2], 12, mesh.data()) == 12 && rs::world_elements<3>(s.S, 1, s.dev[1], 0, nullptr) == 4);
  return frames(s);
}
static int scenarios2() {
  const float dx = 1.0f / 64;
  const int32_t res[2] = {64, 64};
  float script[6] = {0.5f, 0.55f, 0.0f, 10.0f, 0.0f, 0.0f};
  Scene<2> s;
  s.next_pid = 3;
  mpmhip2d_rigid_config c{};
  c.codimensional = 1; c.recenter = 1; c.density = 40.0f; c.initial_position[0] = c.initial_position[1] = 0.5f; c.initial_rotation = 20.0f;
  const std::vector<float> segs = {-0.15f, 0, 0.15f, 0,   0.15f, 0, 0.15f + 0.3f * dx, 0,   0.2f, 0.1f, 0.2f, 0.1f};  // long, shorter than dx, a point
  CHECK(add<2>(&s, &c, 3, segs.data(), dx, res, 0.0f) == 1);
  CHECK(s.S.h_smp.size() == 20 + 2 + 2 && s.next_pid == 3 + 24);
  mpmhip2d_rigid_config w = c;
  w.initial_position[0] = 0.15f; w.reverse_vertices = 1; w.scale[0] = 0.0f; w.scale[1] = 3.0f;
  CHECK(add<2>(&s, &w, 1, segs.data(), dx, res, 0.0f) == 2 && s.S.bodies[2].n_samples < 20 && s.next_pid == 3 + 24 + 20);
  mpmhip2d_rigid_config sc = c;
  sc.recenter = 0; sc.scripted_position = script_pos; sc.position_user = script; sc.scripted_rotation = script_rot; sc.rotation_user = script;
  CHECK(add<2>(&s, &sc, 1, segs.data(), dx, res, 0.125f) == 3 && s.dev[3].scripted == 3 && s.dev[3].inv_I == 0.0f);
  sc.scripted_position = nullptr;
  CHECK(add<2>(&s, &sc, 1, segs.data(), dx, res, 0.0f) == -1 && s.why == "recenter = 0 needs a scripted position and rotation");
  CHECK(add<2>(&s, &c, 1, segs.data() + 8, dx, res, 0.0f) == -1 && s.why == "rigid body without mass");
  const auto st = rs::scripted_steps<2>(s.S, 0.5f, 0.25f);
  CHECK(st.s[3].has_pos == 1 && st.s[3].has_rot == 1 && st.s[3].a0 == (10.0f + 90.0f * 0.5f) * (float)(M_PI / 180.0));
  std::vector<float> mesh(4 * 3);
  CHECK(rs::world_elements<2>(s.S, 1, s.dev[1], 3, mesh.data()) == 3);
  return frames(s);
}
int main() {
  if (int line = scenarios3()) return line > 255 ? 1 : line;
  if (int line = scenarios2()) return line > 255 ? 1 : line;
  std::printf("rigid_setup: scenarios ok\n");
  return 0;
}
