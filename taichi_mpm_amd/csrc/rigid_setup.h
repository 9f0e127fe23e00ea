// taichi_mpm_amd/csrc/rigid_setup.h — what turns a mesh and a config into a CPIC rigid body, 3D (triangles) and 2D (segments): host
// only, no HIP header, no ctx.  Creation as MPM::add_rigid_particle (src/mpm_rigid_body.cpp:130-252), the poses of scripted bodies for
// one substep (advect_rigid_bodies, :255-286), an anchor's world position and velocity, the boundary particles' rows of a .bgeo frame.
// The callers (rigid_api.h, the 2D block of mpmhip.hip, the frame encoders) keep the device work: allocation, uploads, launches.
// Checked without a GPU by tests/test_rigid_setup_cpu.py (tests/cpp/rigid_setup_host.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>
#include "../../include/mpmhip.h"
#include "rigid_records.h"

namespace rigid_setup {
template <int D> struct Dim;
template <> struct Dim<3> { using Config = mpmhip_rigid_config; using Body = mpm::RigidBodyDev; using Sample = mpm::RigidSample; using Steps = mpm::RigidSteps; };
template <> struct Dim<2> { using Config = mpmhip2d_rigid_config; using Body = mpm2d::Rigid2; using Sample = mpm2d::Sample2; using Steps = mpm2d::Steps2; };
template <int D> constexpr int ELEM = D * D;            // floats per element: a triangle's 3 x 3, a segment's 2 x 2
template <int D> constexpr int ROT = D == 3 ? 3 : 1;    // angular components: Euler angles / one angle
template <int D> constexpr int INERTIA = ROT<D> * ROT<D>;
template <int D> using Tag = std::integral_constant<int, D>;  // picks the triangle / segment form of a function
template <class T> auto *ptr(T &a) { if constexpr (std::is_array_v<T>) return &a[0]; else return &a; }  // a 3D array or a 2D scalar field

// what the host keeps of every body (0 = the background) and of their boundary particles and elements
template <int D> struct HostBody {
  typename Dim<D>::Config cfg{};
  float mass = 0.0f, inertia[INERTIA<D>] = {};  // body frame, row-major
  int first_sample = 0, n_samples = 0;
  int64_t first_elem = 0, n_elems = 0;
};
template <int D> struct Store {
  std::vector<HostBody<D>> bodies;
  std::vector<typename Dim<D>::Sample> h_smp;
  std::vector<int32_t> h_smp_id;  // creation id of every boundary particle (they share the material particles' counter)
  std::vector<float> h_elems;     // mesh space (scaled, recentred), ELEM<D> floats each
};

inline void quat_from_euler_deg(const float deg[3], float q[4]) {  // X * Y * Z, src/mpm_rigid_body.cpp:108-114
  const float r = (float)(M_PI / 180.0);
  float ax[3][4];
  for (int k = 0; k < 3; k++) {
    const float a = deg[k] * r;
    ax[k][0] = std::cos(a / 2); ax[k][1] = ax[k][2] = ax[k][3] = 0.0f;
    ax[k][1 + k] = std::sin(a / 2);
  }
  auto mul = [](const float a[4], const float b[4], float o[4]) {
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  };
  float xy[4];
  mul(ax[0], ax[1], xy);
  mul(xy, ax[2], q);
}
inline void quat_to_matrix(const float q[4], float R[9]) {
  const float w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}
inline void rotation_of(const float e[3], float (&q)[4]) { quat_from_euler_deg(e, q); }  // angles in degrees as the records hold a
inline void rotation_of(const float e[3], float &angle) { angle = e[0] * (float)(M_PI / 180.0); }  // rotation: a quaternion / radians

// world position x[D] and (v != nullptr) velocity of the point at `off` in the body frame (align_with_rigid_body)
inline void anchor(const mpm::RigidBodyDev &B, const float off[3], float x[3], float *v = nullptr) {
  float ro[3];
  for (int r = 0; r < 3; r++) ro[r] = B.R[3 * r] * off[0] + B.R[3 * r + 1] * off[1] + B.R[3 * r + 2] * off[2];
  for (int r = 0; r < 3; r++) x[r] = ro[r] + B.pos[r];
  if (!v) return;
  v[0] = B.vel[0] + (B.omega[1] * ro[2] - B.omega[2] * ro[1]);
  v[1] = B.vel[1] + (B.omega[2] * ro[0] - B.omega[0] * ro[2]);
  v[2] = B.vel[2] + (B.omega[0] * ro[1] - B.omega[1] * ro[0]);
}
inline void anchor(const mpm2d::Rigid2 &B, const float off[2], float x[2], float *v = nullptr) {
  const float cs = std::cos(B.angle), sn = std::sin(B.angle);
  const float r0 = cs * off[0] - sn * off[1], r1 = sn * off[0] + cs * off[1];
  x[0] = r0 + B.pos[0]; x[1] = r1 + B.pos[1];
  if (v) { v[0] = B.vel[0] - B.omega * r1; v[1] = B.vel[1] + B.omega * r0; }
}
// the elements of body `id` in world space (get_mesh_to_world applied to mesh->elements: what write_rigid_body puts next to every
// frame, src/visualize.cpp:102-154), at most `cap` of them; returns the body's element count
template <int D> int64_t world_elements(const Store<D> &S, int id, const typename Dim<D>::Body &B, int64_t cap, float *out) {
  const HostBody<D> &H = S.bodies[id];
  if (out)
    for (int64_t q = 0; q < std::min<int64_t>(H.n_elems, cap) * D; q++) anchor(B, &S.h_elems[(size_t)(H.first_elem * D + q) * D], out + q * D);
  return H.n_elems;
}

// mass, centre of mass, inertia about it (body frame) and its inverse; nullptr or why the body is refused.
// 3D: a shell of surface density `density` (codimensional) or the enclosed solid of volume density `density` (signed tetrahedra
// against the origin; an inward-facing mesh has negative volume: flipped)
inline const char *mass_properties(Tag<3>, const std::vector<float> &tri, bool codimensional, double density, double &M, double com[3], double I[9], double invI[9]) {
  double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  M = 0; com[0] = com[1] = com[2] = 0;
  auto add = [&](double w, const double a[3], const double b[3]) {
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) S[r][c] += w * 0.5 * (a[r] * b[c] + b[r] * a[c]);
  };
  for (size_t e = 0; e < tri.size() / 9; e++) {
    double v[3][3];
    for (int q = 0; q < 3; q++) for (int k = 0; k < 3; k++) v[q][k] = tri[9 * e + 3 * q + k];
    const double s[3] = {v[0][0] + v[1][0] + v[2][0], v[0][1] + v[1][1] + v[2][1], v[0][2] + v[1][2] + v[2][2]};
    double m, cw, sw;
    if (codimensional) {
      const double a[3] = {v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2]}, b[3] = {v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2]};
      const double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
      m = 0.5 * std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) * density; cw = 1.0 / 3.0; sw = 1.0 / 12.0;
    } else {
      const double det = v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) - v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0]) +
                         v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
      m = det / 6.0 * density; cw = 0.25; sw = 1.0 / 20.0;
    }
    M += m;
    for (int k = 0; k < 3; k++) com[k] += m * cw * s[k];
    for (int q = 0; q < 3; q++) add(m * sw, v[q], v[q]);
    add(m * sw, s, s);
  }
  static const char *const refused = "rigid body: the mesh has no mass or a singular inertia tensor";
  if (!(std::abs(M) > 0)) return refused;
  for (int k = 0; k < 3; k++) com[k] /= M;
  const double flip = M < 0 ? -1.0 : 1.0;
  M *= flip;
  double Sc[3][3];
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Sc[r][c] = flip * S[r][c] - M * com[r] * com[c];
  const double tr = Sc[0][0] + Sc[1][1] + Sc[2][2];
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) I[3 * r + c] = (r == c ? tr : 0.0) - Sc[r][c];
  const double *a = I, det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
  if (det == 0) return refused;
  const double id = 1.0 / det;
  double *o = invI;
  o[0] = (a[4] * a[8] - a[5] * a[7]) * id; o[1] = (a[2] * a[7] - a[1] * a[8]) * id; o[2] = (a[1] * a[5] - a[2] * a[4]) * id;
  o[3] = (a[5] * a[6] - a[3] * a[8]) * id; o[4] = (a[0] * a[8] - a[2] * a[6]) * id; o[5] = (a[2] * a[3] - a[0] * a[5]) * id;
  o[6] = (a[3] * a[7] - a[4] * a[6]) * id; o[7] = (a[1] * a[6] - a[0] * a[7]) * id; o[8] = (a[0] * a[4] - a[1] * a[3]) * id;
  return nullptr;
}
// 2D: the segments as a shell of line density `density` (the rigid body the reference build is tested against,
// oracle/taichi_shim/.../rigid_body_shim.h, treats 2D bodies this way whether codimensional or not)
inline const char *mass_properties(Tag<2>, const std::vector<float> &seg, bool, double density, double &M, double com[2], double I[1], double invI[1]) {
  double S00 = 0, S11 = 0;
  M = 0; com[0] = com[1] = 0;
  for (size_t e = 0; e < seg.size() / 4; e++) {
    const double a[2] = {seg[4 * e], seg[4 * e + 1]}, b[2] = {seg[4 * e + 2], seg[4 * e + 3]};
    const double mm = std::sqrt((b[0] - a[0]) * (b[0] - a[0]) + (b[1] - a[1]) * (b[1] - a[1])) * density;
    M += mm;
    for (int k = 0; k < 2; k++) com[k] += mm * 0.5 * (a[k] + b[k]);
    S00 += mm / 6.0 * (a[0] * a[0] + b[0] * b[0] + (a[0] + b[0]) * (a[0] + b[0]));
    S11 += mm / 6.0 * (a[1] * a[1] + b[1] * b[1] + (a[1] + b[1]) * (a[1] + b[1]));
  }
  if (!(M > 0)) return "rigid body without mass";
  com[0] /= M; com[1] /= M;
  I[0] = (S00 - M * com[0] * com[0]) + (S11 - M * com[1] * com[1]);
  invI[0] = 1.0 / I[0];
  return nullptr;
}

// emit(offset, element) for every boundary particle of the mesh, in the reference's order (= the order of their creation ids).
// Triangles (src/mpm_rigid_body.cpp:214-235): a lattice along two edges, accumulated in float like the reference
template <class Emit> void sample_elements(Tag<3>, const std::vector<float> &tri, float dx, float, Emit emit) {
  for (size_t e = 0; e < tri.size() / 9; e++) {
    const float *v0 = &tri[9 * e], *v1 = v0 + 3, *v2 = v0 + 6;
    float a[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, b[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    const float xl = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), yl = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    if (!(xl > 0.0f) || !(yl > 0.0f)) continue;  // a degenerate triangle carries no boundary particles
    for (int k = 0; k < 3; k++) { a[k] /= xl; b[k] /= yl; }
    for (float _x = std::min(xl / 3.0f, dx / 2.0f); _x < xl + dx; _x += dx)
      for (float _y = std::min(yl / 3.0f, dx / 2.0f); _y < yl + dx; _y += dx) {
        const float x = (_x < xl) ? _x : _x - dx / 2.0f, y = (_y < yl) ? _y : _y - dx / 2.0f;
        if (x / xl + y / yl > 1.0f - 1e-6f) continue;
        const float off[3] = {v0[0] + a[0] * x + b[0] * y, v0[1] + a[1] * x + b[1] * y, v0[2] + a[2] * x + b[2] * y};
        emit(off, e);
      }
  }
}
// segments (:196-207): max(ceil(length / dx), 2) per segment, at the mid points of equal parts
template <class Emit> void sample_elements(Tag<2>, const std::vector<float> &seg, float, float idx, Emit emit) {
  for (size_t e = 0; e < seg.size() / 4; e++) {
    const float a[2] = {seg[4 * e], seg[4 * e + 1]}, b[2] = {seg[4 * e + 2], seg[4 * e + 3]};
    const float len = std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]));
    const int ns = std::max((int)std::ceil(len * idx), 2);
    for (int j = 0; j < ns; j++) {
      const float t = (0.5f + j) / ns;
      const float off[2] = {a[0] * (1.0f - t) + b[0] * t, a[1] * (1.0f - t) + b[1] * t};
      emit(off, e);
    }
  }
}

// One body from `cfg` and n_elems elements (mesh space, before `scale`), at time t on a grid of `res` cells of size dx = 1 / idx.
// Fills the device record Dv, appends the body, its elements and its boundary particles to S and sets ids_used to the creation ids
// the boundary particles took from next_pid on: every one takes an id from the same counter as the material particles
// (allocator.allocate_particle, src/particle_allocator.h:68-74), the ones near the domain wall too, which are then not created
// (near_boundary(*p), src/mpm_rigid_body.cpp:237-247).  Returns nullptr, or the reason for a refusal (S is then untouched).
template <int D> const char *add_body(const typename Dim<D>::Config &cfg, int64_t n_elems, const float *elems, float dx, float idx, const int32_t *res,
                                      float t, int32_t next_pid, Store<D> &S, typename Dim<D>::Body &Dv, int32_t &ids_used) {
  const bool spos = cfg.scripted_position != nullptr, srot = cfg.scripted_rotation != nullptr;
  if (!cfg.recenter && !(spos && srot))  // check_scripting_parameters (:15-56) as far as the struct can express it
    return D == 3 ? "recenter = 0 needs a scripted position and rotation (src/mpm_rigid_body.cpp:186-190)" : "recenter = 0 needs a scripted position and rotation";
  std::vector<float> el(elems, elems + ELEM<D> * n_elems);
  for (int64_t e = 0; e < n_elems; e++) {
    if (cfg.reverse_vertices) for (int k = 0; k < D; k++) std::swap(el[ELEM<D> * e + k], el[ELEM<D> * e + D + k]);
    for (int q = 0; q < D; q++) for (int k = 0; k < D; k++) el[ELEM<D> * e + D * q + k] *= cfg.scale[k] != 0 ? cfg.scale[k] : 1.0f;
  }
  const double density = cfg.density > 0 ? cfg.density : (cfg.codimensional ? 40.0 : 400.0);
  double M, com[D], I[INERTIA<D>], invI[INERTIA<D>];
  if (const char *why = mass_properties(Tag<D>(), el, cfg.codimensional != 0, density, M, com, I, invI)) return why;
  if (!cfg.recenter) for (int k = 0; k < D; k++) com[k] = 0.0;
  for (size_t i = 0; i < el.size(); i++) el[i] -= (float)com[i % D];  // (D floats per vertex)
  memset(&Dv, 0, sizeof Dv);  // the device record
  float p0[3] = {0, 0, 0}, euler[3] = {0, 0, 0};
  for (int k = 0; k < D; k++) p0[k] = cfg.initial_position[k];
  if (spos) cfg.scripted_position(cfg.position_user, t, p0);
  for (int k = 0; k < ROT<D>; k++) euler[k] = ptr(cfg.initial_rotation)[k];
  if (srot) cfg.scripted_rotation(cfg.rotation_user, t, euler);
  if constexpr (D == 3) { rotation_of(euler, Dv.q); quat_to_matrix(Dv.q, Dv.R); for (int k = 0; k < 3; k++) Dv.axis[k] = cfg.rotation_axis[k]; }
  else rotation_of(euler, Dv.angle);
  for (int k = 0; k < D; k++) { Dv.pos[k] = p0[k]; Dv.vel[k] = spos ? 0.0f : cfg.initial_velocity[k]; }
  for (int k = 0; k < ROT<D>; k++) ptr(Dv.omega)[k] = srot ? 0.0f : ptr(cfg.initial_angular_velocity)[k];
  Dv.mass = (float)M;
  Dv.inv_mass = spos ? 0.0f : (float)(1.0 / M);                                       // set_infinity_mass
  for (int k = 0; k < INERTIA<D>; k++) ptr(Dv.inv_I)[k] = srot ? 0.0f : (float)invI[k];  // set_infinity_inertia
  Dv.fric[0] = cfg.friction[0]; Dv.fric[1] = cfg.friction[1]; Dv.lin_damp = cfg.linear_damping; Dv.ang_damp = cfg.angular_damping;
  Dv.scripted = (spos ? 1 : 0) | (srot ? 2 : 0);
  HostBody<D> H;  // the host's record; then the boundary particles
  H.cfg = cfg; H.mass = (float)M;
  for (int k = 0; k < INERTIA<D>; k++) H.inertia[k] = (float)I[k];
  const int body = (int)S.bodies.size();
  H.first_sample = (int)S.h_smp.size(); H.first_elem = (int64_t)(S.h_elems.size() / ELEM<D>); H.n_elems = n_elems;
  int32_t allocated = 0;
  sample_elements(Tag<D>(), el, dx, idx, [&](const float *off, size_t e) {
    typename Dim<D>::Sample s;
    for (int k = 0; k < D; k++) s.off[k] = off[k];
    s.body = body; s.elem = (int)(H.first_elem + (int64_t)e);
    float w[D];
    bool near_wall = false;
    anchor(Dv, s.off, w);
    for (int r = 0; r < D; r++) { w[r] *= idx; near_wall = near_wall || w[r] < 7.0f || w[r] - (float)res[r] > -7.0f; }
    if (!near_wall) { S.h_smp.push_back(s); S.h_smp_id.push_back(next_pid + allocated); }
    allocated++;
  });
  ids_used = allocated; H.n_samples = (int)S.h_smp.size() - H.first_sample;
  S.h_elems.insert(S.h_elems.end(), el.begin(), el.end());
  S.bodies.push_back(H);
  return nullptr;
}

// advect_rigid_bodies(dt) at current_t = t: the scripts of every body evaluated at t and t + dt, for this one substep
template <int D> typename Dim<D>::Steps scripted_steps(const Store<D> &S, float t, float dt) {
  typename Dim<D>::Steps st;
  memset(&st, 0, sizeof st);
  for (size_t b = 1; b < S.bodies.size(); b++) {
    const auto &cfg = S.bodies[b].cfg;
    float p0[3] = {0, 0, 0}, p1[3] = {0, 0, 0}, e0[3] = {0, 0, 0}, e1[3] = {0, 0, 0};
    if (cfg.scripted_position) {
      st.s[b].has_pos = 1;
      cfg.scripted_position(cfg.position_user, t, p0);
      cfg.scripted_position(cfg.position_user, t + dt, p1);
      for (int k = 0; k < D; k++) { st.s[b].p0[k] = p0[k]; st.s[b].p1[k] = p1[k]; }
    }
    if (cfg.scripted_rotation) {
      st.s[b].has_rot = 1;
      cfg.scripted_rotation(cfg.rotation_user, t, e0);
      cfg.scripted_rotation(cfg.rotation_user, t + dt, e1);
      if constexpr (D == 3) { rotation_of(e0, st.s[b].q0); rotation_of(e1, st.s[b].q1); }
      else { rotation_of(e0, st.s[b].a0); rotation_of(e1, st.s[b].a1); }
    }
  }
  return st;
}

// the row of boundary particle `ir` in a frame (RigidBoundaryParticle, src/boundary_particle.h): position = anchor point (z = 0 in
// 2D), type = 1, index = creation id, v = body velocity at the anchor (align_with_rigid_body); every other field keeps MPMParticle's
// constructor value.  row_bytes = 48 (plain) or 92 (verbose); `bodies`: the device records, indexed by body.
template <int D> void bgeo_boundary_row(const Store<D> &S, const typename Dim<D>::Body *bodies, size_t ir, uint8_t *row, size_t row_bytes) {
  auto be32 = [](uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; };
  auto bef = [&](uint8_t *p, float f) { uint32_t u; std::memcpy(&u, &f, 4); be32(p, u); };
  float x[3] = {0, 0, 0}, v[3] = {0, 0, 0};
  anchor(bodies[S.h_smp[ir].body], S.h_smp[ir].off, x, v);
  std::memset(row, 0, row_bytes);
  bef(row, x[0]); bef(row + 4, x[1]); bef(row + 8, x[2]); bef(row + 12, 1.0f);
  be32(row + 16, 1u); be32(row + 20, (uint32_t)S.h_smp_id[ir]);
  be32(row + 24, 1u); be32(row + 28, 1u); be32(row + 32, 1u);
  bef(row + 36, v[0]); bef(row + 40, v[1]); bef(row + 44, v[2]);
}
// the rows of a frame in ascending creation id (write_partio sorts by id): nm material rows, whose ascending ids mat_id(im) gives and
// put_mat(im, row) writes, merged with the boundary particles' (bnd_id, ascending; put_bnd(ir, row)).
template <class MatId, class PutMat, class PutBnd> void merge_rows_by_id(uint8_t *row, size_t row_bytes, size_t nm, MatId mat_id, const std::vector<int32_t> &bnd_id, PutMat put_mat, PutBnd put_bnd) {
  for (size_t im = 0, ir = 0; im < nm || ir < bnd_id.size(); row += row_bytes) {
    if (ir < bnd_id.size() && (im >= nm || bnd_id[ir] < mat_id(im))) put_bnd(ir++, row);
    else put_mat(im++, row);
  }
}
}  // namespace rigid_setup
