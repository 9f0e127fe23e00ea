// tests/cpp/rigid_collide_host.cpp — host build of the rigid-rigid collision arithmetic the device runs
// (taichi_mpm_amd/csrc/k_rigid_collide.h), as a small shared library for tests/test_rigid_collide_cpu.py and
// tests/test_gpu_rigid_collide.py: the same header, compiled by g++ with -ffp-contract=off, checked against libccd's own
// single-precision results (tests/golden/rigid_mpr.npz) without a GPU, and the yardstick the device is held to bit for bit.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../taichi_mpm_amd/csrc/k_rigid_collide.h"

using namespace mpm;

extern "C" {
int rc_sizeof_body() { return (int)sizeof(JointBody); }
int rc_sizeof_collision() { return (int)sizeof(RigidCollision); }
int rc_sizeof_impulse() { return (int)sizeof(RigidImpulse); }
void rc_loop_bounds(int *out) { out[0] = MPR_MAX_DISCOVER; out[1] = MPR_MAX_REFINE; out[2] = MPR_MAX_PENETR; }
int rc_pair_index(int i, int j) { return rigid_pair_index(i, j); }

// detection on raw vertex clouds, the twin of mpmhip_rigid_mpr_test: pair q is cloud 2q against cloud 2q + 1; cloud c has the
// vertices [offsets[c], offsets[c + 1]) of verts, the rotation rot[9 c] (null: none) and the centre ctr[3 c].
// out: 9 floats per pair — hit, depth, dir[3], pos[3], support calls.  Returns the number of pairs whose loop bound expired.
int rc_mpr(int n_pairs, const float *verts, const int64_t *offsets, const float *rot, const float *ctr, float *out) {
  const int64_t nv = offsets[2 * n_pairs];
  std::vector<float> r((size_t)nv * 3), p((size_t)nv * 3);
  for (int c = 0; c < 2 * n_pairs; c++)
    for (int64_t v = offsets[c]; v < offsets[c + 1]; v++) {
      if (rot) hull_vertex(rot + 9 * c, ctr + 3 * c, verts + 3 * v, &r[3 * v], &p[3 * v]);
      else for (int k = 0; k < 3; k++) { r[3 * v + k] = verts[3 * v + k]; p[3 * v + k] = r[3 * v + k] + ctr[3 * c + k]; }
    }
  int expired = 0;
  for (int q = 0; q < n_pairs; q++) {
    const int a = 2 * q, b = 2 * q + 1;
    HostSupport sup;
    sup.A = HullView{&r[3 * offsets[a]], &p[3 * offsets[a]], (int)(offsets[a + 1] - offsets[a])};
    sup.B = HullView{&r[3 * offsets[b]], &p[3 * offsets[b]], (int)(offsets[b + 1] - offsets[b])};
    MprResult res;
    mpr_penetration(sup, ctr + 3 * a, ctr + 3 * b, res);
    float *o = out + 9 * q;
    o[0] = (float)res.hit; o[1] = res.depth;
    for (int k = 0; k < 3; k++) { o[2 + k] = res.dir[k]; o[5 + k] = res.pos[k]; }
    o[8] = (float)res.calls;
    expired += res.expired;
  }
  return expired;
}

// resolution alone: bodies[nb] (body 0 = background) in place, fric / rest per body, cols[nc] the collision list.
// log (may be null): one RigidImpulse per projection.  Returns the number of projections.
int rc_resolve(int nb, JointBody *bodies, const float *fric, const float *rest, int nc, const RigidCollision *cols, int iterations,
               int position_iterations, float penalty, float dt, RigidImpulse *log) {
  RigidContactParams cp;
  std::memset(&cp, 0, sizeof cp);
  for (int b = 0; b < nb && b < MAX_COLLIDE_BODIES; b++) { cp.fric[b] = fric[b]; cp.rest[b] = rest[b]; }
  const RigidSolveConfig cfg{iterations, position_iterations, penalty, dt};
  return rigidify_resolve(bodies, nb, cp, cols, nc, cfg, log);
}

// MPM::rigidify whole: hull[b] = the body-frame vertices [hull_off[b], hull_off[b + 1]) of body b (none for body 0),
// scripted[b] = 3 for a body that follows a script in position and rotation.  cols_out[rigid_pair_count(nb)]: the collision list
// in (i, j) order; returns its length.  bodies: vel / omega updated in place.
int rc_rigidify(int nb, JointBody *bodies, const int *scripted, const float *hull, const int64_t *hull_off, const float *fric,
                const float *rest, int iterations, int position_iterations, float penalty, float dt, RigidCollision *cols_out) {
  const int64_t nv = hull_off[nb];
  std::vector<float> r((size_t)nv * 3), p((size_t)nv * 3);
  for (int b = 1; b < nb; b++)
    for (int64_t v = hull_off[b]; v < hull_off[b + 1]; v++) hull_vertex(bodies[b].R, bodies[b].pos, hull + 3 * v, &r[3 * v], &p[3 * v]);
  int n = 0;
  for (int i = 2; i < nb; i++)
    for (int j = 1; j < i; j++) {
      if (scripted[i] == 3 && scripted[j] == 3) continue;
      if (hull_off[i + 1] == hull_off[i] || hull_off[j + 1] == hull_off[j]) continue;
      HostSupport sup;
      sup.A = HullView{&r[3 * hull_off[i]], &p[3 * hull_off[i]], (int)(hull_off[i + 1] - hull_off[i])};
      sup.B = HullView{&r[3 * hull_off[j]], &p[3 * hull_off[j]], (int)(hull_off[j + 1] - hull_off[j])};
      MprResult res;
      mpr_penetration(sup, bodies[i].pos, bodies[j].pos, res);
      if (!res.hit) continue;
      RigidCollision C;
      C.hit = 1; C.i = i; C.j = j; C.calls = res.calls; C.depth = res.depth;
      for (int k = 0; k < 3; k++) { C.dir[k] = res.dir[k]; C.pos[k] = res.pos[k]; }
      cols_out[n++] = C;
    }
  rc_resolve(nb, bodies, fric, rest, n, cols_out, iterations, position_iterations, penalty, dt, nullptr);
  return n;
}
}
