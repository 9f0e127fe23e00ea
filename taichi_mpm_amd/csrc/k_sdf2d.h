// taichi_mpm_amd/csrc/k_sdf2d.h — MPM<2> against a sampled level set (mpmhip2d_set_levelset_sdf; rules: include/mpmhip.h; the sampler:
// mpm_math.h, the sdf_* templates at D = 2).  Part of libmpmhip.  A ctx without a sampled set launches none of these kernels except k2_delete_inside: its
// substep is k_mpm2d.h's, unchanged.  With one installed:
//   k_grid_sdf        k_grid's node update with the boundary condition read from the lattice
//   k2_sdf_collide    particle_collision behind G2P.  g2p_particle pushes against shapes inside its particle loop (LS.n > 0); a sampled
//                     set has LS.n == 0, so both of its users (k_g2p, k2d_g2p) skip that, and this pass follows: one lane per slot,
//                     live particles only — those alive_pos kept — with the expressions of the inline push.  8 bytes read per
//                     particle, v only below the surface.  No atomics, no dependence on the order of lanes: the deterministic mode
//                     stays bitwise.
//   k2_delete_inside  general_action "delete_particles_inside_level_set" for shapes or a sampled set
//   k2_debug_levelset_sample   the device's evaluation at host-given points (tests)
#pragma once
#include "k_mpm2d.h"

namespace mpm2d {

// whichever level set is installed, read in the plane
__device__ __forceinline__ bool levelset_eval_any2(const LevelSetDev &LS, float t, const float x[2], float idx, float &phi, float n[2],
                                                   float *dphidt = nullptr) {
  if (LS.sdf.phi0) return mpm::sdf_eval<2>(LS.sdf, t, x, idx, phi, n, dphidt);
  const float xw[3] = {x[0], x[1], 0.0f};
  float g[3] = {0.0f, 0.0f, 0.0f};
  const bool hit = mpm::levelset_eval(LS, t, xw, idx, phi, g, dphidt);
  n[0] = g[0]; n[1] = g[1];
  return hit;
}

// k_grid (k_mpm2d.h) with the boundary condition read from the lattice.  The node update is restated here, not shared through a
// device function: moving k_grid's body into one changed k_grid's register allocation (profiles/kernel_diff.py), and a ctx without
// a sampled set must launch the code it always did.
__global__ __launch_bounds__(256) void k_grid_sdf(Params P, LevelSetDev LS, float *__restrict__ grid) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int ny = P.res[1] + 1;
  if (t >= (P.res[0] + 1) * ny) return;
  float *g = grid + 3 * (size_t)t;
  const float m = g[2];
  float v[2] = {g[0], g[1]};
  if (m > 0.0f) {
    const float im = 1.0f / m;
    v[0] = v[0] * im + (P.particle_gravity ? 0.0f : P.g[0] * P.dt);
    v[1] = v[1] * im + (P.particle_gravity ? 0.0f : P.g[1] * P.dt);
  }
  if (m != 0.0f) {
    const float xn[2] = {(float)(t / ny) * P.dx, (float)(t % ny) * P.dx};
    float phi, dphidt, nrm[2];
    if (mpm::sdf_eval<2>(LS.sdf, P.t, xn, P.idx, phi, nrm, &dphidt) && !(phi < -3.0f || 0.0f < phi)) {
      const float vb[2] = {-dphidt * nrm[0] * P.dx, -dphidt * nrm[1] * P.dx};
      friction_project2(v, vb, nrm, LS.friction);
    }
  }
  if (P.dirichlet) {  // src/mpm.cpp:389-397, behind the boundary condition
    const float px = (float)(t / ny) * P.dx;
    if (px < P.dl) { v[0] = P.vl; v[1] = 0.0f; }
    else if (px > 1.0f - P.dr) { v[0] = P.vr; v[1] = 0.0f; }
  }
  g[0] = v[0]; g[1] = v[1];
}

// particle_collision_resolution (src/mpm.cpp:414-426) against the sampled set
__global__ __launch_bounds__(256) void k2_sdf_collide(Params P, mpm::SdfDev S, int64_t n, float *__restrict__ x, float *__restrict__ v,
                                                      const int32_t *__restrict__ pid) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || pid[p] < 0) return;
  const float xx[2] = {x[2 * p], x[2 * p + 1]};
  int c[2];
  float f[2];
  if (!mpm::sdf_locate<2>(S, xx, c, f)) return;
  const float phi = mpm::sdf_phi<2>(S, P.t, P.idx, c, f);
  if (!(phi < 0.0f)) return;
  float gr[2];
  mpm::sdf_normal<2>(S, P.t, c, f, gr);
  const float nv[2] = {v[2 * p], v[2 * p + 1]};
  const float vn = gr[0] * nv[0] + gr[1] * nv[1];
  x[2 * p] = xx[0] - gr[0] * phi * P.dx; x[2 * p + 1] = xx[1] - gr[1] * phi * P.dx;
  v[2 * p] = nv[0] - vn * gr[0]; v[2 * p + 1] = nv[1] - vn * gr[1];
}

// every live particle whose level-set value at its position is negative is deleted for good, the way g2p_particle marks one
__global__ __launch_bounds__(256) void k2_delete_inside(Params P, LevelSetDev LS, int64_t n, const float *__restrict__ x,
                                                        int32_t *__restrict__ pid, unsigned int *__restrict__ n_dead) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || pid[p] < 0) return;
  const float xx[2] = {x[2 * p], x[2 * p + 1]};
  float phi, nrm[2];
  if (levelset_eval_any2(LS, P.t, xx, P.idx, phi, nrm) && phi < 0.0f) {
    pid[p] = -1;
    atomicAdd(n_dead, 1u);
  }
}

// out: phi [n], grad [2 n], dphidt [n], hit [n]
__global__ __launch_bounds__(256) void k2_debug_levelset_sample(LevelSetDev LS, float t, float idx, int64_t n, const float *__restrict__ pos,
                                                                float *__restrict__ phi, float *__restrict__ grad,
                                                                float *__restrict__ dphidt, int32_t *__restrict__ hit) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x[2] = {pos[2 * i], pos[2 * i + 1]};
  float ph = 0.0f, g[2] = {0.0f, 0.0f}, dt = 0.0f;
  const bool h = levelset_eval_any2(LS, t, x, idx, ph, g, &dt);
  hit[i] = h ? 1 : 0;
  phi[i] = h ? ph : 0.0f;
  dphidt[i] = h ? dt : 0.0f;
  grad[2 * i] = h ? g[0] : 0.0f; grad[2 * i + 1] = h ? g[1] : 0.0f;
}

}  // namespace mpm2d
