// taichi_mpm_amd/csrc/k_sdf.h — sampled level set: particle collision behind G2P, and the sampler exposed for tests
// Part of libmpmhip (see mpmhip.hip for the substep overview and the data layout; the sampler itself is in mpm_math.h).
#pragma once
#include "mpm_common.h"

namespace mpm {

// particle_collision_resolution (src/mpm.cpp:414-426) against a sampled level set.  k_g2p / k_g2p_packed / k_g2p_rigid carry the push
// against analytic shapes inside their particle loop; a sampled set must not become a branch of those tuned kernels, so the ctx
// launches them with particle_collision = 0 and this kernel follows: one particle per lane over the sorted positions [0, n_sorted)
// of the records G2P just wrote.  It reads x (16 bytes) — and, only for a particle below the surface, v — pushes, and rewrites what
// the push changes: x in both records, v, the sort key (+ the creation id beside it in the deterministic mode), the block flag of
// the new position, and for a particle the push moves out of the admissible region n_dead and pid = -1, as k_g2p does it.
// (A particle G2P already deleted stays deleted: its key is INVALID before the push is looked at.)  No float atomics, no
// dependence on the order of the lanes: the deterministic mode stays bitwise.
__global__ __launch_bounds__(256) void k_sdf_collide(Params P, const Counters *__restrict__ cnt, float4 *__restrict__ rg,
                                                     float4 *__restrict__ rp, uint32_t *__restrict__ key,
                                                     uint8_t *__restrict__ blk_flag, Counters *cnt_w, SdfDev S) {
  const uint32_t n = min(cnt->n_sorted, P.n_slots);
  const uint32_t n_up = (n + 63u) & ~63u;  // whole waves: flag_block is a wave operation
  for (uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x; pos < n_up; pos += gridDim.x * blockDim.x) {
    uint32_t bkey = INVALID;
    if (pos < n) {
      const float4 g0 = rg[(size_t)pos * 4];
      const float x[3] = {g0.x, g0.y, g0.z};
      int c[3];
      float f[3];
      if (sdf_locate<3>(S, x, c, f)) {
        const float phi = sdf_phi<3>(S, P.t, P.idx, c, f);
        if (phi < 0.0f && key[pos] != INVALID) {
          float gr[3];
          sdf_normal<3>(S, P.t, c, f, gr);
          const float4 q0 = rp[(size_t)pos * 4], q1 = rp[(size_t)pos * 4 + 1];
          float v[3] = {q0.w, q1.x, q1.y};
          const float vn = gr[0] * v[0] + gr[1] * v[1] + gr[2] * v[2];
          const float nx[3] = {x[0] - gr[0] * phi * P.dx, x[1] - gr[1] * phi * P.dx, x[2] - gr[2] * phi * P.dx};
          v[0] -= vn * gr[0]; v[1] -= vn * gr[1]; v[2] -= vn * gr[2];
          const uint32_t kk = particle_key(P, nx, v, bkey);
          if (kk == INVALID) {
            float4 g3 = rg[(size_t)pos * 4 + 3];
            g3.z = __int_as_float(-1);
            rg[(size_t)pos * 4 + 3] = g3;
            atomicAdd(&cnt_w->n_dead, 1u);
            if (P.pidc) P.pidc[pos] = 0xFFFFFFFFu;
          }
          key[pos] = kk;
          rg[(size_t)pos * 4] = make_float4(nx[0], nx[1], nx[2], g0.w);
          rp[(size_t)pos * 4] = make_float4(nx[0], nx[1], nx[2], v[0]);
          rp[(size_t)pos * 4 + 1] = make_float4(v[1], v[2], q1.z, q1.w);
        }
      }
    }
    flag_block(blk_flag, bkey);
  }
}

// mpmhip_debug_levelset_sample: the device's level-set evaluation (sampled or analytic, whichever is installed) at given points
__global__ __launch_bounds__(256) void k_debug_levelset_sample(LevelSetDev LS, float t, float idx, int64_t n,
                                                               const float *__restrict__ pos, float *__restrict__ phi,
                                                               float *__restrict__ grad, float *__restrict__ dphidt,
                                                               int32_t *__restrict__ hit) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float x[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
    float ph = 0.0f, g[3] = {0, 0, 0}, dt = 0.0f;
    const bool h = levelset_eval_any(LS, t, x, idx, ph, g, &dt);
    hit[i] = h ? 1 : 0;
    phi[i] = h ? ph : 0.0f;
    dphidt[i] = h ? dt : 0.0f;
    grad[3 * i] = h ? g[0] : 0.0f; grad[3 * i + 1] = h ? g[1] : 0.0f; grad[3 * i + 2] = h ? g[2] : 0.0f;
  }
}

}  // namespace mpm
