// taichi_mpm_amd/csrc/k_debug2d.h — the 2D device math exposed for parity tests (mpmhip2d_debug_force / _plasticity / _svd2):
// the inline functions of mpm2d_math.h that k_p2g, k_g2p and the deterministic mode call, one lane per row, no LDS.
// Part of libmpmhip (see k_mpm2d.h for the 2D substep; k_debug.h for the 3D twins).
#pragma once
#include "k_mpm2d.h"

namespace mpm2d {

// the rotation and the signed singular values exactly as the models consume them: U = [cu -su; su cu], S = signed_sigma
__global__ __launch_bounds__(256) void k2_debug_svd(int64_t n, const float *__restrict__ F, float *__restrict__ cu, float *__restrict__ su,
                                                    float *__restrict__ S) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const m2 f = {F[4 * i], F[4 * i + 1], F[4 * i + 2], F[4 * i + 3]};
    float c, s, lam[2], sg[2];
    eig_FFt(f, c, s, lam);
    signed_sigma(lam, det(f), sg);
    cu[i] = c; su[i] = s;
    S[2 * i] = sg[0]; S[2 * i + 1] = sg[1];
  }
}
__global__ __launch_bounds__(256) void k2_debug_force(GroupParams g, int64_t n, const float *__restrict__ F, const float *__restrict__ aux,
                                                      float *__restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const m2 f = {F[4 * i], F[4 * i + 1], F[4 * i + 2], F[4 * i + 3]};
    const m2 r = calculate_force(g, f, aux[i]);
    out[4 * i] = r.a; out[4 * i + 1] = r.b; out[4 * i + 2] = r.c; out[4 * i + 3] = r.d;
  }
}
// plasticity alone, or (force_out != nullptr) followed by calculate_force of the updated state: the order in which k_g2p and the
// next substep's k_p2g run them.  Water keeps its F (src/particles.cpp:469-478), as g2p_particle does.
__global__ __launch_bounds__(256) void k2_debug_plasticity(GroupParams g, int64_t n, const float *__restrict__ cdg, float *__restrict__ F,
                                                           float *__restrict__ aux, float *__restrict__ force_out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    m2 f = {F[4 * i], F[4 * i + 1], F[4 * i + 2], F[4 * i + 3]};
    const m2 c = {cdg[4 * i], cdg[4 * i + 1], cdg[4 * i + 2], cdg[4 * i + 3]};
    float a = aux[i];
    plasticity(g, c, f, a);
    if (g.type != MPMHIP_WATER) { F[4 * i] = f.a; F[4 * i + 1] = f.b; F[4 * i + 2] = f.c; F[4 * i + 3] = f.d; }
    aux[i] = a;
    if (force_out) {
      const m2 r = calculate_force(g, f, a);
      force_out[4 * i] = r.a; force_out[4 * i + 1] = r.b; force_out[4 * i + 2] = r.c; force_out[4 * i + 3] = r.d;
    }
  }
}

}  // namespace mpm2d
