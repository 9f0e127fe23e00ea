// taichi_mpm_amd/csrc/k_region.h — region expressions on the device (rules: include/mpmhip.h, "Region expressions"; checks:
// region_program.h; host side: region_api.h).  RegionExpr<D> is a postfix program over at most 8 leaves, evaluated per point; it is
// the `Region` of k_seed_bounds / k_seed_count (k_seed.h) and what the two kernels below sample.  A leaf's distance comes from the
// evaluators the plain regions use — levelset_eval_key with one shape, sdf_locate / sdf_phi_frame for a sampled field (mpm_math.h) —
// so an expression of one plain leaf decides as SeedRegion does.  The whole description travels by value in the kernel arguments
// (1 384 bytes): the program is wave-uniform, the loop over it branches uniformly, leaves and fields are read with scalar loads, and the
// four stack slots are named registers, never an indexed private array.
#pragma once
#include <hip/hip_runtime.h>

#include "mpm_common.h"

namespace mpm {

// no multiply-add of a placement may be fused: tests/region_model.py restates it to the bit
#define REGION_NO_CONTRACT _Pragma("clang fp contract(off)")

constexpr int REGION_WG = 256;

struct RegionLeafDev {
  int kind, field, placed, banded;
  ShapeDev shape;  // kind 0 (D = 2: prepared for the plane by the host, as Seed2::shapes prepares them)
  float rot[9];    // row-major R (D = 2: the upper-left 2 x 2)
  float scale, inv_scale;
  float t[3], p[3];
  float lo, hi;
};

template <int D>
struct RegionExpr {
  int n_ops;
  int ops[MPMHIP_REGION_MAX_OPS];  // opcode | leaf << 2
  RegionLeafDev leaf[MPMHIP_REGION_MAX_LEAVES];
  SdfDev field[MPMHIP_REGION_MAX_FIELDS];

  // phi of leaf L in its own space, grid units; +inf outside a sampled leaf's lattice
  __device__ __forceinline__ float leaf_own(const RegionLeafDev &L, const float x[D], float idx) const {
    REGION_NO_CONTRACT
    if (L.kind) {
      const SdfDev &S = field[L.field];
      int c[D];
      float f[D];
      if (!sdf_locate<D>(S, x, c, f)) return __builtin_inff();
      return sdf_phi_frame<D>(S, S.phi0, c, f) * idx;
    }
    float xw[3] = {x[0], x[1], 0.0f};
    if constexpr (D == 3) xw[2] = x[2];
    float phi = 0.0f, n[3];
    levelset_eval_key(&L.shape, 1, xw, idx, phi, n);
    return phi;
  }

  __device__ __forceinline__ float leaf_phi(const RegionLeafDev &L, const float x[D], float idx) const {
    REGION_NO_CONTRACT
    float phi;
    if (L.placed) {
      float d[D], local[D];
#pragma unroll
      for (int k = 0; k < D; k++) d[k] = x[k] - L.t[k];
#pragma unroll
      for (int k = 0; k < D; k++) {
        float y = L.rot[k] * d[0] + L.rot[3 + k] * d[1];
        if constexpr (D == 3) y = y + L.rot[6 + k] * d[2];
        const float q = y * L.inv_scale;
        local[k] = q + L.p[k];
      }
      phi = leaf_own(L, local, idx) * L.scale;
    } else {
      phi = leaf_own(L, x, idx);
    }
    if (L.banded) phi = fmaxf(L.lo - phi, phi - L.hi);
    return phi;
  }

  __device__ __forceinline__ float phi(const float x[D], float idx) const {
    float s0 = __builtin_inff(), s1 = s0, s2 = s0, s3 = s0;
    for (int i = 0; i < n_ops; i++) {
      const int w = ops[i], op = w & 3;
      if (op == MPMHIP_REGION_PUSH) {
        const float v = leaf_phi(leaf[w >> 2], x, idx);
        s3 = s2; s2 = s1; s1 = s0; s0 = v;
      } else if (op == MPMHIP_REGION_NEG) {
        s0 = -s0;
      } else {
        s0 = op == MPMHIP_REGION_UNION ? fminf(s0, s1) : fmaxf(s0, s1);
        s1 = s2; s2 = s3;
      }
    }
    return s0;
  }

  __device__ __forceinline__ bool inside(const float x[D], float idx) const { return phi(x, idx) < 0.0f; }
};

// the description's size in the kernel arguments (4 096 bytes hold them all): what DESIGN.md section 9 and profiles/seed_ab.txt quote
static_assert(sizeof(RegionLeafDev) == 124 && sizeof(SdfDev) == 72, "k_region.h: a leaf of 124 bytes, a field of 72");
static_assert(sizeof(RegionExpr<3>) == 1384 && sizeof(RegionExpr<2>) == 1384, "k_region.h: the region travels as 1 384 bytes");

// phi (grid units) at n given points: one lane per point
template <int D>
__global__ __launch_bounds__(REGION_WG) void k_region_sample(RegionExpr<D> R, float idx, uint32_t n, const float *__restrict__ pos,
                                                             float *__restrict__ out) {
  const uint32_t i = blockIdx.x * (uint32_t)REGION_WG + threadIdx.x;
  if (i >= n) return;
  float x[D];
#pragma unroll
  for (int k = 0; k < D; k++) x[k] = pos[D * (size_t)i + k];
  out[i] = R.phi(x, idx);
}

// phi in world units, clamped to +-band, at the nodes of a lattice of `count` samples in C order: one lane per node
template <int D>
struct RegionLattice {
  int res[D];
  float origin[D];
  float spacing;
};
template <int D>
__global__ __launch_bounds__(REGION_WG) void k_region_bake(RegionExpr<D> R, RegionLattice<D> L, float dx, float idx, float band,
                                                           uint32_t count, float *__restrict__ out) {
  REGION_NO_CONTRACT
  const uint32_t i = blockIdx.x * (uint32_t)REGION_WG + threadIdx.x;
  if (i >= count) return;
  uint32_t rem = i;
  float x[D];
#pragma unroll
  for (int k = D - 1; k >= 0; k--) {
    const uint32_t up = k ? rem / (uint32_t)L.res[k] : 0u;
    const uint32_t at = k ? rem - up * (uint32_t)L.res[k] : rem;
    const float step = (float)at * L.spacing;
    x[k] = L.origin[k] + step;
    rem = up;
  }
  const float w = R.phi(x, idx) * dx;
  out[i] = fminf(fmaxf(w, -band), band);
}

#undef REGION_NO_CONTRACT

}  // namespace mpm
