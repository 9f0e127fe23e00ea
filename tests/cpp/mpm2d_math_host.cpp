// tests/cpp/mpm2d_math_host.cpp — host build of the 2D constitutive math the device runs (taichi_mpm_amd/csrc/mpm2d_math.h):
// the same header compiled by g++ into a small shared library for tests/test_materials2d_cpu.py, which holds it to the
// reference's dim = 2 particles (tests/golden/ref_materials2d.npz, ref_illcond2d.npz) without a GPU.  The three exports
// mirror mpmhip2d_debug_force / _plasticity / _svd2 (include/mpmhip.h) as plain loops.
//
// With -DMPM2D_MATH_MAIN the file is a stand-alone program instead: it generates a few hundred fixture-like rows per
// material (large strains, cond(F) up to 1e4, det F < 0, scaled rotations, sand's clamp rows, singular and zero F) and
// runs them through the three loops — the place for a sanitizer pass over these lines
//     g++ -std=c++17 -O1 -g -fsanitize=undefined,address -fno-sanitize-recover=all -DMPM2D_MATH_MAIN mpm2d_math_host.cpp
// Non-finite outputs are counted, not refused: only the rows the reference keeps finite are held to be finite (the tests).
#include <cstdint>
#include <cstring>

#include "../../taichi_mpm_amd/csrc/mpm2d_math.h"

namespace {
bool make_group(int32_t material, const float *params, mpm::GroupParams &g) {
  if (material < MPMHIP_VISCO || material > MPMHIP_ELASTIC || !params) return false;
  memset(&g, 0, sizeof g);
  memcpy(g.p, params, sizeof g.p);
  g.type = material;
  return true;
}
}  // namespace

extern "C" {
int mpm2d_host_sizeof_group() { return (int)sizeof(mpm::GroupParams); }

int mpm2d_host_force(int32_t material, const float *params, int64_t n, const float *F, const float *aux, float *out) {
  mpm::GroupParams g;
  if (n < 0 || !F || !aux || !out || !make_group(material, params, g)) return MPMHIP_EINVAL;
  for (int64_t i = 0; i < n; i++) {
    const mpm2d::m2 f = {F[4 * i], F[4 * i + 1], F[4 * i + 2], F[4 * i + 3]};
    const mpm2d::m2 r = mpm2d::calculate_force(g, f, aux[i]);
    out[4 * i] = r.a; out[4 * i + 1] = r.b; out[4 * i + 2] = r.c; out[4 * i + 3] = r.d;
  }
  return MPMHIP_OK;
}

int mpm2d_host_plasticity(int32_t material, const float *params, int64_t n, const float *cdg, float *F, float *aux, float *force_out) {
  mpm::GroupParams g;
  if (n < 0 || !cdg || !F || !aux || !make_group(material, params, g)) return MPMHIP_EINVAL;
  for (int64_t i = 0; i < n; i++) {
    mpm2d::m2 f = {F[4 * i], F[4 * i + 1], F[4 * i + 2], F[4 * i + 3]};
    const mpm2d::m2 c = {cdg[4 * i], cdg[4 * i + 1], cdg[4 * i + 2], cdg[4 * i + 3]};
    float a = aux[i];
    mpm2d::plasticity(g, c, f, a);
    if (g.type != MPMHIP_WATER) { F[4 * i] = f.a; F[4 * i + 1] = f.b; F[4 * i + 2] = f.c; F[4 * i + 3] = f.d; }
    aux[i] = a;
    if (force_out) {
      const mpm2d::m2 r = mpm2d::calculate_force(g, f, a);
      force_out[4 * i] = r.a; force_out[4 * i + 1] = r.b; force_out[4 * i + 2] = r.c; force_out[4 * i + 3] = r.d;
    }
  }
  return MPMHIP_OK;
}

int mpm2d_host_svd2(int64_t n, const float *F, float *cu, float *su, float *S) {
  if (n < 0 || !F || !cu || !su || !S) return MPMHIP_EINVAL;
  for (int64_t i = 0; i < n; i++) {
    const mpm2d::m2 f = {F[4 * i], F[4 * i + 1], F[4 * i + 2], F[4 * i + 3]};
    float lam[2], sg[2];
    mpm2d::eig_FFt(f, cu[i], su[i], lam);
    mpm2d::signed_sigma(lam, mpm2d::det(f), sg);
    S[2 * i] = sg[0]; S[2 * i + 1] = sg[1];
  }
  return MPMHIP_OK;
}
}

#if defined(MPM2D_MATH_MAIN)
#include <cmath>
#include <cstdio>
#include <vector>

namespace {
uint32_t rng_state = 12345u;
float uniform() {  // xorshift32 -> [0, 1)
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
  return (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}
void push_rsr(std::vector<float> &F, double a, double s0, double s1, double b) {  // R(a) diag(s0, s1) R(b)^T
  const double ca = cos(a), sa = sin(a), cb = cos(b), sb = sin(b);
  const double m[4] = {ca * s0, -sa * s1, sa * s0, ca * s1};  // R(a) diag
  F.push_back((float)(m[0] * cb - m[1] * sb)); F.push_back((float)(m[0] * sb + m[1] * cb));
  F.push_back((float)(m[2] * cb - m[3] * sb)); F.push_back((float)(m[2] * sb + m[3] * cb));
}
}  // namespace

int main() {
  std::vector<float> F;
  for (double c : {1.0, 10.0, 1e2, 1e3, 1e4})
    for (double scale : {1.0, 0.8, 1.3})
      for (int k = 0; k < 6; k++) {
        push_rsr(F, 6.28 * uniform(), scale, scale / c, 6.28 * uniform());
        push_rsr(F, 6.28 * uniform(), scale * sqrt(c), scale / sqrt(c), 6.28 * uniform());
        push_rsr(F, 6.28 * uniform(), scale, -scale / c, 6.28 * uniform());
      }
  for (double s : {1.0, 1.5, 2.0, 1e-4, 0.0})
    for (double a : {0.0, 1.5707963267948966, 3.141592653589793, 0.3}) push_rsr(F, a, s, s, 0.0);  // scaled rotations, zero
  for (int k = 0; k < 4; k++) {
    push_rsr(F, 6.28 * uniform(), 1.0, 1e-4, 6.28 * uniform());
    push_rsr(F, 6.28 * uniform(), 1.0, 5e-5, 6.28 * uniform());
    push_rsr(F, 6.28 * uniform(), 2e-4, 0.9e-4, 6.28 * uniform());
    push_rsr(F, 6.28 * uniform(), 1.0, 0.0, 6.28 * uniform());  // singular
  }
  for (int k = 0; k < 120; k++)  // large strains about the identity
    for (int e = 0; e < 4; e++) F.push_back((e == 0 || e == 3 ? 1.0f : 0.0f) + 0.4f * (uniform() - 0.5f));
  const int64_t n = (int64_t)F.size() / 4;
  std::vector<float> cdg(4 * n), aux(n), out(4 * n), f2(4 * n), a2(n), cu(n), su(n), S(2 * n);
  for (int64_t i = 0; i < 4 * n; i++) cdg[i] = (i % 4 == 0 || i % 4 == 3 ? 1.0f : 0.0f) + 0.12f * (uniform() - 0.5f);
  // parameter rows in the layout the models read: mass, vol, mu, lambda, then the type's own (magnitudes of the defaults)
  const float vol = 6.1e-5f, mu = 1.9e4f, la = 2.9e4f;
  int64_t nonfinite = 0;
  for (int32_t mat = MPMHIP_VISCO; mat <= MPMHIP_ELASTIC; mat++) {
    float p[MPMHIP_NPARAM] = {400.0f * vol, vol, mu, la, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = 0; i < n; i++) aux[i] = 0.0f;
    switch (mat) {
      case MPMHIP_SNOW: p[4] = 10.0f; p[5] = 2.5e-2f; p[6] = 7.5e-3f; p[7] = 0.6f; p[8] = 20.0f;
        for (int64_t i = 0; i < n; i++) aux[i] = 0.9f + 0.2f * uniform();
        break;
      case MPMHIP_SAND: p[4] = 0.27f; p[5] = 0.0f; p[6] = 1.0f;
        for (int64_t i = 0; i < n; i++) aux[i] = 0.04f * uniform();
        break;
      case MPMHIP_WATER: p[2] = 1e4f; p[3] = 7.0f;
        for (int64_t i = 0; i < n; i++) aux[i] = 0.9f + 0.2f * uniform();
        break;
      case MPMHIP_VON_MISES: p[4] = 50.0f; break;
      case MPMHIP_VISCO: p[4] = 1e4f; p[5] = 0.0f; p[6] = 1e-4f;
        for (int64_t i = 0; i < n; i++) aux[i] = (i & 1) ? 1000.0f : 10.0f;
        break;
      default: break;
    }
    if (mpm2d_host_force(mat, p, n, F.data(), aux.data(), out.data())) return 2;
    for (float v : out) nonfinite += !std::isfinite(v);
    f2 = F; a2 = aux;
    if (mpm2d_host_plasticity(mat, p, n, cdg.data(), f2.data(), a2.data(), out.data())) return 2;
    for (float v : out) nonfinite += !std::isfinite(v);
    f2 = F; a2 = aux;
    if (mpm2d_host_plasticity(mat, p, n, cdg.data(), f2.data(), a2.data(), nullptr)) return 2;
  }
  if (mpm2d_host_svd2(n, F.data(), cu.data(), su.data(), S.data())) return 2;
  if (mpm2d_host_force(99, nullptr, n, F.data(), aux.data(), out.data()) != MPMHIP_EINVAL) return 3;
  printf("mpm2d_math_host: %lld rows x 8 materials, %lld non-finite output values (singular / det < 0 rows of the log models)\n",
         (long long)n, (long long)nonfinite);
  return 0;
}
#endif
