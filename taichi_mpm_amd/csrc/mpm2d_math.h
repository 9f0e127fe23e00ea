// taichi_mpm_amd/csrc/mpm2d_math.h — 2x2 math and the eight constitutive models of MPM<2> (src/particles.cpp with dim = 2).
// Every 2D kernel evaluates its particles through these functions: k_p2g / k_g2p (k_mpm2d.h), the deterministic mode
// (k_mpm2d_det.h), the CPIC transfers and the asynchronous stepper (k_async.h), and the test entries mpmhip2d_debug_*
// (k_debug2d.h).  Plain C++ (MPM_HD as in k_joints.h): the same lines compile for the host in tests/cpp/mpm2d_math_host.cpp,
// where tests/test_materials2d_cpu.py holds them to the reference's dim = 2 particles without a GPU.
//
// As in 3D (mpm_math.h) every model is isotropic, so stress and return map need only U and the singular values:
// F F^T = U diag(sigma^2) U^T, one Jacobi rotation in 2D.
#pragma once
#include <math.h>

#include "group_params.h"

#if !defined(MPM_HD)
#if defined(__HIPCC__)
#define MPM_HD __host__ __device__ __forceinline__
#else
#define MPM_HD inline
#endif
#endif

namespace mpm2d {

using mpm::GroupParams;

MPM_HD float rsqrt_f(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return rsqrtf(x);
#else
  return 1.0f / sqrtf(x);
#endif
}

struct m2 {
  float a, b, c, d;  // [a b; c d]
};
MPM_HD m2 mul(const m2 &x, const m2 &y) {
  return {x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c, x.c * y.b + x.d * y.d};
}
// a d - b c by Kahan's difference of products: the rounding error of b c is recovered by one fma and added back, so the result is
// good to ~1.5 ulp of the DETERMINANT (not of the products, which are cond(F) times larger: the plain form loses eps cond(F)).
// signed_sigma takes the smaller singular value from it.
MPM_HD float det(const m2 &x) {
  const float w = x.b * x.c;
  const float e = fmaf(-x.b, x.c, w), f = fmaf(x.a, x.d, -w);
  return f + e;
}

// eigen-decomposition of the symmetric F F^T = U diag(lam) U^T by ONE Jacobi rotation (exact in 2D); U = [c s; -s c]^T form:
// columns (c, -s)... kept as (cu, su): U = [cu -su; su cu]
MPM_HD void eig_FFt(const m2 &F, float &cu, float &su, float lam[2]) {
  float app = F.a * F.a + F.b * F.b, aqq = F.c * F.c + F.d * F.d, apq = F.a * F.c + F.b * F.d;
  const float d = aqq - app, x = apq + apq, xx = x * x;
  const float h = sqrtf(d * d + xx), den = fabsf(d) + h, n2 = den * den + xx;
  if (n2 > 1e-30f) {
    const float r = rsqrt_f(n2);
    const float c = den * r, s = (d < 0.0f ? -1.0f : 1.0f) * x * r;
    const float sum = app + aqq, hs = d < 0.0f ? -h : h;
    lam[0] = 0.5f * (sum - hs); lam[1] = 0.5f * (sum + hs);
    // columns p, q of U rotated from the identity: (1,0) -> (c, ?) ...: U = G with G[p][p] = c, G[p][q] = s, G[q][p] = -s, G[q][q] = c
    cu = c; su = -s;  // U = [c s; -s c] = [cu -su; su cu]
  } else {
    lam[0] = app; lam[1] = aqq; cu = 1.0f; su = 0.0f;
  }
}
// The singular values the models consume, the sign of det F on the smaller one.  lam_min = (sum - h) / 2 of eig_FFt cancels like
// eps cond(F)^2 (at cond 1e4 it is mostly <= 0 in fp32), so only the LARGER value is taken from its eigenvalue; the smaller one
// is det F / sigma_max, which carries the error of the determinant alone.  lam of the smaller one is set to match (the
// fixed-corotated stress takes lam - s = s (s - 1)).  No loop, no LDS; DESIGN.md section 2.
MPM_HD void signed_sigma(float lam[2], float detF, float s[2]) {
  const bool hi1 = lam[1] > lam[0];  // (equal: the sign goes on s[0], as before)
  const float smax = sqrtf(fmaxf(hi1 ? lam[1] : lam[0], 0.0f));
  const float smin = smax > 0.0f ? detF / smax : 0.0f;
  s[0] = hi1 ? smin : smax; s[1] = hi1 ? smax : smin;
  lam[0] = hi1 ? smin * smin : lam[0]; lam[1] = hi1 ? lam[1] : smin * smin;
}
// U diag(e) U^T with U = [cu -su; su cu]
MPM_HD m2 sandwich(float cu, float su, const float e[2]) {
  const float xx = cu * cu * e[0] + su * su * e[1], yy = su * su * e[0] + cu * cu * e[1], xy = cu * su * (e[0] - e[1]);
  return {xx, xy, xy, yy};
}

// U diag(ratio) U^T M of the return maps (M = U diag(s) V^T, ratio = new sigma / s), without the eps cond(M) of the plain product:
// the row u_min^T M of U^T M is a difference of entries cond(M) times its size, and ratio_min then multiplies its error (and the
// error of U's angle) by 1 / sigma_min.  The rows of U^T M are s_k v_k^T, orthogonal, with r0 x r1 = det M — so the row of the
// smaller singular value is rebuilt from the larger one, which has no cancellation, and the determinant.
MPM_HD m2 restretch(float cu, float su, const float ratio[2], const float lam[2], float detM, const m2 &M) {
  float r0x = cu * M.a + su * M.c, r0y = cu * M.b + su * M.d;    // u0 = (cu, su)
  float r1x = cu * M.c - su * M.a, r1y = cu * M.d - su * M.b;    // u1 = (-su, cu)
  if (lam[1] > lam[0]) {
    const float n = r1x * r1x + r1y * r1y;
    if (n > 0.0f) { const float k = -detM / n; r0x = -k * r1y; r0y = k * r1x; }
  } else {
    const float n = r0x * r0x + r0y * r0y;
    if (n > 0.0f) { const float k = detM / n; r1x = -k * r0y; r1y = k * r0x; }
  }
  r0x *= ratio[0]; r0y *= ratio[0]; r1x *= ratio[1]; r1y *= ratio[1];
  return {cu * r0x - su * r1x, cu * r0y - su * r1y, su * r0x + cu * r1x, su * r0y + cu * r1y};
}

// calculate_force(): -vol * P(F) * F^T for dim = 2 (src/particles.cpp; same formulas as the 3D path with d = 2)
MPM_HD m2 calculate_force(const GroupParams &g, const m2 &F, float aux) {
  const float vol = g.p[1];
  switch (g.type) {
    case MPMHIP_VISCO:
    case MPMHIP_JELLY:
    case MPMHIP_SNOW: {
      float mu = g.p[2], la = g.p[3];
      if (g.type == MPMHIP_SNOW) { const float e = expf(g.p[4] * (1.0f - aux)); mu *= e; la *= e; }
      float cu, su, lam[2], s[2];
      eig_FFt(F, cu, su, lam);
      const float J = det(F);
      signed_sigma(lam, J, s);
      const float vl = la * (J - 1.0f) * J;
      const float e[2] = {-vol * (2.0f * mu * (lam[0] - s[0]) + vl), -vol * (2.0f * mu * (lam[1] - s[1]) + vl)};
      return sandwich(cu, su, e);
    }
    case MPMHIP_LINEAR: {
      const float mu = g.p[2], la = g.p[3];
      const float tr = la * (F.a + F.d - 2.0f);
      const m2 P = {mu * (2.0f * F.a - 2.0f) + tr, mu * (F.b + F.c), mu * (F.b + F.c), mu * (2.0f * F.d - 2.0f) + tr};
      const m2 Ft = {F.a, F.c, F.b, F.d};
      m2 o = mul(P, Ft);
      o.a *= -vol; o.b *= -vol; o.c *= -vol; o.d *= -vol;
      return o;
    }
    case MPMHIP_WATER: {
      const float p = g.p[2] * (powf(aux, -g.p[3]) - 1.0f);
      const float dd = vol * aux * p;
      return {dd, 0.0f, 0.0f, dd};
    }
    default: {  // SAND, VON_MISES, ELASTIC: P F^T = U (2 mu ln S + lambda tr(ln S) I) U^T
      const float mu = g.p[2], la = g.p[3];
      float cu, su, lam[2], s[2];
      eig_FFt(F, cu, su, lam);
      signed_sigma(lam, det(F), s);
      const float l0 = logf(s[0]), l1 = logf(s[1]), tr = l0 + l1;
      const float e[2] = {-vol * (2.0f * mu * l0 + la * tr), -vol * (2.0f * mu * l1 + la * tr)};
      return sandwich(cu, su, e);
    }
  }
}

// plasticity(cdg) for dim = 2 (src/particles.cpp)
MPM_HD void plasticity(const GroupParams &g, const m2 &cdg, m2 &F, float &aux) {
  if (g.type == MPMHIP_WATER) {  // :469-478  j *= tr(cdg) - (dim - 1)
    const float j = aux * (cdg.a + cdg.d - 1.0f);
    aux = j < 0.1f ? 0.1f : j;
    return;
  }
  if (g.type == MPMHIP_VISCO) {  // :87-134 with dim = 2
    const float mu = g.p[2], la = g.p[3], vnu = g.p[4], kappa = g.p[5], dt = g.p[6];
    float pnorm;
    {
      float cu, su, lam[2], s[2];
      eig_FFt(F, cu, su, lam);
      const float J0 = det(F);
      signed_sigma(lam, J0, s);
      const float p0 = 2.0f * mu * (s[0] - 1.0f) + la * (J0 - 1.0f) * J0 / s[0];
      const float p1 = 2.0f * mu * (s[1] - 1.0f) + la * (J0 - 1.0f) * J0 / s[1];
      pnorm = sqrtf(p0 * p0 + p1 * p1);
    }
    m2 sm = {cdg.a - 1.0f, cdg.b, cdg.c, cdg.d - 1.0f}, r;
    int halvings = 0;
    for (;;) {
      const m2 hm = {0.5f * sm.a + 1.0f, 0.5f * sm.b, 0.5f * sm.c, 0.5f * sm.d + 1.0f};
      r = mul(hm, sm);
      r.a += 1.0f; r.d += 1.0f;
      if (det(r) > 0.0f || halvings > 20) break;
      sm.a *= 0.5f; sm.b *= 0.5f; sm.c *= 0.5f; sm.d *= 0.5f;
      halvings++;
    }
    for (int i = 0; i < halvings; i++) r = mul(r, r);
    F = mul(r, F);
    float cu, su, lam[2], s[2];
    eig_FFt(F, cu, su, lam);
    const float J = det(F);
    signed_sigma(lam, J, s);
    float gamma = 0.0f;
    if (pnorm > 1e-5f) gamma = fminf(fmaxf(dt * vnu * (pnorm - aux) / pnorm, 0.0f), 1.0f);
    const float dets = s[0] * s[1];
    const float scale = fabsf(dets) > 1e-5f ? 1.0f / powf(dets, 0.5f) : 1.0f;
    float ratio[2];
    for (int k = 0; k < 2; k++) {
      const float md = powf(s[k] * scale, gamma);
      const float inv = fabsf(md) > 1e-5f ? 1.0f / md : 1.0f;
      ratio[k] = fminf(fmaxf(s[k] * inv, 0.1f), 10.0f) / s[k];
    }
    aux = aux + kappa * gamma * pnorm;
    F = restretch(cu, su, ratio, lam, J, F);
    return;
  }
  F = mul(cdg, F);
  if (g.type == MPMHIP_JELLY || g.type == MPMHIP_LINEAR || g.type == MPMHIP_ELASTIC) return;
  float cu, su, lam[2], s[2];
  eig_FFt(F, cu, su, lam);
  const float J = det(F);
  signed_sigma(lam, J, s);
  float ratio[2];
  if (g.type == MPMHIP_SNOW) {  // :222-242
    const float lo = 1.0f - g.p[5], hi = 1.0f + g.p[6];
    float det_o = 1.0f, det_n = 1.0f;
    for (int i = 0; i < 2; i++) {
      const float c = fminf(fmaxf(s[i], lo), hi);
      det_o *= s[i]; det_n *= c;
      ratio[i] = c / s[i];
    }
    float Jp = aux * det_o / det_n;
    if (!(Jp <= g.p[8])) Jp = g.p[8];
    if (!(Jp >= g.p[7])) Jp = g.p[7];
    aux = Jp;
  } else if (g.type == MPMHIP_SAND) {  // :599-626, 639-647 with d = 2
    const float mu = g.p[2], la = g.p[3], alpha = g.p[4], coh = g.p[5], beta = g.p[6];
    const float e0 = logf(fmaxf(fabsf(s[0]), 1e-4f)) - coh, e1 = logf(fmaxf(fabsf(s[1]), 1e-4f)) - coh;
    const float sum = e0 + e1, tr = sum + aux;
    const float h0 = e0 - tr * 0.5f, h1 = e1 - tr * 0.5f;
    const float ehn = sqrtf(h0 * h0 + h1 * h1);
    float n0, n1;
    if (tr >= 0.0f) {
      n0 = n1 = expf(coh);
      aux = beta * sum + aux;
    } else {
      aux = 0.0f;
      const float dg = ehn + (2.0f * la + 2.0f * mu) / (2.0f * mu) * tr * alpha;
      const float k = (dg <= 0.0f) ? 0.0f : dg / ehn;
      n0 = expf(e0 - k * h0 + coh); n1 = expf(e1 - k * h1 + coh);
    }
    ratio[0] = n0 / s[0]; ratio[1] = n1 / s[1];
  } else {  // VON_MISES :713-732
    const float e0 = logf(s[0]), e1 = logf(s[1]), tr = e0 + e1;
    const float h0 = e0 - tr * 0.5f, h1 = e1 - tr * 0.5f;
    const float n2 = h0 * h0 + h1 * h1;
    const float dg = n2 - g.p[4] / (2.0f * g.p[2]);
    if (dg <= 0.0f) return;
    ratio[0] = expf(e0 - (dg / n2) * h0) / s[0];
    ratio[1] = expf(e1 - (dg / n2) * h1) / s[1];
  }
  F = restretch(cu, su, ratio, lam, J, F);
}

}  // namespace mpm2d
