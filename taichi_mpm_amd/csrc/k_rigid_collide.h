// taichi_mpm_amd/csrc/k_rigid_collide.h — rigid-rigid collisions: MPM::rigidify (src/mpm_rigid_body.cpp:306-345)
// Part of libmpmhip (see mpmhip.hip for the substep overview; k_rigid.h for the bodies, k_joints.h for JointBody).
//
// rigidify(dt) opens the coupling block of a substep (src/mpm.cpp:466-472):
//   detection   RigidSolver<3>::detect_rigid_collision (src/rigid_body_solver.h:150-198): for every pair of bodies i > j >= 1 that
//               are not both fully scripted, libccd's Minkowski Portal Refinement (ccdMPRPenetration, CCD_SINGLE, mpr_tolerance
//               1e-4, centres = the bodies' positions) on the convex hulls of the bodies' mesh vertices -> depth, direction,
//               position of the contact.
//   resolution  `rigid_body_iterations` rounds of [project_position over all collisions (if rigid_body_position_iterations),
//               project_velocity over all collisions], then the same number of rounds of project_velocity alone
//               (Collision<dim>, src/rigid_body_solver.h:39-87): sequential impulses, every one reads what the last one wrote.
//
// The MPR of a deep or tied contact is ill-conditioned (single and double precision builds of libccd disagree by 0.04 in depth
// and tens of degrees in direction on such pairs), so "close to libccd" is not a usable criterion.  Reproducing its fp32
// arithmetic exactly is: every operation below is written in the order libccd performs it, nothing is contracted into an fma,
// sqrt and / are the IEEE ones, and the result is a pure function of the inputs — the host build of this header
// (tests/cpp/rigid_collide_host.cpp), the device and libccd itself (tests/golden/rigid_mpr.npz) agree bit for bit.
// That is also why the arithmetic does not go through the j_* helpers of k_joints.h: those may be contracted on the device
// (and the joints' tests pin them as they are); the c_* functions below are their uncontracted twins.
//
// The support mapping (supportRigid, :120-147) is the hot loop: arg-max of dot(dir, R v) over the body's vertices, the FIRST
// vertex winning a tie (the reference's strict >).  A pre-pass writes r = R v and p = r + pos for every vertex once per rigidify;
// one workgroup handles one pair, its lanes stride the vertex arrays, a wave reduction on (value, index) and one LDS step
// across the waves give the winner to every lane.  The portal itself (four support points) is uniform across the workgroup
// and is carried redundantly by every lane: identical inputs, identical arithmetic, identical branches.
//
// libccd's max_iterations is unlimited; every loop here is bounded (MPR_MAX_*).  A pair whose bound expires reports no
// collision and sets RIGID_MPR_ERROR_BIT in the ctx's sticky error word.
#pragma once
#include <math.h>
#include <stdint.h>

#include "k_joints.h"

#if defined(__clang__)
#define MPR_EXACT _Pragma("clang fp contract(off)")  // first statement of a block: no fma contraction inside it
#else
#define MPR_EXACT  // (g++: build with -ffp-contract=off)
#endif

namespace mpm {

constexpr float MPR_EPS = 1.1920928955078125e-07f;  // CCD_EPS = FLT_EPSILON
constexpr float MPR_TOLERANCE = 1e-4f;              // ccd.mpr_tolerance (src/rigid_body_solver.h:184)
// loop bounds, in support calls: the largest count of any pair of tests/golden/rigid_mpr.npz is recorded there
// (max_support_calls); tests/test_rigid_collide_cpu.py asserts every bound below is at least 4 x that
constexpr int MPR_MAX_DISCOVER = 256;  // the while loop of portal discovery
constexpr int MPR_MAX_REFINE = 256;    // portal refinement
constexpr int MPR_MAX_PENETR = 256;    // findPenetr
constexpr uint32_t RIGID_MPR_ERROR_BIT = 32u;
constexpr int MAX_RIGID_PAIRS = 55;    // bodies 1 .. 11: 11 * 10 / 2

// ------------------------------------------------------------------------------------------------ exact fp32 vector helpers
// IEEE square root and division: the library is built without fast-math, where sqrtf and / are the correctly rounded ones on the
// device as on the host (the __fsqrt_rn / __fdiv_rn intrinsics are NOT: without OCML's rounded operations they are the native,
// 1-ulp instructions)
MPM_HD float c_sqrt(float x) { return sqrtf(x); }
MPM_HD float c_div(float a, float b) { return a / b; }
MPM_HD float c_dot(const float a[3], const float b[3]) {
  MPR_EXACT
  float d = a[0] * b[0];
  d += a[1] * b[1];
  d += a[2] * b[2];
  return d;
}
MPM_HD void c_cross(const float a[3], const float b[3], float o[3]) {  // o must not alias a or b
  MPR_EXACT
  o[0] = (a[1] * b[2]) - (a[2] * b[1]);
  o[1] = (a[2] * b[0]) - (a[0] * b[2]);
  o[2] = (a[0] * b[1]) - (a[1] * b[0]);
}
MPM_HD void c_sub(const float a[3], const float b[3], float o[3]) { MPR_EXACT for (int k = 0; k < 3; k++) o[k] = a[k] - b[k]; }
MPM_HD void c_add(float a[3], const float b[3]) { MPR_EXACT for (int k = 0; k < 3; k++) a[k] += b[k]; }
MPM_HD void c_scale(float a[3], float s) { MPR_EXACT for (int k = 0; k < 3; k++) a[k] *= s; }
MPM_HD void c_copy(float a[3], const float b[3]) { for (int k = 0; k < 3; k++) a[k] = b[k]; }
MPM_HD void c_normalize(float a[3]) { MPR_EXACT c_scale(a, c_div(1.0f, c_sqrt(c_dot(a, a)))); }
MPM_HD float c_dist2(const float a[3], const float b[3]) {
  MPR_EXACT
  float d[3];
  c_sub(a, b, d);
  return c_dot(d, d);
}
MPM_HD bool c_is_zero(float x) { return fabsf(x) < MPR_EPS; }
MPM_HD bool c_eq(float a, float b) {  // ccdEq
  MPR_EXACT
  const float ab = fabsf(a - b);
  if (ab < MPR_EPS) return true;
  const float fa = fabsf(a), fb = fabsf(b);
  return fb > fa ? ab < MPR_EPS * fb : ab < MPR_EPS * fa;
}
MPM_HD bool c_vec_is_origin(const float a[3]) { return c_eq(a[0], 0.0f) && c_eq(a[1], 0.0f) && c_eq(a[2], 0.0f); }
MPM_HD void c_mat_vec(const float M[9], const float v[3], float o[3]) {
  MPR_EXACT
  for (int r = 0; r < 3; r++) {
    float d = M[3 * r] * v[0];
    d += M[3 * r + 1] * v[1];
    d += M[3 * r + 2] * v[2];
    o[r] = d;
  }
}
// what the pre-pass writes for a hull vertex v of a body (R, pos): r = R v, p = r + pos — one fixed operation order
MPM_HD void hull_vertex(const float R[9], const float pos[3], const float v[3], float r[3], float p[3]) {
  MPR_EXACT
  c_mat_vec(R, v, r);
  for (int k = 0; k < 3; k++) p[k] = r[k] + pos[k];
}

// ------------------------------------------------------------------------------------------------ support mapping
// a point of the Minkowski difference: v = a - b, a on the first body, b on the second
struct MprPoint { float v[3], a[3], b[3]; };
// the portal: v0 an interior point of the Minkowski difference, v1 v2 v3 the face the origin ray leaves through.  Four named
// members and no array: every access is static, so the whole portal lives in registers
struct MprPortal { MprPoint v0, v1, v2, v3; };
// dst = src where `take`: a select per component, never a store through a selected address (which would put the portal in memory)
MPM_HD void mpr_take(bool take, MprPoint &dst, const MprPoint &src) {
  for (int k = 0; k < 3; k++) {
    dst.v[k] = take ? src.v[k] : dst.v[k];
    dst.a[k] = take ? src.a[k] : dst.a[k];
    dst.b[k] = take ? src.b[k] : dst.b[k];
  }
}

// the direction a body's support is asked in: normalised once more, as supportRigid does (:126-127)
MPM_HD void support_dir(const float dir[3], float sign, float nd[3]) {
  MPR_EXACT
  for (int k = 0; k < 3; k++) nd[k] = dir[k] * sign;
  c_normalize(nd);
}
// one candidate against the best so far: larger value, then smaller index (the reference's strict > in ascending order)
MPM_HD void support_take(float v, int i, float &best, int &idx) {
  if (v > best || (v == best && i < idx)) { best = v; idx = i; }
}
constexpr float SUPPORT_FLOOR = -1e30f;  // supportRigid's initial max_dist: a vertex has to exceed it
constexpr int SUPPORT_NONE = 0x7FFFFFFF;

// host: a plain walk over r[n][3] / p[n][3]
struct HullView { const float *r, *p; int n; };
MPM_HD void support_walk(const HullView &H, const float nd[3], float out[3]) {
  float best = SUPPORT_FLOOR;
  int idx = SUPPORT_NONE;
  for (int i = 0; i < H.n; i++) {
    const float d = c_dot(nd, H.r + 3 * i);
    if (d > best) { best = d; idx = i; }
  }
  if (idx == SUPPORT_NONE) idx = 0;  // (a NaN direction: the reference leaves its output untouched; here vertex 0)
  c_copy(out, H.p + 3 * idx);
}
struct HostSupport {
  HullView A, B;
  MPM_HD void operator()(const float dir[3], float a[3], float b[3]) const {
    float nd[3];
    support_dir(dir, 1.0f, nd);
    support_walk(A, nd, a);
    support_dir(dir, -1.0f, nd);  // __ccdSupport: the second body is asked along -dir
    support_walk(B, nd, b);
  }
};

// ------------------------------------------------------------------------------------------------ MPR
struct MprResult {
  int hit;       // 1: ccdMPRPenetration returned 0 (the bodies intersect or touch)
  float depth, dir[3], pos[3];
  int calls;     // support calls (Minkowski-difference points asked for)
  int expired;   // a loop bound ran out: reported as no collision
};

template <class S>
MPM_HD void mpr_support(S &sup, const float dir[3], MprPoint &o, int &calls) {
  MPR_EXACT
  sup(dir, o.a, o.b);
  c_sub(o.a, o.b, o.v);
  calls++;
}
MPM_HD void mpr_portal_dir(const MprPortal &P, float dir[3]) {
  MPR_EXACT
  float v2v1[3], v3v1[3];
  c_sub(P.v2.v, P.v1.v, v2v1);
  c_sub(P.v3.v, P.v1.v, v3v1);
  c_cross(v2v1, v3v1, dir);
  c_normalize(dir);
}
MPM_HD bool mpr_reach_tolerance(const MprPortal &P, const MprPoint &v4, const float dir[3]) {
  MPR_EXACT
  const float dv1 = c_dot(P.v1.v, dir), dv2 = c_dot(P.v2.v, dir), dv3 = c_dot(P.v3.v, dir), dv4 = c_dot(v4.v, dir);
  float d1 = dv4 - dv1;
  const float d2 = dv4 - dv2, d3 = dv4 - dv3;
  d1 = fminf(d1, d2);
  d1 = fminf(d1, d3);
  return c_eq(d1, MPR_TOLERANCE) || d1 < MPR_TOLERANCE;
}
MPM_HD void mpr_expand(MprPortal &P, const MprPoint &v4) {
  MPR_EXACT
  float v4v0[3];
  c_cross(v4.v, P.v0.v, v4v0);
  int which;  // the vertex v4 replaces
  if (c_dot(P.v1.v, v4v0) > 0.0f) which = c_dot(P.v2.v, v4v0) > 0.0f ? 1 : 3;
  else which = c_dot(P.v3.v, v4v0) > 0.0f ? 2 : 1;
  mpr_take(which == 1, P.v1, v4);
  mpr_take(which == 2, P.v2, v4);
  mpr_take(which == 3, P.v3, v4);
}
// squared distance of P to the segment x0-b and the closest point (vec3.c: __ccdVec3PointSegmentDist2, witness given)
MPM_HD float c_point_segment_dist2(const float P[3], const float x0[3], const float b[3], float wit[3]) {
  MPR_EXACT
  float d[3], a[3];
  c_sub(b, x0, d);
  c_sub(x0, P, a);
  float t = -1.0f * c_dot(a, d);
  t = c_div(t, c_dot(d, d));
  if (t < 0.0f || c_is_zero(t)) {
    c_copy(wit, x0);
    return c_dist2(x0, P);
  }
  if (t > 1.0f || c_eq(t, 1.0f)) {
    c_copy(wit, b);
    return c_dist2(b, P);
  }
  c_copy(wit, d);
  c_scale(wit, t);
  c_add(wit, x0);
  return c_dist2(wit, P);
}
// ... to the triangle x0-B-C (ccdVec3PointTriDist2, witness given)
MPM_HD float c_point_tri_dist2(const float P[3], const float x0[3], const float B[3], const float C[3], float wit[3]) {
  MPR_EXACT
  float d1[3], d2[3], a[3];
  c_sub(B, x0, d1);
  c_sub(C, x0, d2);
  c_sub(x0, P, a);
  const float v = c_dot(d1, d1), w = c_dot(d2, d2), p = c_dot(a, d1), q = c_dot(a, d2), r = c_dot(d1, d2);
  const float s = c_div(q * r - w * p, w * v - r * r);
  const float t = c_div(-s * r - q, w);
  if ((c_is_zero(s) || s > 0.0f) && (c_eq(s, 1.0f) || s < 1.0f) && (c_is_zero(t) || t > 0.0f) && (c_eq(t, 1.0f) || t < 1.0f) &&
      (c_eq(t + s, 1.0f) || t + s < 1.0f)) {
    c_scale(d1, s);
    c_scale(d2, t);
    c_copy(wit, x0);
    c_add(wit, d1);
    c_add(wit, d2);
    return c_dist2(wit, P);
  }
  float w2[3];
  float dist = c_point_segment_dist2(P, x0, B, wit);
  float dist2 = c_point_segment_dist2(P, x0, C, w2);
  if (dist2 < dist) { dist = dist2; c_copy(wit, w2); }
  dist2 = c_point_segment_dist2(P, B, C, w2);
  if (dist2 < dist) { dist = dist2; c_copy(wit, w2); }
  return dist;
}
MPM_HD void mpr_weigh(const MprPoint &q, float w, float p1[3], float p2[3]) {  // p1 += w q.a, p2 += w q.b
  MPR_EXACT
  float vec[3];
  c_copy(vec, q.a); c_scale(vec, w); c_add(p1, vec);
  c_copy(vec, q.b); c_scale(vec, w); c_add(p2, vec);
}
// the contact position from the portal's barycentric coordinates of the origin (findPos)
MPM_HD void mpr_find_pos(const MprPortal &P, float pos[3]) {
  MPR_EXACT
  float dir[3], vec[3], b[4];
  mpr_portal_dir(P, dir);
  c_cross(P.v1.v, P.v2.v, vec); b[0] = c_dot(vec, P.v3.v);
  c_cross(P.v3.v, P.v2.v, vec); b[1] = c_dot(vec, P.v0.v);
  c_cross(P.v0.v, P.v1.v, vec); b[2] = c_dot(vec, P.v3.v);
  c_cross(P.v2.v, P.v1.v, vec); b[3] = c_dot(vec, P.v0.v);
  float sum = b[0] + b[1] + b[2] + b[3];
  if (c_is_zero(sum) || sum < 0.0f) {
    b[0] = 0.0f;
    c_cross(P.v2.v, P.v3.v, vec); b[1] = c_dot(vec, dir);
    c_cross(P.v3.v, P.v1.v, vec); b[2] = c_dot(vec, dir);
    c_cross(P.v1.v, P.v2.v, vec); b[3] = c_dot(vec, dir);
    sum = b[1] + b[2] + b[3];
  }
  const float inv = c_div(1.0f, sum);
  float p1[3] = {0.0f, 0.0f, 0.0f}, p2[3] = {0.0f, 0.0f, 0.0f};
  mpr_weigh(P.v0, b[0], p1, p2);
  mpr_weigh(P.v1, b[1], p1, p2);
  mpr_weigh(P.v2, b[2], p1, p2);
  mpr_weigh(P.v3, b[3], p1, p2);
  c_scale(p1, inv);
  c_scale(p2, inv);
  c_copy(pos, p1);
  c_add(pos, p2);
  c_scale(pos, 0.5f);
}

// portal discovery: -1 the origin is outside, 1 it lies on v1, 2 on the segment v0-v1, 0 a portal was built; -2 bound expired
template <class S>
MPM_HD int mpr_discover(S &sup, const float c1[3], const float c2[3], MprPortal &P, int &calls) {
  MPR_EXACT
  float dir[3], va[3], vb[3];
  c_copy(P.v0.a, c1);
  c_copy(P.v0.b, c2);
  c_sub(c1, c2, P.v0.v);
  if (c_vec_is_origin(P.v0.v)) {  // the centres coincide: moved a little, so that a direction exists
    const float nudge[3] = {MPR_EPS * 10.0f, 0.0f, 0.0f};
    c_add(P.v0.v, nudge);
  }
  c_copy(dir, P.v0.v);
  c_scale(dir, -1.0f);
  c_normalize(dir);
  mpr_support(sup, dir, P.v1, calls);
  float dot = c_dot(P.v1.v, dir);
  if (c_is_zero(dot) || dot < 0.0f) return -1;
  c_cross(P.v0.v, P.v1.v, dir);
  if (c_is_zero(c_dot(dir, dir))) return c_vec_is_origin(P.v1.v) ? 1 : 2;
  c_normalize(dir);
  mpr_support(sup, dir, P.v2, calls);
  dot = c_dot(P.v2.v, dir);
  if (c_is_zero(dot) || dot < 0.0f) return -1;
  c_sub(P.v1.v, P.v0.v, va);
  c_sub(P.v2.v, P.v0.v, vb);
  c_cross(va, vb, dir);
  c_normalize(dir);
  dot = c_dot(dir, P.v0.v);
  {  // the faces are kept oriented away from the origin
    const bool flip = dot > 0.0f;
    const MprPoint t = P.v1;
    mpr_take(flip, P.v1, P.v2);
    mpr_take(flip, P.v2, t);
    if (flip) c_scale(dir, -1.0f);
  }
  for (int it = 0; it < MPR_MAX_DISCOVER; it++) {
    mpr_support(sup, dir, P.v3, calls);
    dot = c_dot(P.v3.v, dir);
    if (c_is_zero(dot) || dot < 0.0f) return -1;
    bool cont = false;
    c_cross(P.v1.v, P.v3.v, va);  // the origin outside (v1, v0, v3): v3 replaces v2
    dot = c_dot(va, P.v0.v);
    cont = dot < 0.0f && !c_is_zero(dot);
    mpr_take(cont, P.v2, P.v3);
    if (!cont) {
      c_cross(P.v3.v, P.v2.v, va);  // outside (v3, v0, v2): v3 replaces v1
      dot = c_dot(va, P.v0.v);
      cont = dot < 0.0f && !c_is_zero(dot);
      mpr_take(cont, P.v1, P.v3);
    }
    if (!cont) return 0;
    c_sub(P.v1.v, P.v0.v, va);
    c_sub(P.v2.v, P.v0.v, vb);
    c_cross(va, vb, dir);
    c_normalize(dir);
  }
  return -2;
}

// ccdMPRPenetration(body 1, body 2) with centres c1, c2
template <class S>
MPM_HD void mpr_penetration(S &sup, const float c1[3], const float c2[3], MprResult &out) {
  MPR_EXACT
  MprPortal P;
  MprPoint v4;
  float dir[3];
  out.hit = 0; out.depth = 0.0f; out.calls = 0; out.expired = 0;
  for (int k = 0; k < 3; k++) out.dir[k] = out.pos[k] = 0.0f;
  const int res = mpr_discover(sup, c1, c2, P, out.calls);
  if (res == -2) { out.expired = 1; return; }
  if (res < 0) return;
  if (res == 1) {  // findPenetrTouch: touching contact on v1
    c_copy(out.pos, P.v1.a);
    c_add(out.pos, P.v1.b);
    c_scale(out.pos, 0.5f);
    out.hit = 1;
    return;
  }
  if (res == 2) {  // findPenetrSegment: the origin on v0-v1
    c_copy(out.pos, P.v1.a);
    c_add(out.pos, P.v1.b);
    c_scale(out.pos, 0.5f);
    c_copy(out.dir, P.v1.v);
    out.depth = c_sqrt(c_dot(out.dir, out.dir));
    c_normalize(out.dir);
    out.hit = 1;
    return;
  }
  bool inside = false;
  for (int it = 0; it < MPR_MAX_REFINE; it++) {  // refinePortal
    mpr_portal_dir(P, dir);
    const float d1 = c_dot(dir, P.v1.v);
    if (c_is_zero(d1) || d1 > 0.0f) { inside = true; break; }
    mpr_support(sup, dir, v4, out.calls);
    const float d4 = c_dot(v4.v, dir);
    if (!(c_is_zero(d4) || d4 > 0.0f) || mpr_reach_tolerance(P, v4, dir)) return;
    mpr_expand(P, v4);
  }
  if (!inside) { out.expired = 1; return; }
  for (int it = 0; it < MPR_MAX_PENETR; it++) {  // findPenetr
    mpr_portal_dir(P, dir);
    mpr_support(sup, dir, v4, out.calls);
    if (mpr_reach_tolerance(P, v4, dir)) {
      const float origin[3] = {0.0f, 0.0f, 0.0f};
      out.depth = c_sqrt(c_point_tri_dist2(origin, P.v1.v, P.v2.v, P.v3.v, out.dir));
      c_normalize(out.dir);
      mpr_find_pos(P, out.pos);
      out.hit = 1;
      return;
    }
    mpr_expand(P, v4);
  }
  out.expired = 1;
}

// ------------------------------------------------------------------------------------------------ resolution
struct RigidCollision {  // Collision<3>: objects[0] = body i, objects[1] = body j (i > j)
  int hit, i, j, calls;
  float depth, dir[3], pos[3];
};
constexpr int MAX_COLLIDE_BODIES = 12;  // = MAX_RIGID of k_rigid.h (asserted where both are visible)
struct RigidContactParams { float fric[MAX_COLLIDE_BODIES], rest[MAX_COLLIDE_BODIES]; };  // per body: frictions[0], restitution (indexed by body)
struct RigidSolveConfig { int iterations, position_iterations; float penalty, dt; };
// canonical index of the pair (i, j), i > j >= 1: (2,1) (3,1) (3,2) (4,1) ... — the order of the collision list
MPM_HD int rigid_pair_index(int i, int j) { return (i - 1) * (i - 2) / 2 + (j - 1); }
MPM_HD int rigid_pair_count(int nb) { return nb >= 3 ? (nb - 1) * (nb - 2) / 2 : 0; }  // nb counts the background

MPM_HD void c_to_world(const float R[9], const float M[9], float o[9]) {  // R M R^T
  MPR_EXACT
  float t[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      float d = R[3 * r] * M[c];
      d += R[3 * r + 1] * M[3 + c];
      d += R[3 * r + 2] * M[6 + c];
      t[3 * r + c] = d;
    }
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      float d = t[3 * r] * R[3 * c];
      d += t[3 * r + 1] * R[3 * c + 1];
      d += t[3 * r + 2] * R[3 * c + 2];
      o[3 * r + c] = d;
    }
}
MPM_HD void c_apply_impulse(JointBody &B, const float imp[3], const float r[3]) {
  MPR_EXACT
  for (int k = 0; k < 3; k++) B.vel[k] += imp[k] * B.inv_mass;
  float t[3], d[3];
  c_cross(r, imp, t);
  c_mat_vec(B.Iw, t, d);
  c_add(B.omega, d);
}
MPM_HD void c_velocity_at(const JointBody &B, const float r[3], float o[3]) {
  MPR_EXACT
  float c[3];
  c_cross(B.omega, r, c);
  for (int k = 0; k < 3; k++) o[k] = B.vel[k] + c[k];
}
MPM_HD float c_impulse_contribution(const JointBody &B, const float r[3], const float n[3]) {
  MPR_EXACT
  float rn[3], t[3], u[3];
  c_cross(r, n, rn);
  c_mat_vec(B.Iw, rn, t);
  c_cross(t, r, u);
  return B.inv_mass + c_dot(u, n);
}
// what one projection did (tests): the normal impulse J and the friction impulse j (0 where it returned early) and the impulse
// vectors handed to apply_impulse for body i and body j, normal then friction
struct RigidImpulse { float J, j, normal_i[3], normal_j[3], friction_i[3], friction_j[3]; };
MPM_HD void rigid_impulse_clear(RigidImpulse *log) {
  if (!log) return;
  log->J = log->j = 0.0f;
  for (int k = 0; k < 3; k++) log->normal_i[k] = log->normal_j[k] = log->friction_i[k] = log->friction_j[k] = 0.0f;
}

// Collision::project_velocity (:39-71)
MPM_HD void collision_project_velocity(const RigidCollision &C, JointBody &A, JointBody &B, float friction, float restitution,
                                       RigidImpulse *log) {
  MPR_EXACT
  rigid_impulse_clear(log);
  float r0[3], r1[3], va[3], vb[3], v10[3];
  c_sub(C.pos, A.pos, r0);
  c_sub(C.pos, B.pos, r1);
  c_velocity_at(B, r1, vb);
  c_velocity_at(A, r0, va);
  c_sub(vb, va, v10);
  const float v0 = -c_dot(C.dir, v10);
  const float J = ((1.0f + restitution) * v0) * c_div(1.0f, c_impulse_contribution(A, r0, C.dir) + c_impulse_contribution(B, r1, C.dir));
  if (!(J >= 0.0f)) return;  // J < 0: separating (and 0 / 0 of two immovable bodies)
  float imp[3], nimp[3];
  for (int k = 0; k < 3; k++) { imp[k] = J * C.dir[k]; nimp[k] = -imp[k]; }
  c_apply_impulse(A, nimp, r0);
  c_apply_impulse(B, imp, r1);
  if (log) { log->J = J; c_copy(log->normal_i, nimp); c_copy(log->normal_j, imp); }
  c_velocity_at(B, r1, vb);
  c_velocity_at(A, r0, va);
  c_sub(vb, va, v10);
  const float vn = c_dot(C.dir, v10);
  float tao[3];
  for (int k = 0; k < 3; k++) tao[k] = v10[k] - C.dir[k] * vn;
  if (fmaxf(fabsf(tao[0]), fmaxf(fabsf(tao[1]), fabsf(tao[2]))) > 1e-7f) {
    c_scale(tao, c_div(1.0f, c_sqrt(c_dot(tao, tao))));
    float j = c_div(-c_dot(v10, tao), c_impulse_contribution(A, r0, tao) + c_impulse_contribution(B, r1, tao));
    j = fmaxf(fminf(j, friction * J), -friction * J);
    float fi[3], nfi[3];
    for (int k = 0; k < 3; k++) { fi[k] = j * tao[k]; nfi[k] = -fi[k]; }
    c_apply_impulse(A, nfi, r0);
    c_apply_impulse(B, fi, r1);
    if (log) { log->j = j; c_copy(log->friction_i, nfi); c_copy(log->friction_j, fi); }
  }
}
// Collision::project_position (:73-87)
MPM_HD void collision_project_position(const RigidCollision &C, JointBody &A, JointBody &B, float dt, float penalty, RigidImpulse *log) {
  MPR_EXACT
  rigid_impulse_clear(log);
  float r0[3], r1[3];
  c_sub(C.pos, A.pos, r0);
  c_sub(C.pos, B.pos, r1);
  const float J = penalty * dt * C.depth * c_div(1.0f, c_impulse_contribution(A, r0, C.dir) + c_impulse_contribution(B, r1, C.dir));
  if (!(J >= 0.0f)) return;
  float imp[3], nimp[3];
  for (int k = 0; k < 3; k++) { imp[k] = J * C.dir[k]; nimp[k] = -imp[k]; }
  c_apply_impulse(A, nimp, r0);
  c_apply_impulse(B, imp, r1);
  if (log) { log->J = J; c_copy(log->normal_i, nimp); c_copy(log->normal_j, imp); }
}
// the resolution half of MPM::rigidify (src/mpm_rigid_body.cpp:325-344) on the bodies b[0 .. nb) and the collisions cols[0 .. nc)
// (hits only, in list order).  log: one RigidImpulse per projection in the order they run, or null; returns their number.
MPM_HD int rigidify_resolve(JointBody *b, int nb, const RigidContactParams &cp, const RigidCollision *cols, int nc,
                            const RigidSolveConfig &cfg, RigidImpulse *log) {
  MPR_EXACT
  if (nc == 0) return 0;
  for (int i = 0; i < nb; i++) c_to_world(b[i].R, b[i].inv_I, b[i].Iw);
  int nl = 0;
  for (int pass = 0; pass < 2; pass++)
    for (int it = 0; it < cfg.iterations; it++) {
      if (pass == 0 && cfg.position_iterations)
        for (int c = 0; c < nc; c++)
          collision_project_position(cols[c], b[cols[c].i], b[cols[c].j], cfg.dt, cfg.penalty, log ? log + nl++ : nullptr);
      for (int c = 0; c < nc; c++) {
        const RigidCollision &C = cols[c];
        collision_project_velocity(C, b[C.i], b[C.j], c_sqrt(cp.fric[C.i] * cp.fric[C.j]), c_sqrt(cp.rest[C.i] * cp.rest[C.j]),
                                   log ? log + nl++ : nullptr);
      }
    }
  return nl;
}

// ------------------------------------------------------------------------------------------------ device
#if defined(__HIPCC__)
static_assert(MAX_COLLIDE_BODIES == MAX_RIGID && MAX_RIGID_PAIRS == (MAX_RIGID - 1) * (MAX_RIGID - 2) / 2, "pair table size");
// pre-pass: r = R v and p = r + pos of every hull vertex (body[v]: the vertex's body)
__global__ __launch_bounds__(256) void k_rigid_hull_pose(const RigidBodyDev *__restrict__ rb, const float *__restrict__ verts,
                                                         const int *__restrict__ body, int n, float4 *__restrict__ r4,
                                                         float4 *__restrict__ p4) {
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const RigidBodyDev &B = rb[body[v]];
    const float x[3] = {verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]};
    float r[3], p[3];
    hull_vertex(B.R, B.pos, x, r, p);
    r4[v] = make_float4(r[0], r[1], r[2], 0.0f);
    p4[v] = make_float4(p[0], p[1], p[2], 0.0f);
  }
}
// the same for the stand-alone test entry: cloud c has rotation rot[9 c] (null: identity — r = v) and centre ctr[3 c]
__global__ __launch_bounds__(256) void k_rigid_cloud_pose(const float *__restrict__ verts, const int *__restrict__ cloud,
                                                          const float *__restrict__ rot, const float *__restrict__ ctr, int n,
                                                          float4 *__restrict__ r4, float4 *__restrict__ p4) {
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const int c = cloud[v];
    const float x[3] = {verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]};
    float r[3], p[3];
    if (rot) hull_vertex(rot + 9 * c, ctr + 3 * c, x, r, p);
    else for (int k = 0; k < 3; k++) { r[k] = x[k]; p[k] = r[k] + ctr[3 * c + k]; }
    r4[v] = make_float4(r[0], r[1], r[2], 0.0f);
    p4[v] = make_float4(p[0], p[1], p[2], 0.0f);
  }
}

constexpr int MPR_WG = 256;  // lanes per pair
// the support mapping of both bodies of a pair by the whole workgroup; every lane returns the same two points.
// One barrier per call: the LDS slots alternate, and a wave can only be one call ahead of the slowest (it waits at the next barrier).
struct WgSupport {
  const float4 *rA, *pA, *rB, *pB;
  int nA, nB;
  float (*slot)[MPR_WG / 64][4];  // [2][waves]: best value / index of A, of B
  int parity;
  __device__ void operator()(const float dir[3], float a[3], float b[3]) {
    float ndA[3], ndB[3];
    support_dir(dir, 1.0f, ndA);
    support_dir(dir, -1.0f, ndB);
    float bestA = SUPPORT_FLOOR, bestB = SUPPORT_FLOOR;
    int ia = SUPPORT_NONE, ib = SUPPORT_NONE;
    for (int i = threadIdx.x; i < nA; i += MPR_WG) {
      const float4 r = rA[i];
      const float x[3] = {r.x, r.y, r.z};
      const float d = c_dot(ndA, x);
      if (d > bestA) { bestA = d; ia = i; }
    }
    for (int i = threadIdx.x; i < nB; i += MPR_WG) {
      const float4 r = rB[i];
      const float x[3] = {r.x, r.y, r.z};
      const float d = c_dot(ndB, x);
      if (d > bestB) { bestB = d; ib = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      support_take(__shfl_xor(bestA, off), __shfl_xor(ia, off), bestA, ia);
      support_take(__shfl_xor(bestB, off), __shfl_xor(ib, off), bestB, ib);
    }
    float *mine = slot[parity][threadIdx.x >> 6];
    if ((threadIdx.x & 63) == 0) { mine[0] = bestA; mine[1] = __int_as_float(ia); mine[2] = bestB; mine[3] = __int_as_float(ib); }
    __syncthreads();
    bestA = bestB = SUPPORT_FLOOR;
    ia = ib = SUPPORT_NONE;
#pragma unroll
    for (int w = 0; w < MPR_WG / 64; w++) {
      const float *s = slot[parity][w];
      support_take(s[0], __float_as_int(s[1]), bestA, ia);
      support_take(s[2], __float_as_int(s[3]), bestB, ib);
    }
    parity ^= 1;
    if (ia == SUPPORT_NONE) ia = 0;
    if (ib == SUPPORT_NONE) ib = 0;
    const float4 pa = pA[ia], pb = pB[ib];
    a[0] = pa.x; a[1] = pa.y; a[2] = pa.z;
    b[0] = pb.x; b[1] = pb.y; b[2] = pb.z;
  }
};
// one pair per workgroup.  pairs[q] = (cloud of body 1, cloud of body 2, skip); first / count: each cloud's vertices; ctr: centres.
// out[q] is written by lane 0 — at the pair's own index, whatever order the workgroups finish in.
struct MprPair { int a, b, skip, pad; };
__global__ __launch_bounds__(MPR_WG) void k_rigid_mpr(const MprPair *__restrict__ pairs, const int *__restrict__ first,
                                                      const int *__restrict__ count, const float *__restrict__ ctr,
                                                      const float4 *__restrict__ r4, const float4 *__restrict__ p4,
                                                      RigidCollision *__restrict__ out, uint32_t *error) {
  __shared__ float slot[2][MPR_WG / 64][4];
  const int q = blockIdx.x;
  const MprPair pr = pairs[q];
  MprResult res;
  res.hit = 0; res.depth = 0.0f; res.calls = 0; res.expired = 0;
  for (int k = 0; k < 3; k++) res.dir[k] = res.pos[k] = 0.0f;
  if (!pr.skip && count[pr.a] > 0 && count[pr.b] > 0) {  // (workgroup-uniform)
    WgSupport sup;
    sup.rA = r4 + first[pr.a]; sup.pA = p4 + first[pr.a]; sup.nA = count[pr.a];
    sup.rB = r4 + first[pr.b]; sup.pB = p4 + first[pr.b]; sup.nB = count[pr.b];
    sup.slot = slot; sup.parity = 0;
    const float c1[3] = {ctr[3 * pr.a], ctr[3 * pr.a + 1], ctr[3 * pr.a + 2]};
    const float c2[3] = {ctr[3 * pr.b], ctr[3 * pr.b + 1], ctr[3 * pr.b + 2]};
    mpr_penetration(sup, c1, c2, res);
  }
  if (threadIdx.x == 0) {
    RigidCollision C;
    C.hit = res.hit; C.i = pr.a; C.j = pr.b; C.calls = res.calls; C.depth = res.depth;
    for (int k = 0; k < 3; k++) { C.dir[k] = res.dir[k]; C.pos[k] = res.pos[k]; }
    out[q] = C;
    if (res.expired && error) atomicOr(error, RIGID_MPR_ERROR_BIT);
  }
}
// the bodies' centres and the pair table of a ctx: pair q = (i, j) of rigid_pair_index, skipped when both follow a script in
// position and rotation (:174-176)
__global__ __launch_bounds__(64) void k_rigid_pairs(const RigidBodyDev *__restrict__ rb, int nb, MprPair *__restrict__ pairs,
                                                    float *__restrict__ ctr) {
  const int t = threadIdx.x;
  if (t < nb) for (int k = 0; k < 3; k++) ctr[3 * t + k] = rb[t].pos[k];
  for (int q = t; q < rigid_pair_count(nb); q += 64) {
    int i = 2;
    while (rigid_pair_index(i + 1, 1) <= q) i++;
    const int j = q - rigid_pair_index(i, 1) + 1;
    MprPair p;
    p.a = i; p.b = j; p.skip = (rb[i].scripted == 3 && rb[j].scripted == 3) ? 1 : 0; p.pad = 0;
    pairs[q] = p;
  }
}
// resolution: the bodies in LDS, one lane walks the sequential chain (as k_articulate does), vel / omega written back for bodies >= 1.
// n_hits: the length of the compacted list left in `hits` (read back by mpmhip_rigid_get_collisions).
__global__ __launch_bounds__(64) void k_rigid_resolve(RigidBodyDev *rb, int nb, const RigidCollision *__restrict__ cols, int n_pairs,
                                                      RigidCollision *__restrict__ hits, int *__restrict__ n_hits,
                                                      RigidContactParams cp, RigidSolveConfig cfg) {
  __shared__ JointBody sb[MAX_RIGID];
  __shared__ RigidCollision sc[MAX_RIGID_PAIRS];
  __shared__ int s_n;
  const int t = threadIdx.x;
  if (t < nb) {
    const RigidBodyDev &B = rb[t];
    JointBody &J = sb[t];
    for (int k = 0; k < 3; k++) { J.pos[k] = B.pos[k]; J.vel[k] = B.vel[k]; J.omega[k] = B.omega[k]; }
    for (int k = 0; k < 9; k++) { J.R[k] = B.R[k]; J.inv_I[k] = B.inv_I[k]; }
    J.inv_mass = B.inv_mass;
  }
  if (t == 0) {
    int n = 0;
    for (int q = 0; q < n_pairs && q < MAX_RIGID_PAIRS; q++)
      if (cols[q].hit) { sc[n] = cols[q]; hits[n] = cols[q]; n++; }
    s_n = n;
    *n_hits = n;
  }
  __syncthreads();
  if (t == 0) rigidify_resolve(sb, nb, cp, sc, s_n, cfg, nullptr);
  __syncthreads();
  if (t >= 1 && t < nb && s_n > 0) {
    for (int k = 0; k < 3; k++) { rb[t].vel[k] = sb[t].vel[k]; rb[t].omega[k] = sb[t].omega[k]; }
  }
}
#endif  // __HIPCC__

}  // namespace mpm
