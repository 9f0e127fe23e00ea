// taichi_mpm_amd/csrc/rigid_collide_api.h — host side of the rigid-rigid collisions (included by mpmhip.hip inside extern "C",
// behind rigid_api.h).  Device side and the arithmetic: k_rigid_collide.h.
//
// MPM::rigidify(dt) (src/mpm_rigid_body.cpp:306-345) as four launches on the ctx stream, at the head of the rigid block of a
// substep (src/mpm.cpp:466-472: rigidify, articulate, rasterize_rigid_boundary), ahead of the fork of MPMHIP_RIGID_CONCURRENT:
//   k_rigid_pairs      the pair table (i > j >= 1, fully scripted pairs skipped) and the bodies' centres
//   k_rigid_hull_pose  r = R v, p = r + pos of every hull vertex
//   k_rigid_mpr        one workgroup per pair: MPR, the collision written at the pair's canonical index
//   k_rigid_resolve    the hits compacted in (i, j) order, the sequential impulses, vel / omega written back
// The hull vertices of a body are its triangles' vertices in element order: the array the rasterisation already keeps on the
// device (RigidState::d_elems, three vertices of three floats per triangle).  What the pass adds is allocated by its first
// run, so a ctx that never enables it owns nothing more than before.

static int rigid_collide_prepare(mpmhip_ctx *c) {
  auto &R = c->rigid;
  auto &K = R.col;
  const size_t nv = R.store.h_elems.size() / 3;
  const int nb = (int)R.store.bodies.size();
  if (K.n_verts == nv && K.n_bodies == nb && K.d_cols) return MPMHIP_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<int> body(nv), first(MAX_RIGID, 0), count(MAX_RIGID, 0);
  for (int b = 1; b < nb; b++) {
    first[b] = (int)(R.store.bodies[b].first_elem * 3);
    count[b] = (int)(R.store.bodies[b].n_elems * 3);
    for (int v = 0; v < count[b]; v++) body[(size_t)first[b] + v] = b;
  }
  hipError_t e = hipSuccess;
  auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  A(K.d_body.alloc(std::max<size_t>(nv, 1)));
  A(K.d_r.alloc(std::max<size_t>(nv, 1)));
  A(K.d_p.alloc(std::max<size_t>(nv, 1)));
  A(K.d_first.alloc(MAX_RIGID));
  A(K.d_count.alloc(MAX_RIGID));
  A(K.d_ctr.alloc(3 * MAX_RIGID));
  A(K.d_pairs.alloc(MAX_RIGID_PAIRS));
  A(K.d_cols.alloc(MAX_RIGID_PAIRS));
  A(K.d_hits.alloc(MAX_RIGID_PAIRS));
  A(K.d_nhits.alloc(1));
  if (e != hipSuccess) return fail(c, MPMHIP_ENOMEM, "rigid-rigid collisions: device allocation failed: %s", hipGetErrorString(e));
  if (nv) HIPCHK(c, hipMemcpy(K.d_body, body.data(), sizeof(int) * nv, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(K.d_first, first.data(), sizeof(int) * MAX_RIGID, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(K.d_count, count.data(), sizeof(int) * MAX_RIGID, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemset(K.d_nhits, 0, sizeof(int)));
  K.n_verts = nv;
  K.n_bodies = nb;
  return MPMHIP_OK;
}
// at least two bodies beside the background, and the pass switched on
static inline bool rigid_collide_active(const mpmhip_ctx *c) { return c->rigid.enabled && c->rigid.col.on && c->rigid.store.bodies.size() > 2; }

static int do_rigid_rigidify(mpmhip_ctx *c, float dt) {
  if (!rigid_collide_active(c)) return MPMHIP_OK;
  if (int rc = rigid_collide_prepare(c)) return rc;
  auto &R = c->rigid;
  auto &K = R.col;
  const int nb = (int)R.store.bodies.size(), np = rigid_pair_count(nb), nv = (int)K.n_verts;
  hipLaunchKernelGGL(k_rigid_pairs, dim3(1), dim3(64), 0, c->stream, (const RigidBodyDev *)R.d_rb, nb, K.d_pairs.get(), K.d_ctr.get());
  hipLaunchKernelGGL(k_rigid_hull_pose, dim3(std::min(particle_grid(nv), 1024)), dim3(256), 0, c->stream, (const RigidBodyDev *)R.d_rb,
                     (const float *)R.d_elems, (const int *)K.d_body, nv, K.d_r.get(), K.d_p.get());
  hipLaunchKernelGGL(k_rigid_mpr, dim3(np), dim3(MPR_WG), 0, c->stream, (const MprPair *)K.d_pairs, (const int *)K.d_first,
                     (const int *)K.d_count, (const float *)K.d_ctr, (const float4 *)K.d_r, (const float4 *)K.d_p, K.d_cols.get(),
                     &c->cnt->error);
  RigidContactParams cp;
  memset(&cp, 0, sizeof cp);
  for (int b = 1; b < nb; b++) { cp.fric[b] = R.store.bodies[b].cfg.friction[0]; cp.rest[b] = R.store.bodies[b].cfg.restitution; }
  const RigidSolveConfig cfg{K.iterations, K.position_iterations ? 1 : 0, K.penalty, dt};
  hipLaunchKernelGGL(k_rigid_resolve, dim3(1), dim3(64), 0, c->stream, R.d_rb.get(), nb, (const RigidCollision *)K.d_cols, np,
                     K.d_hits.get(), K.d_nhits.get(), cp, cfg);
  return launch_check(c, "rigidify");
}

int mpmhip_set_rigid_collision(mpmhip_ctx *c, int32_t enabled, int32_t iterations, float rigid_penalty, int32_t position_iterations) {
  if (!c) return MPMHIP_EINVAL;
  if (iterations < 0) return fail(c, MPMHIP_EINVAL, "rigid_body_iterations = %d: must not be negative", iterations);
  if (enabled && c->T.enabled) return fail(c, MPMHIP_EINVAL, "rigid_body_collision is not supported on a tiled (multi-GPU) ctx: the bodies of a job meet no other body");
  if (enabled && c->async.enabled) return fail(c, MPMHIP_EINVAL, "rigid_body_collision: asynchronous stepping has no rigid bodies");
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "set_rigid_collision inside a substep");
  auto &K = c->rigid.col;
  K.on = enabled != 0;
  K.iterations = iterations;
  K.penalty = rigid_penalty;
  K.position_iterations = position_iterations != 0;
  return MPMHIP_OK;
}

int mpmhip_rigidify(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "rigidify inside a substep");
  return do_rigid_rigidify(c, c->P.dt);
}

// the collision list the last rigidify resolved, in (i, j) order: 9 floats per row — body i, body j, depth, dir[3], pos[3].
// Returns the length of the list (rows beyond cap are not written).
int64_t mpmhip_rigid_get_collisions(mpmhip_ctx *c, int64_t cap, float *out) {
  if (!c) return MPMHIP_EINVAL;
  auto &K = c->rigid.col;
  if (!c->rigid.enabled || !K.d_nhits) return 0;
  if (hipSetDevice(c->device) != hipSuccess) return MPMHIP_EHIP;
  int n = 0;
  HIPCHK(c, hipMemcpyAsync(&n, K.d_nhits, sizeof n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n < 0 || n > MAX_RIGID_PAIRS) return fail(c, MPMHIP_EHIP, "rigid collisions: the list length %d is out of range", n);
  std::vector<RigidCollision> h((size_t)n);
  if (n) HIPCHK(c, hipMemcpy(h.data(), K.d_hits, sizeof(RigidCollision) * n, hipMemcpyDeviceToHost));
  for (int q = 0; q < n && q < cap && out; q++) {
    float *o = out + 9 * q;
    o[0] = (float)h[q].i; o[1] = (float)h[q].j; o[2] = h[q].depth;
    for (int k = 0; k < 3; k++) { o[3 + k] = h[q].dir[k]; o[6 + k] = h[q].pos[k]; }
  }
  return n;
}

// the hull vertices of body id as the support mapping walks them: body frame (scaled, recentred), three per triangle in element
// order.  out: 3 floats per vertex; returns the body's vertex count.
int64_t mpmhip_rigid_get_hull(mpmhip_ctx *c, int32_t id, int64_t cap_vertices, float *out) {
  if (!c) return MPMHIP_EINVAL;
  if (!c->rigid.enabled || id < 1 || id >= (int)c->rigid.store.bodies.size()) return fail(c, MPMHIP_EINVAL, "no rigid body %d", id);
  const auto &B = c->rigid.store.bodies[id];
  const int64_t n = B.n_elems * 3;
  if (out) memcpy(out, &c->rigid.store.h_elems[(size_t)B.first_elem * 9], sizeof(float) * 3 * (size_t)std::min<int64_t>(n, std::max<int64_t>(cap_vertices, 0)));
  return n;
}

// the detection kernel alone on raw vertex clouds (no ctx): pair q is cloud 2q against cloud 2q + 1 — see include/mpmhip.h
int mpmhip_rigid_mpr_test(int32_t device, int32_t n_pairs, const float *verts, const int64_t *offsets, const float *rotations,
                          const float *centres, float *out) {
  if (n_pairs <= 0 || !verts || !offsets || !centres || !out) return fail(nullptr, MPMHIP_EINVAL, "rigid_mpr_test: missing argument");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
    return fail(nullptr, MPMHIP_EINVAL, "rigid_mpr_test: device %d is not one of the %d visible GPUs", device, n_dev);
  const int nc = 2 * n_pairs;
  for (int k = 0; k < nc; k++)
    if (offsets[k + 1] <= offsets[k] || offsets[k] < 0 || offsets[k + 1] > (1ll << 30))
      return fail(nullptr, MPMHIP_EINVAL, "rigid_mpr_test: cloud %d is empty or its offsets are not ascending", k);
  if (offsets[0] != 0) return fail(nullptr, MPMHIP_EINVAL, "rigid_mpr_test: offsets[0] must be 0");
  HIPCHK(nullptr, hipSetDevice(device));
  const size_t nv = (size_t)offsets[nc];
  std::vector<int> cloud(nv), first(nc), count(nc);
  std::vector<MprPair> pairs(n_pairs);
  for (int k = 0; k < nc; k++) {
    first[k] = (int)offsets[k];
    count[k] = (int)(offsets[k + 1] - offsets[k]);
    for (int64_t v = offsets[k]; v < offsets[k + 1]; v++) cloud[(size_t)v] = k;
  }
  for (int q = 0; q < n_pairs; q++) pairs[q] = MprPair{2 * q, 2 * q + 1, 0, 0};
  DevBuf<float> d_verts, d_rot, d_ctr;
  DevBuf<int> d_cloud, d_first, d_count;
  DevBuf<float4> d_r, d_p;
  DevBuf<MprPair> d_pairs;
  DevBuf<RigidCollision> d_cols;
  DevBuf<uint32_t> d_err;
  hipError_t e = hipSuccess;
  auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  A(d_verts.alloc(3 * nv)); A(d_ctr.alloc(3 * (size_t)nc)); A(d_cloud.alloc(nv)); A(d_first.alloc(nc)); A(d_count.alloc(nc));
  A(d_r.alloc(nv)); A(d_p.alloc(nv)); A(d_pairs.alloc(n_pairs)); A(d_cols.alloc(n_pairs)); A(d_err.alloc(1));
  if (rotations) A(d_rot.alloc(9 * (size_t)nc));
  if (e != hipSuccess) return fail(nullptr, MPMHIP_ENOMEM, "rigid_mpr_test: device allocation failed: %s", hipGetErrorString(e));
  HIPCHK(nullptr, hipMemcpy(d_verts, verts, sizeof(float) * 3 * nv, hipMemcpyHostToDevice));
  HIPCHK(nullptr, hipMemcpy(d_ctr, centres, sizeof(float) * 3 * nc, hipMemcpyHostToDevice));
  if (rotations) HIPCHK(nullptr, hipMemcpy(d_rot, rotations, sizeof(float) * 9 * nc, hipMemcpyHostToDevice));
  HIPCHK(nullptr, hipMemcpy(d_cloud, cloud.data(), sizeof(int) * nv, hipMemcpyHostToDevice));
  HIPCHK(nullptr, hipMemcpy(d_first, first.data(), sizeof(int) * nc, hipMemcpyHostToDevice));
  HIPCHK(nullptr, hipMemcpy(d_count, count.data(), sizeof(int) * nc, hipMemcpyHostToDevice));
  HIPCHK(nullptr, hipMemcpy(d_pairs, pairs.data(), sizeof(MprPair) * n_pairs, hipMemcpyHostToDevice));
  HIPCHK(nullptr, hipMemset(d_err, 0, sizeof(uint32_t)));
  hipLaunchKernelGGL(k_rigid_cloud_pose, dim3((unsigned)std::min<size_t>((nv + 255) / 256, 1024)), dim3(256), 0, 0, (const float *)d_verts,
                     (const int *)d_cloud, rotations ? (const float *)d_rot : (const float *)nullptr, (const float *)d_ctr, (int)nv,
                     d_r.get(), d_p.get());
  hipLaunchKernelGGL(k_rigid_mpr, dim3(n_pairs), dim3(MPR_WG), 0, 0, (const MprPair *)d_pairs, (const int *)d_first, (const int *)d_count,
                     (const float *)d_ctr, (const float4 *)d_r, (const float4 *)d_p, d_cols.get(), d_err.get());
  HIPCHK(nullptr, hipGetLastError());
  HIPCHK(nullptr, hipDeviceSynchronize());
  std::vector<RigidCollision> h(n_pairs);
  uint32_t err = 0;
  HIPCHK(nullptr, hipMemcpy(h.data(), d_cols, sizeof(RigidCollision) * n_pairs, hipMemcpyDeviceToHost));
  HIPCHK(nullptr, hipMemcpy(&err, d_err, sizeof err, hipMemcpyDeviceToHost));
  for (int q = 0; q < n_pairs; q++) {
    float *o = out + 9 * q;
    o[0] = (float)h[q].hit; o[1] = h[q].depth;
    for (int k = 0; k < 3; k++) { o[2 + k] = h[q].dir[k]; o[5 + k] = h[q].pos[k]; }
    o[8] = (float)h[q].calls;
  }
  if (err & RIGID_MPR_ERROR_BIT) return fail(nullptr, MPMHIP_EHIP, "rigid_mpr_test: a loop bound of the MPR expired (k_rigid_collide.h)");
  return MPMHIP_OK;
}
