// taichi_mpm_amd/csrc/rigid_api.h — host side of the CPIC rigid coupling (included by mpmhip.hip inside extern "C")
// Part of libmpmhip.  Device side: k_rigid.h (bodies, colored distance field, particle colours), k_rigid_transfer.h.
//
// A rigid body = triangles (mesh space) + pose + mass properties.  Creation (MPM::add_rigid_particle), the scripts' poses of a
// substep and the world-space mesh are host arithmetic and live in rigid_setup.h; here: the device arrays, uploads and launches.
// The rigid-body arithmetic itself
// (what an impulse does, how a script becomes a velocity) belongs to the absent taichi core; the conventions used here
// are those of the body the reference build is tested against (oracle/taichi_shim/taichi/dynamics/rigid_body_shim.h)
// and are restated in k_rigid.h.  Joints between bodies (MPM::articulate) are in k_joints.h; rigid-rigid collisions
// (MPM::rigidify, src/mpm.cpp:468, libccd's MPR) are in k_rigid_collide.h / rigid_collide_api.h, an opt-in pass — without it the
// Python layer warns when a scene has more than one body that could collide.

static int rigid_enable(mpmhip_ctx *c) {
  auto &R = c->rigid;
  if (R.enabled) return MPMHIP_OK;
  // bodies on a tiled ctx: every rank of the job holds ALL bodies and mpmhip_tiled_setup sizes the arena for their impulse rows
  // (tiled_plan.h), so they come before it; the callback path (mpmhip_set_halo) does not carry the rows
  if (c->tn.on) return fail(c, MPMHIP_EINVAL, "rigid bodies on a tiled job: add the bodies before mpmhip_tiled_setup, or set the job up again");
  if (c->T.n_boxes > 0) return fail(c, MPMHIP_EINVAL, "rigid bodies on a tiled ctx need the native plan (mpmhip_tiled_setup): the callback path (mpmhip_set_halo) does not carry the bodies' impulses");
  if (c->rigid.col.on && c->T.enabled) return fail(c, MPMHIP_EINVAL, "rigid_body_collision is not supported on a tiled (multi-GPU) ctx");
  if (c->async.enabled) return fail(c, MPMHIP_EINVAL, "rigid bodies are not supported with asynchronous stepping");
  hipError_t e = hipSuccess;
  auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  R.max_pages = (uint32_t)std::min<int64_t>((int64_t)c->NB, std::max<int64_t>(8192, (int64_t)c->P.max_blocks * 2));
  R.max_pages = (R.max_pages + CDF_POOLS - 1) / CDF_POOLS * CDF_POOLS;
  const int rpd[3] = {c->P.res[0] / 4 + 2, c->P.res[1] / 4 + 2, c->P.res[2] / 8 + 2};
  R.rpage_words = ((size_t)rpd[0] * rpd[1] * rpd[2] + 31) / 32;
  A(R.d_rb.alloc((size_t)MAX_RIGID));
  A(R.d_joints.alloc((size_t)MAX_JOINTS));
  A(R.cdf_slot.alloc((size_t)c->NB));
  A(R.cdf_page_key.alloc((size_t)R.max_pages));
  A(R.cdf_mind.alloc((size_t)R.max_pages * 64));
  A(R.cdf_tags.alloc((size_t)R.max_pages * 64));
  A(R.d_counters.alloc((size_t)CDF_POOLS + 4));  // [0, CDF_POOLS) pages handed out per sub-pool, [CDF_POOLS] cutting_counter,
                                                    // [CDF_POOLS + 1] length of d_rigid_list
  A(R.cdf_rpage.alloc(R.rpage_words));
  A(R.d_bnd.alloc((size_t)c->cap));
  A(R.d_blk_rigid.alloc((size_t)c->P.max_blocks + 1));
  A(R.d_rigid_list.alloc((size_t)c->P.max_blocks + 1));
  if (e != hipSuccess) return fail(c, MPMHIP_ENOMEM, "rigid coupling: device allocation failed: %s", hipGetErrorString(e));
  R.cdf.slot = R.cdf_slot; R.cdf.page_key = R.cdf_page_key; R.cdf.mind = R.cdf_mind; R.cdf.tags = R.cdf_tags; R.cdf.rpage = R.cdf_rpage;
  R.cdf.n_pages = R.d_counters; R.cdf.error = &c->cnt->error;
  R.cdf.nb_axis = 1 << c->P.kbits;
  R.cdf.max_pages = R.max_pages;
  R.cdf.pool_cap = R.max_pages / CDF_POOLS;
  for (int k = 0; k < 3; k++) R.cdf.rpd[k] = rpd[k];
  HIPCHK(c, hipMemset(R.d_rb, 0, sizeof(RigidBodyDev) * MAX_RIGID));
  {  // body 0, the background (RigidBody::set_as_background): at the origin, unrotated, immovable — joints may link to it
    RigidBodyDev G;
    memset(&G, 0, sizeof G);
    G.R[0] = G.R[4] = G.R[8] = 1.0f;
    G.q[0] = 1.0f;
    G.mass = 1.0f;
    HIPCHK(c, hipMemcpy(R.d_rb, &G, sizeof G, hipMemcpyHostToDevice));
  }
  HIPCHK(c, hipMemset(R.cdf.slot, 0xFF, sizeof(uint32_t) * (size_t)c->NB));
  HIPCHK(c, hipMemset(R.cdf.mind, 0xFF, sizeof(unsigned long long) * (size_t)R.max_pages * 64));
  HIPCHK(c, hipMemset(R.cdf.tags, 0, sizeof(uint32_t) * (size_t)R.max_pages * 64));
  HIPCHK(c, hipMemset(R.cdf.page_key, 0, sizeof(uint32_t) * (size_t)R.max_pages));
  HIPCHK(c, hipMemset(R.d_counters, 0, sizeof(uint32_t) * (CDF_POOLS + 4)));
  HIPCHK(c, hipMemset(R.cdf.rpage, 0, sizeof(uint32_t) * R.rpage_words));
  HIPCHK(c, hipMemset(R.d_bnd, 0, sizeof(BndRec) * (size_t)c->cap));
  HIPCHK(c, hipMemset(R.d_blk_rigid, 0, (size_t)c->P.max_blocks + 1));
  R.store.bodies.clear();
  R.store.bodies.emplace_back();  // body 0: the background (MPM::initialize, src/mpm.cpp:72-74); it has no surface
  R.store.bodies[0].mass = 1.0f;
  R.store.bodies[0].inertia[0] = R.store.bodies[0].inertia[4] = R.store.bodies[0].inertia[8] = 1.0f;  // set_as_background: inertia 1, inverse 0
  R.joints.clear();
  R.enabled = true;
  return MPMHIP_OK;
}

static RigidXfer rigid_xfer(mpmhip_ctx *c) {
  RigidXfer X;
  X.C = c->rigid.cdf; X.rb = c->rigid.d_rb; X.bnd = c->rigid.d_bnd; X.imp_rows = c->rigid.d_imp_rows;
  X.rigid_list = c->rigid.d_rigid_list; X.n_rigid = c->rigid.d_counters + CDF_POOLS + 1;
  X.rp_in = (const float4 *)c->rp.get();
  X.penalty = c->rigid.penalty; X.pushing_force = c->rigid.pushing_force;
  return X;
}
static inline bool rigid_active(const mpmhip_ctx *c) { return c->rigid.enabled && c->rigid.store.bodies.size() > 1; }  // has_rigid_body()

// rasterize_rigid_boundary: clear last substep's pages, then the boundary particles write colours and distances
static int do_rigid_rasterize(mpmhip_ctx *c) {
  auto &R = c->rigid;
  hipLaunchKernelGGL(k_cdf_clear, dim3(16, CDF_POOLS), dim3(256), 0, c->stream, R.cdf);
  HIPCHK(c, hipMemsetAsync(R.cdf.n_pages, 0, sizeof(uint32_t) * CDF_POOLS, c->stream));
  HIPCHK(c, hipMemsetAsync(R.cdf.rpage, 0, sizeof(uint32_t) * R.rpage_words, c->stream));
  if (R.n_smp) {
    hipLaunchKernelGGL(k_cdf_alloc, dim3(particle_grid(R.n_smp)), dim3(256), 0, c->stream, c->P, R.cdf, (const RigidBodyDev *)R.d_rb,
                       (const RigidSample *)R.d_smp, R.n_smp);
    hipLaunchKernelGGL(k_cdf_rasterize, dim3(particle_grid((int64_t)R.n_smp * 27)), dim3(256), 0, c->stream, c->P, R.cdf,
                       (const RigidBodyDev *)R.d_rb, (const RigidSample *)R.d_smp, (const float *)R.d_elems, R.n_smp);
  }
  return launch_check(c, "rasterize_rigid_boundary");
}
static int do_rigid_gather(mpmhip_ctx *c) {
  auto &R = c->rigid;
  hipLaunchKernelGGL(k_gather_cdf, dim3(8192), dim3(256), 0, c->stream, c->P, R.cdf, c->rg, R.d_bnd, R.d_counters + CDF_POOLS,
                     (const Counters *)c->cnt, (const uint32_t *)c->act_blk, (const uint32_t *)c->act_start, (const uint32_t *)c->perm, ++R.gather_epoch);
  return launch_check(c, "gather_cdf");
}
static int do_rigid_block_flags(mpmhip_ctx *c) {
  auto &R = c->rigid;
  HIPCHK(c, hipMemsetAsync(R.d_counters + CDF_POOLS + 1, 0, sizeof(uint32_t), c->stream));
  hipLaunchKernelGGL(k_blk_rigid, dim3(256), dim3(256), 0, c->stream, c->P, (const Counters *)c->cnt, (const uint32_t *)c->act_blk, R.cdf,
                     R.d_blk_rigid, c->act_start, R.d_rigid_list, R.d_counters + CDF_POOLS + 1);
  return launch_check(c, "rigid block flags");
}
// the impulse rows of the deterministic mode: allocated when the mode meets a body, one row per block of the block table
static int rigid_imp_rows(mpmhip_ctx *c) {
  auto &R = c->rigid;
  if (R.d_imp_rows && R.imp_rows_cap >= c->P.max_blocks) return MPMHIP_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (R.side) HIPCHK(c, hipStreamSynchronize(R.side));
  R.imp_rows_cap = 0;
  HIPCHK(c, R.d_imp_rows.alloc((size_t)c->P.max_blocks * IMP_ROW));
  R.imp_rows_cap = c->P.max_blocks;
  return MPMHIP_OK;
}
static int do_rigid_apply_tmp(mpmhip_ctx *c) {
  if (c->deterministic) {  // the rows the colour-aware kernel just wrote, summed in a fixed order and applied (k_rigid.h)
    hipLaunchKernelGGL(k_rigid_rows_apply, dim3((int)c->rigid.store.bodies.size() - 1), dim3(1024), 0, c->stream, c->P, (const Counters *)c->cnt,
                       (const uint8_t *)c->rigid.d_blk_rigid, (const float *)c->rigid.d_imp_rows, c->rigid.d_rb);
    return launch_check(c, "rigid apply_tmp_velocity (deterministic)");
  }
  hipLaunchKernelGGL(k_rigid_apply_tmp, dim3(1), dim3(64), 0, c->stream, c->rigid.d_rb, (int)c->rigid.store.bodies.size());
  return launch_check(c, "rigid apply_tmp_velocity");
}
// MPM<dim>::rigid_body_levelset_collision (src/mpm_rigid_body.cpp:347-387): the boundary particles in the reference's order
// (k_rigid.h), then the sequential impulse chain
static int do_rigid_ls_collision(mpmhip_ctx *c) {
  auto &R = c->rigid;
  const uint32_t n = R.n_smp;
  if (n == 0 || c->LS.n == 0) return MPMHIP_OK;
  if (R.ls_cap < n) {
    R.ls_tmp_bytes = 0;
    const size_t cap = (size_t)n + n / 4 + 1024;
    for (int k = 0; k < 2; k++) { HIPCHK(c, R.d_ls_keys[k].alloc(cap)); HIPCHK(c, R.d_ls_vals[k].alloc(cap)); }
    size_t bytes = 0;
    HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, R.d_ls_keys[0].get(), R.d_ls_keys[1].get(), R.d_ls_vals[0].get(), R.d_ls_vals[1].get(), (int)cap, 0, 64, c->stream));
    HIPCHK(c, R.d_ls_tmp.alloc(bytes));
    R.ls_tmp_bytes = bytes;
    R.ls_cap = (uint32_t)cap;
  }
  if (R.n_ranked < n) {  // boundary particles added since: behind everybody else, in creation order (appended to `particles`)
    std::vector<uint32_t> rk(n);
    // (the ctx stream does not synchronise with the blocking copies below: a collision kernel of an earlier substep may still
    // be writing the ranks)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (R.n_ranked) HIPCHK(c, hipMemcpy(rk.data(), R.d_smp_rank, sizeof(uint32_t) * R.n_ranked, hipMemcpyDeviceToHost));
    for (uint32_t s = R.n_ranked; s < n; s++) rk[s] = s;
    HIPCHK(c, R.d_smp_rank.alloc((size_t)n + n / 4 + 1024));
    HIPCHK(c, hipMemcpy(R.d_smp_rank, rk.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    R.n_ranked = n;
  }
  c->P.t = c->t;
  hipLaunchKernelGGL(k_rigid_ls_keys, dim3(particle_grid(n)), dim3(256), 0, c->stream, c->P, (const RigidBodyDev *)R.d_rb,
                     (const RigidSample *)R.d_smp, n, (const uint32_t *)R.d_smp_rank, R.d_ls_keys[0], R.d_ls_vals[0]);
  size_t bytes = R.ls_tmp_bytes;
  HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(R.d_ls_tmp, bytes, R.d_ls_keys[0].get(), R.d_ls_keys[1].get(), R.d_ls_vals[0].get(), R.d_ls_vals[1].get(), (int)n, 0, 64, c->stream));
  RigidRestitution rest;
  memset(&rest, 0, sizeof rest);
  for (size_t b = 1; b < R.store.bodies.size(); b++) rest.e[b] = R.store.bodies[b].cfg.restitution;
  hipLaunchKernelGGL(k_rigid_ls_collide, dim3(1), dim3(1024), 0, c->stream, c->P, (const LevelSetDev *)c->d_LS, R.d_rb, (int)R.store.bodies.size(),
                     (const RigidSample *)R.d_smp, (const uint32_t *)R.d_ls_vals[1], n, R.d_smp_rank, rest);
  return launch_check(c, "rigid_body_levelset_collision");
}
// advect_rigid_bodies(dt) at current_t = c->t: scripts are evaluated here, on the host, for this one substep
static int do_rigid_advect(mpmhip_ctx *c, float dt) {
  auto &R = c->rigid;
  const RigidSteps st = rigid_setup::scripted_steps<3>(R.store, c->t, dt);
  hipLaunchKernelGGL(k_rigid_advect, dim3(1), dim3(64), 0, c->stream, R.d_rb, (int)R.store.bodies.size(), st, dt, c->P.g[0], c->P.g[1], c->P.g[2]);
  return launch_check(c, "advect_rigid_bodies");
}
// what substep() does with rigid bodies between the sort and P2G (src/mpm.cpp:466-472, 506-508)
// MPM::articulate (src/mpm.h:278-319): between the sort and rasterize_rigid_boundary (src/mpm.cpp:466-471)
static int do_rigid_articulate(mpmhip_ctx *c, float dt) {
  auto &R = c->rigid;
  if (R.joints.empty()) return MPMHIP_OK;
  hipLaunchKernelGGL(k_articulate, dim3(1), dim3(64), 0, c->stream, R.d_rb, (int)R.store.bodies.size(), (const JointDev *)R.d_joints,
                     (int)R.joints.size(), dt, R.joint_iterations);
  return launch_check(c, "articulate");
}
// In two halves: (a) the joints and the colored distance field depend on the bodies alone — substep_begin runs them on the
// side stream NEXT TO the particle sort; (b) the particles' colours and the block flags need both the field and the sort.
static int do_rigid_pre_a(mpmhip_ctx *c, hipStream_t on) {
  hipStream_t keep = c->stream;
  c->stream = on;  // (the launch helpers below enqueue on the ctx's stream)
  int rc;
  if (!(rc = do_rigid_articulate(c, c->P.dt))) rc = do_rigid_rasterize(c);
  c->stream = keep;
  return rc;
}
static int do_rigid_pre_b(mpmhip_ctx *c) {
  int rc;
  if ((rc = do_rigid_gather(c)) || (rc = do_rigid_block_flags(c))) return rc;
  return MPMHIP_OK;
}

int mpmhip_set_rigid_levelset_collision(mpmhip_ctx *c, int32_t enabled) {
  if (!c) return MPMHIP_EINVAL;
  if (enabled && c->LS.sdf.phi0)
    return fail(c, MPMHIP_EINVAL, "rigid_body_levelset_collision is not supported with a sampled level set");
  c->rigid.ls_collision = enabled != 0;
  return MPMHIP_OK;
}

int mpmhip_set_rigid_coupling(mpmhip_ctx *c, float penalty, float pushing_force) {
  if (!c) return MPMHIP_EINVAL;
  c->rigid.penalty = penalty;
  c->rigid.pushing_force = pushing_force;
  return MPMHIP_OK;
}

int mpmhip_add_rigid_body(mpmhip_ctx *c, const mpmhip_rigid_config *cfg, int64_t n_triangles, const float *triangles) {
  if (!c || !cfg || !triangles || n_triangles <= 0) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "add_rigid_body inside a substep");
  if (c->tn.on) return fail(c, MPMHIP_EINVAL, "rigid bodies on a tiled job: add the bodies before mpmhip_tiled_setup, or set the job up again");
  if (int rc = rigid_enable(c)) return rc;
  auto &R = c->rigid;
  if ((int)R.store.bodies.size() >= MAX_RIGID) return fail(c, MPMHIP_ECAPACITY, "at most %d rigid bodies (2 colour bits each in a 24-bit word)", MAX_RIGID - 1);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  RigidBodyDev D;
  int32_t allocated = 0, body = (int32_t)R.store.bodies.size();
  if (const char *why = rigid_setup::add_body<3>(*cfg, n_triangles, triangles, c->P.dx, c->P.idx, c->P.res, c->t, c->next_pid, R.store, D, allocated))
    return fail(c, MPMHIP_EINVAL, "%s", why);
  c->next_pid += allocated;  // later material particles are numbered behind the boundary particles
  // (re)upload samples and elements
  HIPCHK(c, R.d_smp.alloc(std::max<size_t>(R.store.h_smp.size(), 1)));
  HIPCHK(c, R.d_elems.alloc(std::max<size_t>(R.store.h_elems.size(), 9)));
  if (!R.store.h_smp.empty()) HIPCHK(c, hipMemcpy(R.d_smp, R.store.h_smp.data(), sizeof(RigidSample) * R.store.h_smp.size(), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(R.d_elems, R.store.h_elems.data(), sizeof(float) * R.store.h_elems.size(), hipMemcpyHostToDevice));
  R.n_smp = (uint32_t)R.store.h_smp.size();
  HIPCHK(c, hipMemcpy(R.d_rb + body, &D, sizeof D, hipMemcpyHostToDevice));
  return body;
}

int32_t mpmhip_num_rigid_bodies(const mpmhip_ctx *c) { return c && c->rigid.enabled ? (int32_t)c->rigid.store.bodies.size() : 1; }

// out[33]: position 3, quaternion (w, x, y, z) 4, velocity 3, angular velocity 3, mass, inv_mass, inertia 9 (body frame,
// row-major), inv_inertia 9 — the fields of RigidBody the coupling reads
int mpmhip_rigid_get_state(mpmhip_ctx *c, int32_t id, float *out) {
  if (!c || !out) return MPMHIP_EINVAL;
  if (!c->rigid.enabled || id < 1 || id >= (int)c->rigid.store.bodies.size()) return fail(c, MPMHIP_EINVAL, "no rigid body %d", id);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  RigidBodyDev D;
  HIPCHK(c, hipMemcpy(&D, c->rigid.d_rb + id, sizeof D, hipMemcpyDeviceToHost));
  int k = 0;
  for (int i = 0; i < 3; i++) out[k++] = D.pos[i];
  for (int i = 0; i < 4; i++) out[k++] = D.q[i];
  for (int i = 0; i < 3; i++) out[k++] = D.vel[i];
  for (int i = 0; i < 3; i++) out[k++] = D.omega[i];
  out[k++] = D.mass; out[k++] = D.inv_mass;
  for (int i = 0; i < 9; i++) out[k++] = c->rigid.store.bodies[id].inertia[i];
  for (int i = 0; i < 9; i++) out[k++] = D.inv_I[i];
  return MPMHIP_OK;
}
// a digest of the bodies as this ctx holds them: the device records of all bodies (pose, velocities, mass properties, pending
// impulses), the numeric part of their configs, the boundary particles with their creation ids, the elements, the joints and the
// coupling's settings — two 64-bit FNV-1a sums from different offsets.  The ranks of a tiled job, which all hold all bodies, compare
// digests instead of shipping records (tiled.py).  A ctx without bodies: the digest of nothing.
int mpmhip_rigid_digest(mpmhip_ctx *c, uint64_t out[2]) {
  if (!c || !out) return MPMHIP_EINVAL;
  uint64_t h[2] = {0xcbf29ce484222325ull, 0x84222325cbf29ce4ull};
  auto eat = [&](const void *p, size_t n) {
    const uint8_t *b = static_cast<const uint8_t *>(p);
    for (size_t i = 0; i < n; i++) {
      h[0] = (h[0] ^ b[i]) * 0x100000001b3ull;
      h[1] = (h[1] ^ (uint64_t)(b[i] + 0x9e)) * 0x100000001b3ull;
    }
  };
  auto &R = c->rigid;
  const int32_t nb = rigid_active(c) ? (int32_t)R.store.bodies.size() : 1;
  eat(&nb, sizeof nb);
  if (nb > 1) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<RigidBodyDev> hb((size_t)nb);
    HIPCHK(c, hipMemcpy(hb.data(), R.d_rb, sizeof(RigidBodyDev) * (size_t)nb, hipMemcpyDeviceToHost));
    static_assert(sizeof(RigidBodyDev) % 4 == 0 && sizeof(RigidSample) == 20 && sizeof(JointDev) % 4 == 0, "records without padding");
    eat(hb.data(), sizeof(RigidBodyDev) * (size_t)nb);
    for (int b = 1; b < nb; b++) {
      const auto &H = R.store.bodies[(size_t)b];
      const int32_t flags[4] = {H.cfg.codimensional, H.cfg.scripted_position ? 1 : 0, H.cfg.scripted_rotation ? 1 : 0, (int32_t)H.n_samples};
      eat(flags, sizeof flags);
      eat(H.cfg.friction, sizeof H.cfg.friction);
      eat(&H.cfg.restitution, sizeof H.cfg.restitution);
      eat(H.inertia, sizeof H.inertia);
    }
    eat(R.store.h_smp.data(), sizeof(RigidSample) * R.store.h_smp.size());
    eat(R.store.h_smp_id.data(), sizeof(int32_t) * R.store.h_smp_id.size());
    eat(R.store.h_elems.data(), sizeof(float) * R.store.h_elems.size());
    const int32_t nj = (int32_t)R.joints.size();
    eat(&nj, sizeof nj);
    eat(R.joints.data(), sizeof(JointDev) * R.joints.size());
    const float k[2] = {R.penalty, R.pushing_force};
    const int32_t s[2] = {R.ls_collision ? 1 : 0, R.joint_iterations};
    eat(k, sizeof k);
    eat(s, sizeof s);
  }
  out[0] = h[0]; out[1] = h[1];
  return MPMHIP_OK;
}
int mpmhip_rigid_set_velocity(mpmhip_ctx *c, int32_t id, const float *v, const float *w) {
  if (!c) return MPMHIP_EINVAL;
  if (!c->rigid.enabled || id < 1 || id >= (int)c->rigid.store.bodies.size()) return fail(c, MPMHIP_EINVAL, "no rigid body %d", id);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  RigidBodyDev D;
  HIPCHK(c, hipMemcpy(&D, c->rigid.d_rb + id, sizeof D, hipMemcpyDeviceToHost));
  for (int k = 0; k < 3; k++) { if (v) D.vel[k] = v[k]; if (w) D.omega[k] = w[k]; }
  HIPCHK(c, hipMemcpy(c->rigid.d_rb + id, &D, sizeof D, hipMemcpyHostToDevice));
  return MPMHIP_OK;
}
// boundary particles of body id (id < 0: all): world position, body-frame offset, body index.  Returns the count.
int64_t mpmhip_rigid_get_samples(mpmhip_ctx *c, int32_t id, int64_t cap, float *pos, float *offset, int32_t *body) {
  if (!c) return MPMHIP_EINVAL;
  if (!c->rigid.enabled) return 0;
  if (hipSetDevice(c->device) != hipSuccess) return MPMHIP_EHIP;
  auto &R = c->rigid;
  std::vector<float> w((size_t)R.n_smp * 3);
  if (R.n_smp && pos) {
    DevBuf<float> d;
    HIPCHK(c, d.alloc((size_t)R.n_smp * 3));
    hipLaunchKernelGGL(k_rigid_sample_positions, dim3(particle_grid(R.n_smp)), dim3(256), 0, c->stream, (const RigidBodyDev *)R.d_rb,
                       (const RigidSample *)R.d_smp, R.n_smp, d);
    HIPCHK(c, hipMemcpyAsync(w.data(), d, sizeof(float) * w.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  int64_t n = 0;
  for (size_t s = 0; s < R.store.h_smp.size(); s++) {
    if (id >= 0 && R.store.h_smp[s].body != id) continue;
    if (n < cap) {
      for (int k = 0; k < 3; k++) { if (pos) pos[3 * n + k] = w[3 * s + k]; if (offset) offset[3 * n + k] = R.store.h_smp[s].off[k]; }
      if (body) body[n] = R.store.h_smp[s].body;
    }
    n++;
  }
  return n;
}

// the body's triangles in world space (get_mesh_to_world applied to mesh->elements): what write_rigid_body puts into
// frame_directory/rigid_%03d_%04d.obj next to every .bgeo frame (src/visualize.cpp:102-154, src/mpm.h:333-343).
// out: 9 floats per triangle; returns the body's triangle count.
int64_t mpmhip_rigid_get_mesh(mpmhip_ctx *c, int32_t id, int64_t cap_triangles, float *out) {
  if (!c) return MPMHIP_EINVAL;
  if (!c->rigid.enabled || id < 1 || id >= (int)c->rigid.store.bodies.size()) return fail(c, MPMHIP_EINVAL, "no rigid body %d", id);
  if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return MPMHIP_EHIP;
  auto &R = c->rigid;
  RigidBodyDev D;
  HIPCHK(c, hipMemcpy(&D, R.d_rb + id, sizeof D, hipMemcpyDeviceToHost));
  return rigid_setup::world_elements<3>(R.store, id, D, cap_triangles, out);
}

// phase-level entry points (parity tests; substep() runs them itself)
int mpmhip_rasterize_rigid_boundary(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (!rigid_active(c)) return MPMHIP_OK;
  return do_rigid_rasterize(c);
}
int mpmhip_gather_cdf(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (!rigid_active(c)) return MPMHIP_OK;
  int rc = need_sorted(c, "gather_cdf");
  if (rc || (rc = do_rigid_gather(c))) return rc;
  return do_rigid_block_flags(c);
}
// general_action("add_articulation") (src/mpm.cpp:923-933): the joint's initialize() on the bodies' CURRENT poses
int mpmhip_add_articulation(mpmhip_ctx *c, const mpmhip_joint_config *cfg) {
  if (!c || !cfg) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  auto &R = c->rigid;
  const int nb = R.enabled ? (int)R.store.bodies.size() : 0;
  if (cfg->obj0 < 1 || cfg->obj0 >= nb) return fail(c, MPMHIP_EINVAL, "add_articulation: obj0 = %d is not a rigid body of this simulation", cfg->obj0);
  if (cfg->obj1 < 0 || cfg->obj1 >= nb) return fail(c, MPMHIP_EINVAL, "add_articulation: obj1 = %d is not a rigid body of this simulation", cfg->obj1);
  if (cfg->type < JOINT_ROTATION || cfg->type > JOINT_STEPPER) return fail(c, MPMHIP_EINVAL, "add_articulation: unknown type %d", cfg->type);
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "add_articulation inside a substep");
  if ((int)R.joints.size() >= MAX_JOINTS) return fail(c, MPMHIP_ECAPACITY, "at most %d articulations", MAX_JOINTS);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  JointBody jb[2];
  const int ids[2] = {cfg->obj0, cfg->obj1};
  for (int i = 0; i < 2; i++) {
    RigidBodyDev D;
    HIPCHK(c, hipMemcpy(&D, R.d_rb + ids[i], sizeof D, hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; k++) { jb[i].pos[k] = D.pos[k]; jb[i].vel[k] = D.vel[k]; jb[i].omega[k] = D.omega[k]; }
    for (int k = 0; k < 9; k++) { jb[i].R[k] = D.R[k]; jb[i].inv_I[k] = D.inv_I[k]; }
    jb[i].inv_mass = D.inv_mass;
  }
  JointConfig jc;
  jc.type = cfg->type; jc.obj0 = cfg->obj0; jc.obj1 = cfg->obj1; jc.has_offset1 = cfg->has_offset1; jc.has_target = cfg->has_target_distance;
  for (int k = 0; k < 3; k++) { jc.offset0[k] = cfg->offset0[k]; jc.offset1[k] = cfg->offset1[k]; jc.axis[k] = cfg->axis[k]; }
  jc.target_distance = cfg->target_distance; jc.penalty = cfg->penalty; jc.axis_length = cfg->axis_length;
  jc.power = cfg->power; jc.angular_velocity = cfg->angular_velocity;
  JointDev J;
  if (const char *why = joint_init(J, jc, jb[0], jb[1], R.store.bodies[cfg->obj0].inertia, R.store.bodies[cfg->obj1].inertia))
    return fail(c, MPMHIP_EINVAL, "add_articulation: %s", why);
  R.joints.push_back(J);
  HIPCHK(c, hipMemcpy(R.d_joints, R.joints.data(), sizeof(JointDev) * R.joints.size(), hipMemcpyHostToDevice));
  return MPMHIP_OK;
}
int32_t mpmhip_num_articulations(const mpmhip_ctx *c) { return c ? (int32_t)c->rigid.joints.size() : 0; }
int mpmhip_set_articulation_iterations(mpmhip_ctx *c, int32_t n) {
  if (!c || n < 0) return MPMHIP_EINVAL;
  c->rigid.joint_iterations = n;
  return MPMHIP_OK;
}
int mpmhip_articulate(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->rigid.enabled) return MPMHIP_OK;
  return do_rigid_articulate(c, c->P.dt);
}
int mpmhip_advect_rigid_bodies(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (!rigid_active(c)) return MPMHIP_OK;
  return do_rigid_advect(c, c->P.dt);
}
// dense (res+1)^3 views of the colored distance field: GridState::states (24 colour bits | body id + 1 << 24) and distance
int mpmhip_download_cdf(mpmhip_ctx *c, uint32_t *states, float *distance) {
  if (!c || !states || !distance) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nodes = (size_t)(c->P.res[0] + 1) * (c->P.res[1] + 1) * (c->P.res[2] + 1);
  memset(states, 0, nodes * 4);
  memset(distance, 0, nodes * 4);
  if (!c->rigid.enabled) return MPMHIP_OK;
  DevBuf<uint32_t> ds;
  DevBuf<float> dd;
  HIPCHK(c, ds.alloc(nodes));
  HIPCHK(c, dd.alloc(nodes));
  HIPCHK(c, hipMemsetAsync(ds, 0, nodes * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(dd, 0, nodes * 4, c->stream));
  hipLaunchKernelGGL(k_cdf_dense, dim3(1024), dim3(256), 0, c->stream, c->P, c->rigid.cdf, ds, dd);
  HIPCHK(c, hipMemcpyAsync(states, ds, nodes * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(distance, dd, nodes * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MPMHIP_OK;
}
// what gather_cdf left for every live particle, in slot order (like mpmhip_download): boundary_normal 3, boundary_distance,
// near_boundary (0 / 1) — 5 floats per particle
int64_t mpmhip_download_boundary(mpmhip_ctx *c, float *out, int64_t n_capacity) {
  if (!c || !out) return MPMHIP_EINVAL;
  if (hipSetDevice(c->device) != hipSuccess) return MPMHIP_EHIP;
  std::vector<RecG> hg;
  int rc = fetch_records(c, hg, nullptr, nullptr);
  if (rc) return rc;
  std::vector<BndRec> hb(hg.size());
  if (c->rigid.enabled && !hg.empty()) HIPCHK(c, hipMemcpy(hb.data(), c->rigid.d_bnd, sizeof(BndRec) * hg.size(), hipMemcpyDeviceToHost));
  else memset(hb.data(), 0, sizeof(BndRec) * hb.size());
  int64_t m = 0;
  for (size_t i = 0; i < hg.size(); i++) {
    if (hg[i].pid < 0) continue;
    if (m >= n_capacity) return fail(c, MPMHIP_ECAPACITY, "download buffer too small");
    const bool fresh = hb[i].epoch == c->rigid.gather_epoch;  // (particles away from every body are not visited: zeros, as the reference leaves them)
    for (int k = 0; k < 3; k++) out[5 * m + k] = fresh ? hb[i].n[k] : 0.0f;
    out[5 * m + 3] = fresh ? hb[i].dist : 0.0f;
    out[5 * m + 4] = fresh ? (float)hb[i].near : 0.0f;
    m++;
  }
  return m;
}
