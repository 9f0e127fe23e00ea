// taichi_mpm_amd/csrc/snapshot_api.h — whole-state save / load of the three kinds of simulation (included by mpmhip.hip inside
// extern "C", behind async_api.h).  Part of libmpmhip; off the hot path.
//
// Reference: TC_IO serialization of MPM<dim> + ParticleAllocator (src/mpm.h:38-54,134-169), general_action "save" / "load"
// (src/mpm.cpp:940-960); AsyncMPM serialises every pool and the block table (src/async/async_mpm.h:120-172).  A blob holds the raw
// records — including the P2G affine matrices — so a restart continues exactly where the run stopped (up to the in-cell summation
// order).  It is loaded into an object of the same grid whose scene has been set up again: level set, configuration, the rigid
// bodies' meshes / outlines and scripts, mpmhip_async_begin come from the scene, not from the blob.
//
// What a blob looks like, and every test of one, is snapshot_blob.h (host bytes only).  Here: preparing the context, filling the
// header, ONE copy per section addressed through the layout, and the state transitions after a load.  All three loaders follow
// one rule: nothing of the context is written until the whole blob has passed its check.

extern "C++" {
namespace {
void snap_put(void *blob, snap::Sec s, const void *src) { if (s.len) memcpy((char *)blob + s.off, src, s.len); }
void snap_get(void *dst, const void *blob, snap::Sec s) { if (s.len) memcpy(dst, (const char *)blob + s.off, s.len); }
hipError_t snap_from_dev(void *blob, snap::Sec s, const void *dev) {
  return s.len ? hipMemcpy((char *)blob + s.off, dev, s.len, hipMemcpyDeviceToHost) : hipSuccess;
}
hipError_t snap_to_dev(void *dev, const void *blob, snap::Sec s) {
  return s.len ? hipMemcpy(dev, (const char *)blob + s.off, s.len, hipMemcpyHostToDevice) : hipSuccess;
}
// a group table / the six block tables of a scheduler <-> their sections
std::vector<GroupParams> snap_groups(const void *blob, snap::Sec s) {
  std::vector<GroupParams> gs(s.len / snap::GROUP_BYTES);
  snap_get(gs.data(), blob, s);
  return gs;
}
void snap_put_tables(void *blob, const snap::LayoutStore &L, const AsyncSched &A) {
  const std::vector<int64_t> *v[snap::N_TABLES] = {&A.continuous, &A.strength, &A.cfl, &A.particle_t, &A.backup_t, &A.local_min};
  for (int k = 0; k < snap::N_TABLES; k++) snap_put(blob, L.tables[k], v[k]->data());
}
void snap_get_tables(AsyncSched &A, const void *blob, const snap::LayoutStore &L) {
  std::vector<int64_t> *v[snap::N_TABLES] = {&A.continuous, &A.strength, &A.cfl, &A.particle_t, &A.backup_t, &A.local_min};
  for (int k = 0; k < snap::N_TABLES; k++) snap_get(v[k]->data(), blob, L.tables[k]);
}
// the clocks and counters of a stepper <-> the header fields both asynchronous formats name alike
template <class H>
void snap_put_sched(H &h, const AsyncResident &A) {
  h.nblk = (int64_t)A.nblk(); h.containers = A.store.size;
  h.current_t_int = A.current_t_int; h.min_delta_t_int = A.min_delta_t_int; h.max_delta_t_int = A.max_delta_t_int;
  h.update_counter = A.update_counter; h.step_counter = A.step_counter;
}
template <class H>
void snap_get_sched(AsyncResident &A, const H &h) {
  A.current_t_int = h.current_t_int; A.min_delta_t_int = h.min_delta_t_int; A.max_delta_t_int = h.max_delta_t_int;
  A.update_counter = h.update_counter; A.step_counter = h.step_counter;
  A.limits_version++;  // (the neighbour lists are rebuilt from the loaded limits at the next update)
}
// a state a blob can describe: no view, counters settled, the store holds exactly its live containers
template <class Ctx>
int snap_prepare_stepper(Ctx *c) {
  if (int rc = as_pool_particles(c)) return rc;  // (drops a view; pools what was added since)
  if (int rc = as_settle(c)) return rc;
  return as_compact(c);
}
// the store of a checked blob replaces the ctx's
template <class Ctx>
int snap_load_store(Ctx *c, const void *blob, const snap::LayoutStore &L, int64_t containers) {
  AsyncStore &S = c->async.store;
  S.size = S.size_ub = S.live = 0;
  if (int rc = as_store_reserve(c, (uint32_t)containers + 1024)) return rc;
  const hipError_t e = S.load((const char *)blob, L);
  return e == hipSuccess ? MPMHIP_OK : as_fail(c, MPMHIP_EHIP, std::string("loading the snapshot's containers failed: ") + hipGetErrorString(e));
}
}  // namespace
}  // extern "C++"

// ------------------------------------------------------------------------------------------------ 3D, synchronous
static snap::Layout3D snap3d_layout(const mpmhip_ctx *c) {
  snap::Counts3D n;
  n.n_groups = c->groups.size(); n.n_slots = (uint64_t)c->n_slots;
  n.rigid = n.collide = rigid_active(c);
  n.n_bodies = c->rigid.store.bodies.size(); n.n_joints = c->rigid.joints.size();
  snap::Layout3D L;
  snap::layout3d(n, snap::NO_LIMIT, L);
  return L;
}
int64_t mpmhip_snapshot_size(mpmhip_ctx *c) { return c ? (int64_t)snap3d_layout(c).total : MPMHIP_EINVAL; }

int mpmhip_snapshot_save(mpmhip_ctx *c, void *dst, size_t cap) {
  if (!c || !dst) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "snapshot inside a substep");
  const snap::Layout3D L = snap3d_layout(c);
  if (cap < L.total) return fail(c, MPMHIP_ECAPACITY, "snapshot buffer too small: %zu < %zu", cap, (size_t)L.total);
  Counters hc;
  int rc = read_counters(c, hc);
  if (rc) return rc;
  if (!c->rec.affine_valid()) {  // make A current first (fresh uploads), so that the blob is self-consistent
    hipLaunchKernelGGL(k_affine, dim3(particle_grid(c->n_slots)), dim3(256), 0, c->stream, c->P, c->rg, c->rp, c->rb, c->d_groups);
    c->rec.affine_rebuilt();
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  snap::SnapHeader h;
  memset(&h, 0, sizeof h);
  memcpy(h.magic, "MPMHIP01", 8);
  h.abi = MPMHIP_ABI_VERSION; h.n_groups = (uint32_t)c->groups.size();
  h.n_slots = c->n_slots; h.substeps = c->substeps; h.next_pid = c->next_pid;
  h.b_stale = c->rec.b_stale(); h.store_b = c->P.store_b;
  for (int k = 0; k < 3; k++) h.res[k] = c->P.res[k];
  h.t = c->t; h.request_t = c->request_t; h.dx = c->P.dx; h.dt = c->P.dt; h.n_dead = hc.n_dead;
  snap_put(dst, L.header, &h);
  snap_put(dst, L.groups, c->groups.data());
  HIPCHK(c, snap_from_dev(dst, L.rg, c->rg));
  HIPCHK(c, snap_from_dev(dst, L.rp, c->rp));
  HIPCHK(c, snap_from_dev(dst, L.rb, c->rb));
  if (L.rigid.len) {
    snap::SnapRigid r;
    memcpy(r.magic, "MPMRIGID", 8);
    r.n_bodies = (uint32_t)c->rigid.store.bodies.size(); r.n_joints = (uint32_t)c->rigid.joints.size();
    r.sizeof_body = (uint32_t)snap::BODY3_BYTES; r.sizeof_joint = (uint32_t)snap::JOINT3_BYTES;
    snap_put(dst, L.rigid, &r);
    HIPCHK(c, snap_from_dev(dst, L.bodies, c->rigid.d_rb));
    snap_put(dst, L.joints, c->rigid.joints.data());
    snap::SnapRigidCollide k;
    memcpy(k.magic, "MPMRRCOL", 8);
    k.on = c->rigid.col.on; k.iterations = c->rigid.col.iterations; k.position_iterations = c->rigid.col.position_iterations;
    k.penalty = c->rigid.col.penalty;
    snap_put(dst, L.collide, &k);
  }
  return MPMHIP_OK;
}

int mpmhip_snapshot_load(mpmhip_ctx *c, const void *src, size_t size) {
  if (!c || !src || size < sizeof(snap::SnapHeader)) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  snap::Facts f;
  for (int k = 0; k < 3; k++) f.res[k] = c->P.res[k];
  f.dx = c->P.dx; f.dt = c->P.dt; f.capacity = c->cap; f.groups_cap = c->groups_cap;
  f.n_bodies = rigid_active(c) ? (int64_t)c->rigid.store.bodies.size() : 0;
  snap::Blob3D B;
  const snap::Verdict v = snap::check3d(src, size, f, B);
  if (!v.ok()) return fail(c, v.rc, "%s", v.msg.c_str());
  const snap::SnapHeader &h = B.h;
  const snap::Layout3D &L = B.L;
  c->groups = snap_groups(src, L.groups);
  HIPCHK(c, snap_to_dev(c->d_groups, src, L.groups));
  HIPCHK(c, snap_to_dev(c->rg, src, L.rg));
  HIPCHK(c, snap_to_dev(c->rp, src, L.rp));
  HIPCHK(c, snap_to_dev(c->rb, src, L.rb));
  set_slots(c, h.n_slots);
  c->substeps = h.substeps; c->next_pid = h.next_pid;
  c->t = h.t; c->request_t = h.request_t;
  // A travels in the records; apic_b is current only if the saving ctx kept it up to date
  // (keys and block flags are rebuilt by the next sort)
  if (int rc = clear_block_flags(c, c->rec.snapshot_loaded(h.b_stale != 0 || h.store_b == 0))) return rc;
  if (c->P.store_b && c->rec.b_stale()) {  // this ctx keeps apic_b: rebuild it from A once
    int rc = ensure_b_current(c);
    if (rc) return rc;
  }
  Counters hc;
  memset(&hc, 0, sizeof hc);
  hc.n_dead = h.n_dead;
  HIPCHK(c, hipMemcpy(c->cnt, &hc, sizeof hc, hipMemcpyHostToDevice));
  if (B.has_rigid) {  // poses, velocities and joints of the saved run; colours travel in the records, the CDF is rebuilt every substep
    HIPCHK(c, snap_to_dev(c->rigid.d_rb, src, L.bodies));
    c->rigid.joints.resize(B.r.n_joints);
    snap_get(c->rigid.joints.data(), src, L.joints);
    HIPCHK(c, snap_to_dev(c->rigid.d_joints, src, L.joints));
    if (B.has_collide) {
      const snap::SnapRigidCollide &k = B.k;
      c->rigid.col.on = k.on != 0; c->rigid.col.iterations = k.iterations; c->rigid.col.position_iterations = k.position_iterations != 0;
      c->rigid.col.penalty = k.penalty;
    }
  }
  return MPMHIP_OK;
}

// ------------------------------------------------------------------------------------------------ 3D, asynchronous
// Loaded into a ctx of the same grid on which mpmhip_async_begin has run with the same unit_delta_t.
static snap::LayoutAsync snap_async_layout(const mpmhip_ctx *c) {
  snap::LayoutAsync L;
  snap::layout_async(c->groups.size(), c->async.nblk(), c->async.store.size, snap::NO_LIMIT, L);
  return L;
}
int64_t mpmhip_async_snapshot_size(mpmhip_ctx *c) {
  if (!c || !c->async.resident) return MPMHIP_EINVAL;
  if (int rc = snap_prepare_stepper(c)) return rc;
  return (int64_t)snap_async_layout(c).total;
}
int mpmhip_async_snapshot_save(mpmhip_ctx *c, void *dst, size_t cap) {
  if (!c || !dst) return MPMHIP_EINVAL;
  auto &A = c->async;
  if (!A.resident) return fail(c, MPMHIP_EINVAL, "mpmhip_async_begin first");
  const int64_t need = mpmhip_async_snapshot_size(c);
  if (need < 0) return (int)need;
  if (cap < (size_t)need) return fail(c, MPMHIP_ECAPACITY, "snapshot buffer too small: %zu < %lld", cap, (long long)need);
  const snap::LayoutAsync L = snap_async_layout(c);
  snap::SnapAsync h;
  memset(&h, 0, sizeof h);
  memcpy(h.magic, "MPMASYNC", 8);
  h.abi = MPMHIP_ABI_VERSION; h.n_groups = (uint32_t)c->groups.size();
  for (int k = 0; k < 3; k++) { h.res[k] = c->P.res[k]; h.nb[k] = A.nb[k]; }
  h.dx = c->P.dx; h.unit_delta_t = A.cfg.unit_delta_t;
  snap_put_sched(h, A);
  h.next_pid = c->next_pid; h.request_t = A.request_t; h.current_t = A.current_t;
  snap_put(dst, L.header, &h);
  snap_put(dst, L.groups, c->groups.data());
  snap_put_tables(dst, L.store, A);
  HIPCHK(c, A.store.save((char *)dst, L.store));
  c->host_particle_bytes += (int64_t)A.store.size * (int64_t)snap::CONTAINER3_BYTES;
  return MPMHIP_OK;
}
int mpmhip_async_snapshot_load(mpmhip_ctx *c, const void *src, size_t size) {
  if (!c || !src || size < sizeof(snap::SnapAsync)) return MPMHIP_EINVAL;
  auto &A = c->async;
  if (!A.resident) return fail(c, MPMHIP_EINVAL, "mpmhip_async_begin first");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  snap::Facts f;
  for (int k = 0; k < 3; k++) { f.res[k] = c->P.res[k]; f.nb[k] = A.nb[k]; }
  f.dx = c->P.dx; f.unit_delta_t = A.cfg.unit_delta_t; f.groups_cap = c->groups_cap; f.nblk = (int64_t)A.nblk();
  snap::BlobAsync B;
  const snap::Verdict v = snap::check_async(src, size, f, B);
  if (!v.ok()) return fail(c, v.rc, "%s", v.msg.c_str());
  const snap::SnapAsync &h = B.h;
  c->groups = snap_groups(src, B.L.groups);
  HIPCHK(c, snap_to_dev(c->d_groups, src, B.L.groups));
  snap_get_tables(A, src, B.L.store);
  if (int rc = snap_load_store(c, src, B.L.store, h.containers)) return rc;
  c->host_particle_bytes += h.containers * (int64_t)snap::CONTAINER3_BYTES;
  snap_get_sched(A, h);
  A.request_t = h.request_t; A.current_t = h.current_t;
  c->next_pid = h.next_pid;
  c->t = A.current_t;
  // (the one drop that leaves n_dead alone: a count left by the last working set stays until the next advance zeroes it)
  return drop_records(c, DEAD_KEEP);
}

// ------------------------------------------------------------------------------------------------ 2D
static int snap2d_prepare(mpmhip2d_ctx *m) {
  HIPCHK2D(m, hipSetDevice(m->device));
  if (m->async.resident)
    if (int rc = snap_prepare_stepper(m)) return rc;
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  return MPMHIP_OK;
}
static snap::Layout2D snap2d_layout(const mpmhip2d_ctx *m) {
  snap::Counts2D n;
  n.n_groups = m->groups.size(); n.n = (uint64_t)m->n;
  if (m->rigid_enabled) { n.n_bodies = m->rigid.bodies.size(); n.n_ranked = m->n_ranked; }
  n.has_async = m->async.resident; n.nblk = m->async.nblk(); n.containers = m->async.store.size;
  snap::Layout2D L;
  snap::layout2d(n, snap::NO_LIMIT, L);
  return L;
}
// the particle arrays in blob order (snap::P2_X ..)
static void snap2d_arrays(mpmhip2d_ctx *m, void *dev[snap::P2_ARRAYS]) {
  dev[snap::P2_X] = m->x; dev[snap::P2_V] = m->v; dev[snap::P2_F] = m->F; dev[snap::P2_B] = m->B;
  dev[snap::P2_AUX] = m->aux; dev[snap::P2_GID] = m->gid; dev[snap::P2_PID] = m->pid;
}
int64_t mpmhip2d_snapshot_size(mpmhip2d_ctx *m) {
  if (!m) return MPMHIP_EINVAL;
  if (int rc = snap2d_prepare(m)) return rc;
  return (int64_t)snap2d_layout(m).total;
}
int mpmhip2d_snapshot_save(mpmhip2d_ctx *m, void *dst, size_t cap) {
  if (!m || !dst) return MPMHIP_EINVAL;
  if (int rc = snap2d_prepare(m)) return rc;
  const snap::Layout2D L = snap2d_layout(m);
  if (cap < L.total) return fail2d(m, MPMHIP_ECAPACITY, "snapshot buffer too small");
  auto &A = m->async;
  snap::Snap2D h;
  memset(&h, 0, sizeof h);
  memcpy(h.magic, "MPM2DSNP", 8);
  h.abi = MPMHIP_ABI_VERSION; h.n_groups = (uint32_t)m->groups.size();
  h.res[0] = m->P.res[0]; h.res[1] = m->P.res[1]; h.next_pid = m->next_pid;
  h.n_bodies = m->rigid_enabled ? (int32_t)m->rigid.bodies.size() : 0; h.n_joints = m->joints.n; h.has_async = A.resident ? 1 : 0;
  h.n = m->n; h.dx = m->P.dx; h.base_dt = m->base_dt; h.t = m->t; h.request_t = m->request_t; h.n_ranked = m->rigid_enabled ? m->n_ranked : 0;
  HIPCHK2D(m, hipMemcpy(&h.n_dead, m->n_dead, 4, hipMemcpyDeviceToHost));
  if (A.resident) {
    h.nb[0] = A.nb[0]; h.nb[1] = A.nb[1]; h.unit_delta_t = A.cfg.unit_delta_t; h.a_request_t = A.request_t; h.a_current_t = A.current_t;
    snap_put_sched(h, A);
  }
  snap_put(dst, L.header, &h);
  snap_put(dst, L.groups, m->groups.data());
  void *arr[snap::P2_ARRAYS];
  snap2d_arrays(m, arr);
  for (int a = 0; a < snap::P2_ARRAYS; a++) HIPCHK2D(m, snap_from_dev(dst, L.arr[a], arr[a]));
  if (m->rigid_enabled) {
    HIPCHK2D(m, snap_from_dev(dst, L.bodies, m->d_rb));
    snap_put(dst, L.joints, &m->joints);
    HIPCHK2D(m, snap_from_dev(dst, L.ranks, m->d_smp_rank));
    HIPCHK2D(m, snap_from_dev(dst, L.colours, m->d_states));
  }
  if (A.resident) {
    snap_put_tables(dst, L.store, A);
    HIPCHK2D(m, A.store.save((char *)dst, L.store));
  }
  return MPMHIP_OK;
}
static int snap2d_load(mpmhip2d_ctx *m, const void *src, size_t size);
int mpmhip2d_snapshot_load(mpmhip2d_ctx *m, const void *src, size_t size) {
  if (!m || !src || size < sizeof(snap::Snap2D)) return MPMHIP_EINVAL;
  try { return snap2d_load(m, src, size); }
  catch (const std::bad_alloc &) { return fail2d(m, MPMHIP_ENOMEM, "host allocation failed while loading the snapshot"); }
}
static int snap2d_load(mpmhip2d_ctx *m, const void *src, size_t size) {
  HIPCHK2D(m, hipSetDevice(m->device));
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  auto &A = m->async;
  snap::Facts f;
  f.res[0] = m->P.res[0]; f.res[1] = m->P.res[1]; f.dx = m->P.dx;
  f.n_bodies = m->rigid_enabled ? (int64_t)m->rigid.bodies.size() : 0;
  f.resident = A.resident; f.nb[0] = A.nb[0]; f.nb[1] = A.nb[1]; f.nblk = (int64_t)A.nblk(); f.unit_delta_t = A.cfg.unit_delta_t;
  f.n_boundary = m->rigid.h_smp.size();
  snap::Blob2D B;
  const snap::Verdict v = snap::check2d(src, size, f, B);
  if (!v.ok()) return fail2d(m, v.rc, v.msg);
  const snap::Snap2D &h = B.h;
  const snap::Layout2D &L = B.L;
  if (int rc = a2_grow_particles_any(m, h.n)) return rc;
  m->groups = snap_groups(src, L.groups);
  HIPCHK2D(m, snap_to_dev(m->d_groups, src, L.groups));
  void *arr[snap::P2_ARRAYS];
  snap2d_arrays(m, arr);
  for (int a = 0; a < snap::P2_ARRAYS; a++) HIPCHK2D(m, snap_to_dev(arr[a], src, L.arr[a]));
  m->n = h.n; m->next_pid = h.next_pid; m->t = h.t; m->request_t = h.request_t;
  HIPCHK2D(m, hipMemcpy(m->n_dead, &h.n_dead, 4, hipMemcpyHostToDevice));
  if (h.n_bodies) {
    HIPCHK2D(m, snap_to_dev(m->d_rb, src, L.bodies));
    snap_get(&m->joints, src, L.joints);
    m->d_smp_rank.reset(); m->n_ranked = 0;
    if (h.n_ranked) {
      HIPCHK2D(m, m->d_smp_rank.alloc((size_t)m->rigid.h_smp.size() + m->rigid.h_smp.size() / 4 + 1024));
      HIPCHK2D(m, snap_to_dev(m->d_smp_rank, src, L.ranks));
      m->n_ranked = h.n_ranked;
    }
    HIPCHK2D(m, snap_to_dev(m->d_states, src, L.colours));
  }
  if (h.has_async) {
    snap_get_tables(A, src, L.store);
    if (int rc = snap_load_store(m, src, L.store, h.containers)) return rc;
    snap_get_sched(A, h);
    A.request_t = h.a_request_t; A.current_t = h.a_current_t;
    if (int rc = as_best_reserve(m)) return rc;
  }
  return MPMHIP_OK;
}
