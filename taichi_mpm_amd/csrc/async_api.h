// taichi_mpm_amd/csrc/async_api.h — host side of the device-resident asynchronous stepper for both ctx types (included by
// mpmhip.hip inside extern "C", behind both ctx definitions).  Part of libmpmhip.  Device side: k_async.h; block scheduler:
// async_sched.h; the store: AsyncStore (mpmhip.hip).
//
// AsyncMPM<dim> (src/async/async_mpm.{h,cpp}): per scheduler block a continuous_dt_limit (a power of two of unit_delta_t),
// a particle pool at the block's own time and a backup pool at an earlier time; step() walks the power-of-two levels and
// advance(limit) runs ONE ordinary substep, dt = unit_delta_t * limit, on the blocks of that level plus frozen copies of
// their neighbours.  Here the block tables (a few integers per block) and the level walk are host code, as in the reference;
// every container stays in HBM (k_async.h: the store), and an advance costs four small kernels around the substep and one
// 32-byte read-back (how many particles the working set has; how many containers were appended / freed; the append cursor).
//
// ONE driver (as_*), templated on the ctx type, carries both dimensions.  Fields both ctx types have under one name are used
// directly (stream, device, cap, t, P.dt, P.dx, P.idx, next_pid, d_groups, async); what a ctx does its own way comes first, as
// overloads on mpmhip_ctx * / mpmhip2d_ctx *.

struct AsTimer {  // wall time of a host-side section, accumulated into c->async.prof_ms[k] (synchronising sections included)
  double &acc; std::chrono::steady_clock::time_point t0;
  explicit AsTimer(double &a) : acc(a), t0(std::chrono::steady_clock::now()) {}
  ~AsTimer() { acc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// ---- what a ctx does its own way
static int as_fail(mpmhip_ctx *c, int code, const std::string &msg) { return fail(c, code, "%s", msg.c_str()); }
static int as_fail(mpmhip2d_ctx *m, int code, const std::string &msg) { return fail2d(m, code, msg); }
static const char *as_begin_first(const mpmhip_ctx *) { return "mpmhip_async_begin first"; }
static const char *as_begin_first(const mpmhip2d_ctx *) { return "mpmhip2d_async_begin first"; }
// Launch caps, in workgroups of 256: of the passes over the store, of the filing pass over the working set, of the chained scans
// (the compaction and the ordered forms: every launched workgroup must be resident — scan_limit asks the occupancy API per kernel,
// 64 always are).  The test knob MPMHIP_ASYNC_WGS lowers all of them (as_wgs).  The values
// are each dimension's own from before the two steppers shared this file; whether any of them matters for speed has not been measured.
static uint32_t as_store_wgs(const mpmhip_ctx *) { return 4096; }
static uint32_t as_store_wgs(const mpmhip2d_ctx *) { return 2048; }
static uint32_t as_file_wgs(const mpmhip_ctx *) { return 8192; }
static uint32_t as_file_wgs(const mpmhip2d_ctx *) { return 2048; }
static uint32_t as_scan_wgs(mpmhip_ctx *c, const void *kernel) { return scan_limit(c, kernel); }
static uint32_t as_scan_wgs(mpmhip2d_ctx *, const void *) { return 64; }
// deterministic mode: the ordered forms of the kernels that place containers (k_async.h) instead of the ones that place by arrival
static bool as_ordered(const mpmhip_ctx *c) { return c->deterministic; }
static bool as_ordered(const mpmhip2d_ctx *m) { return m->det.on; }
// the device views of the store (twin: the compaction's target) and of the working set
static Store3 as_store(const mpmhip_ctx *c, bool twin = false) {
  const AsyncStore &S = c->async.store;
  auto L = [&](int l) { return twin ? S.lane[l].b.get() : S.lane[l].a.get(); };
  return Store3{twin ? S.tag2 : S.tag, (int32_t *)L(0), (float4 *)L(1), (float4 *)L(2)};
}
static Store2 as_store(const mpmhip2d_ctx *m, bool twin = false) {
  const AsyncStore &S = m->async.store;
  return Store2{twin ? S.tag2 : S.tag, (float4 *)(twin ? S.lane[0].b.get() : S.lane[0].a.get())};
}
static Work3 as_work(const mpmhip_ctx *c) { return Work3{(float4 *)c->rg.get(), (float4 *)c->rp.get(), (float4 *)c->rb.get(), c->d_groups}; }
static Work2 as_work(const mpmhip2d_ctx *m) { return Work2{m->x, m->v, m->F, m->B, m->aux, m->gid, m->pid}; }
static int64_t as_slots(const mpmhip_ctx *c) { return c->n_slots; }
static int64_t as_slots(const mpmhip2d_ctx *m) { return m->n; }
// room for n working slots
static int as_make_room(mpmhip_ctx *c, int64_t n) { return n > c->cap ? mpmhip_reserve(c, n + 1024) : MPMHIP_OK; }
static int as_make_room(mpmhip2d_ctx *m, int64_t n) { return a2_grow_particles(m, n); }
static int as_ensure_blk_of(mpmhip_ctx *c) { return async_ensure_particle_arrays(c); }
static int as_ensure_blk_of(mpmhip2d_ctx *m) {
  auto &A = m->async;
  if (A.blk_of_cap < m->cap) {
    HIPCHK2D(m, A.d_blk_of.alloc((size_t)m->cap));
    A.blk_of_cap = m->cap;
  }
  return MPMHIP_OK;
}
// the working set is now n slots, none of them dead (the count is zeroed on the ctx stream, between the stepper's launches)
static int as_working_set(mpmhip_ctx *c, int64_t n) {
  if (int rc = drop_records(c, DEAD_ZERO_ON_STREAM)) return rc;
  set_slots(c, n);
  return MPMHIP_OK;
}
static int as_working_set(mpmhip2d_ctx *m, int64_t n) {
  m->n = n;
  HIPCHK2D(m, hipMemsetAsync(m->n_dead, 0, sizeof(unsigned int), m->stream));
  return MPMHIP_OK;
}
static int as_substep(mpmhip_ctx *c) {
  AsTimer sub(c->async.prof_ms[3]);
  if (int rc = mpmhip_substep(c)) return rc;
  if (c->async.profile_sync) HIPCHK(c, hipStreamSynchronize(c->stream));
  return MPMHIP_OK;
}
static int as_substep(mpmhip2d_ctx *m) { return substep2d(m); }
static int as_before_filing(mpmhip_ctx *c) { return ensure_b_current(c); }  // (the containers hold apic_b)
static int as_before_filing(mpmhip2d_ctx *) { return MPMHIP_OK; }
static void as_end_step(mpmhip_ctx *c) { set_slots(c, 0); }
static void as_end_step(mpmhip2d_ctx *m) { m->n = 0; m->P.dt = m->base_dt; }
// the 3D profile (mpmhip_async_profile): section k of prof_ms; an advance is counted where its timer starts
static AsTimer as_timer(mpmhip_ctx *c, int k) {
  if (k == 2) c->async.prof_ms[5] += 1.0;
  return AsTimer(c->async.prof_ms[k]);
}
static int as_timer(mpmhip2d_ctx *, int) { return 0; }

// the plain export of the pool containers: rows of Store::ROW floats in order of arrival
static void as_export_plain(const mpmhip_ctx *c, dim3 grid, uint32_t size, float *rows, uint32_t *blk) {
  const Store3 V = as_store(c);
  hipLaunchKernelGGL(k_async_export, grid, dim3(256), 0, c->stream, size, (const uint32_t *)V.tag, (const float4 *)V.g, (const float4 *)V.w, rows, blk,
                     c->async.store.d_cnt.get());
}
static void as_export_plain(const mpmhip2d_ctx *m, dim3 grid, uint32_t size, float *rows, uint32_t *blk) {
  hipLaunchKernelGGL(k_async_export2, grid, dim3(256), 0, m->stream, size, as_store(m), rows, blk, m->async.store.d_cnt.get());
}
static void as_host_bytes(mpmhip_ctx *c, int64_t bytes) { c->host_particle_bytes += bytes; }
static void as_host_bytes(mpmhip2d_ctx *, int64_t) {}

extern "C++" {
namespace {

#define AS_CHK(call)                                                                                                    \
  do {                                                                                                                  \
    const hipError_t e_ = (call);                                                                                       \
    if (e_ != hipSuccess) return as_fail(c, MPMHIP_EHIP, std::string(#call " failed: ") + hipGetErrorString(e_));      \
  } while (0)
#define AS_LAUNCHED(what)                                                                                               \
  do {                                                                                                                  \
    const hipError_t e_ = hipGetLastError();                                                                            \
    if (e_ != hipSuccess) return as_fail(c, MPMHIP_EHIP, std::string("launch of " what " failed: ") + hipGetErrorString(e_)); \
  } while (0)

// workgroups of an asynchronous launch that wants `want` and may have `limit`: TEST KNOB MPMHIP_ASYNC_WGS (read by as_begin) caps
// every one of them, so that a scene of a few thousand containers makes one workgroup walk several chunks of a chained scan
template <class Ctx>
uint32_t as_wgs(const Ctx *c, uint32_t want, uint32_t limit) {
  const uint32_t knob = c->async.test_wgs;
  return std::max<uint32_t>(std::min(std::min(want, limit), knob ? knob : limit), 1);
}
template <class Ctx>
dim3 as_grid(const Ctx *c, uint32_t n) { return dim3(as_wgs(c, (n + 255) / 256, as_store_wgs(c))); }

template <class Ctx>
int as_enter(Ctx *c) {  // every entry point of a resident stepper
  if (!c->async.resident) return as_fail(c, MPMHIP_EINVAL, as_begin_first(c));
  AS_CHK(hipSetDevice(c->device));
  return MPMHIP_OK;
}
// a new session on this ctx: an empty store (whatever an earlier session left goes), the block times of sched_begin
template <class Ctx>
int as_begin(Ctx *c, std::initializer_list<size_t> lane_bytes) {
  auto &A = c->async;
  if (int rc = async_drop_view(c)) return rc;
  AS_CHK(hipStreamSynchronize(c->stream));
  A.resident = false;
  A.sched_begin();  // block times, the reference's block order, cached_neighbours
  A.d_blk_of.reset(); A.blk_of_cap = 0;  // (the next load_pools allocates it again)
  for (int32_t &f : A.forms) f = -1;
  const char *knob = getenv("MPMHIP_ASYNC_WGS");
  A.test_wgs = knob ? (uint32_t)std::max(atoi(knob), 0) : 0u;
  const hipError_t e = A.store.reset(lane_bytes, A.rank_of);
  if (e != hipSuccess) return as_fail(c, MPMHIP_ENOMEM, std::string("async store: tables of a new session: ") + hipGetErrorString(e));
  A.resident = true;
  return MPMHIP_OK;
}

template <class Ctx>
int as_store_reserve(Ctx *c, uint32_t need) {  // room for `need` containers in total
  auto &S = c->async.store;
  if (need <= S.cap) return MPMHIP_OK;
  AS_CHK(hipStreamSynchronize(c->stream));
  const hipError_t e = S.reserve(need);
  if (e != hipSuccess) return as_fail(c, MPMHIP_ENOMEM, "async store: growing to " + std::to_string(AsyncStore::grown(need)) + " containers failed: " + hipGetErrorString(e));
  return MPMHIP_OK;
}
// the per-block action table of an advance -> S.d_tbl, ORDERED ON THE CTX STREAM behind the kernels that still read the
// previous table (the ctx stream is non-blocking: a plain hipMemcpy would run beside them) and from pinned memory (the host
// refills A.tbl right away): a ring of four pinned images — every advance synchronises the stream between its two uploads, so
// an image is never rewritten while its copy is still pending
template <class Ctx>
int as_upload_tbl(Ctx *c) {
  auto &A = c->async;
  auto &S = A.store;
  const size_t nblk = A.tbl.size();
  uint8_t *img = S.h_tbl_pin + (size_t)(S.pin_next++ & 3) * nblk;
  memcpy(img, A.tbl.data(), nblk);
  AS_CHK(hipMemcpyAsync(S.d_tbl, img, nblk, hipMemcpyHostToDevice, c->stream));
  return MPMHIP_OK;
}
template <class Ctx>
int as_best_reserve(Ctx *c) {  // one dedup word per creation id
  auto &S = c->async.store;
  if ((int64_t)c->next_pid <= S.best_cap) return MPMHIP_OK;
  const size_t cap = AsyncStore::ids_grown((size_t)c->next_pid);
  AS_CHK(S.best.alloc(cap));
  AS_CHK(hipMemsetAsync(S.best, 0xFF, sizeof(unsigned long long) * cap, c->stream));
  S.best_cap = (int64_t)cap;
  return MPMHIP_OK;
}
// the ONE read-back of an advance: the transient counters (reset behind the copy) and the append cursor.  Folds what earlier
// launches appended / freed into the host's view of the store.
template <class Ctx>
int as_counters(Ctx *c, AsyncCounters &h) {
  auto &S = c->async.store;
  AS_CHK(hipMemcpyAsync(S.h_cnt, S.d_cnt, sizeof h, hipMemcpyDeviceToHost, c->stream));
  AS_CHK(hipMemsetAsync(S.d_cnt, 0, 16, c->stream));
  AS_CHK(hipStreamSynchronize(c->stream));
  h = *S.h_cnt;
  if (h.pad[0] & SCAN_ERROR_BIT)
    return as_fail(c, MPMHIP_EHIP, "async store: a chained scan of the compaction waited " + std::to_string(SCAN_WAIT_TICKS / 100000000ull) +
                                       " s for a chunk that never published (k_sort.h: the launch did not fit the device's resident set?)");
  S.fold(h.n_append, h.n_freed, h.size);
  S.pending_counters = false;
  return MPMHIP_OK;
}
// counters a previous advance left on the device (appended / freed containers): folded into the host's view of the store
template <class Ctx>
int as_settle(Ctx *c) {
  AsyncCounters h;
  return c->async.store.pending_counters ? as_counters(c, h) : MPMHIP_OK;
}
// the launch of a chained scan over n elements (the compaction, the ordered forms): its scan words sized and zeroed, a fresh epoch,
// no more workgroups than stay resident
struct AsScan { unsigned long long *slots; uint32_t epoch; dim3 grid; };
template <class Ctx>
int as_scan(Ctx *c, uint32_t n, const void *kernel, AsScan &out) {
  auto &S = c->async.store;
  const uint32_t nchunks = (n + 1023) / 1024;
  if (nchunks + 1 > S.scan_cap) {
    AS_CHK(hipStreamSynchronize(c->stream));  // (a pending launch may still read the old words)
    AS_CHK(S.d_scan.alloc((size_t)nchunks + 1024));
    AS_CHK(hipMemsetAsync(S.d_scan, 0, sizeof(unsigned long long) * ((size_t)nchunks + 1024), c->stream));
    S.scan_cap = nchunks + 1024;
  }
  if (++S.scan_epoch == 0u) S.scan_epoch = 1u;  // (0 = never published)
  out = AsScan{S.d_scan.get(), S.scan_epoch, dim3(as_wgs(c, nchunks, as_scan_wgs(c, kernel)))};
  return MPMHIP_OK;
}
// (called with the counters settled: S.size and S.live are exact.)  The store holds exactly its live containers afterwards.
template <class Ctx>
int as_compact(Ctx *c) {
  auto &S = c->async.store;
  if (S.size == 0) return MPMHIP_OK;
  auto whole = as_timer(c, 4);
  (void)whole;
  if (const hipError_t e = S.reserve_twins(); e != hipSuccess) return as_fail(c, MPMHIP_ENOMEM, std::string("async store: compaction buffers: ") + hipGetErrorString(e));
  AS_CHK(hipMemsetAsync(S.tag2, 0xFF, sizeof(uint32_t) * (size_t)S.cap, c->stream));
  AsScan sc;
  if (int rc = as_scan(c, S.size, (const void *)k_async_compact<decltype(as_store(c))>, sc)) return rc;
  const auto V = as_store(c), V2 = as_store(c, true);
  hipLaunchKernelGGL(k_async_compact<decltype(as_store(c))>, sc.grid, dim3(256), 0, c->stream, S.size, V, V2, sc.slots, sc.epoch, S.d_cnt.get());
  AS_LAUNCHED("async_compact");
  S.swap_twins();
  AsyncCounters h;
  if (int rc = as_counters(c, h)) return rc;  // (size = live = what the scan counted)
  S.live = h.size;
  S.compactions++;
  return MPMHIP_OK;
}

// the ctx's particles hold a view of the pools (load_pools): they are copies, dropped before anything else uses the arrays
template <class Ctx>
int as_drop_view(Ctx *c) {
  auto &A = c->async;
  if (!A.resident || !A.store.view) return MPMHIP_OK;
  A.store.view = false;
  return as_working_set(c, 0);
}

// the working set (n slots) -> containers behind the store's end; all_to_pool: every particle goes to its block's pool
template <class Ctx>
int as_file(Ctx *c, uint32_t n, int all_to_pool) {
  auto &A = c->async;
  auto &S = A.store;
  if (int rc = as_store_reserve(c, AsyncStore::sum(S.size, n))) return rc;
  if ((A.forms[1] = as_ordered(c))) {
    AsScan sc;
    if (int rc = as_scan(c, n, (const void *)k_async_file_ordered<decltype(as_work(c))>, sc)) return rc;
    hipLaunchKernelGGL(k_async_file_ordered<decltype(as_work(c))>, sc.grid, dim3(256), 0, c->stream, c->P.idx, n, as_work(c),
                       (const uint8_t *)S.d_tbl, all_to_pool, A.nb[0], A.nb[1], A.nb[2], S.cap, as_store(c), sc.slots, sc.epoch, S.d_cnt.get());
  } else {
    hipLaunchKernelGGL(k_async_file<decltype(as_work(c))>, dim3(as_wgs(c, (n + 255) / 256, as_file_wgs(c))), dim3(256), 0, c->stream, c->P.idx, n,
                       as_work(c), (const uint8_t *)S.d_tbl, all_to_pool, A.nb[0], A.nb[1], A.nb[2], S.cap, as_store(c), S.d_cnt.get());
  }
  AS_LAUNCHED("async_file");
  return MPMHIP_OK;
}

// AsyncMPM<dim>::add_particles (src/async/async_mpm.cpp:57-75): the particles currently in the ctx's arrays (just added) move to
// the particle pools of their blocks; the arrays are empty afterwards (creation ids keep counting: next_pid stays).
template <class Ctx>
int as_pool_particles(Ctx *c) {
  if (int rc = as_enter(c)) return rc;
  if (int rc = as_drop_view(c)) return rc;
  if (as_slots(c) == 0) return MPMHIP_OK;
  if (int rc = as_settle(c)) return rc;
  if (int rc = as_before_filing(c)) return rc;
  if (int rc = as_file(c, (uint32_t)as_slots(c), 1)) return rc;
  AsyncCounters h;
  if (int rc = as_counters(c, h)) return rc;
  return as_working_set(c, 0);
}

// AsyncMPM<dim>::update_dt_limits (src/async/async_mpm.cpp:90-253) over the resident pools
template <class Ctx>
int as_update_dt_limits(Ctx *c) {
  auto &A = c->async;
  auto &S = A.store;
  const uint32_t nblk = (uint32_t)A.nblk();
  auto whole = as_timer(c, 0);
  (void)whole;
  hipLaunchKernelGGL(k_async_table_reset, as_grid(c, nblk), dim3(256), 0, c->stream, nblk, A.d_tab.get());
  hipLaunchKernelGGL(k_async_store_reduce<decltype(as_store(c))>, as_grid(c, S.size_ub), dim3(256), 0, c->stream, c->P.dx, S.size_ub, as_store(c),
                     (const GroupParams *)c->d_groups, A.d_tab.get());
  AS_LAUNCHED("async_store_reduce");
  A.scratch = A.continuous;
  if (int rc = async_limits_from_table(c)) return rc;  // the block state machine shared with mpmhip_async_update_dt_limits
  if (A.scratch != A.continuous) A.limits_version++;
  auto lists = as_timer(c, 1);
  (void)lists;
  A.rebuild_lists();  // larger / smaller neighbours per level (:183-247), local_min_dt_limit (:165-182)
  return MPMHIP_OK;
}

// AsyncMPM<dim>::advance (src/async/async_mpm.cpp:255-373)
template <class Ctx>
int as_advance(Ctx *c, int64_t limit) {
  auto &A = c->async;
  auto &S = A.store;
  const int64_t t = A.current_t_int;
  auto whole = as_timer(c, 2);
  (void)whole;
  if (!A.plan_gather(limit)) return as_fail(c, MPMHIP_EINVAL, A.sched_err);
  if (int rc = as_best_reserve(c)) return rc;
  if (int rc = as_upload_tbl(c)) return rc;
  // the working set holds at most one container per id (duplicates are dropped by the gather), i.e. at most
  // min(containers, ids handed out) particles: the ctx's arrays get that room BEFORE the gather writes into them — a
  // C-ABI caller may have pooled several batches of up to `cap` particles each (pool_particles empties the slots)
  if (int rc = as_make_room(c, std::min<int64_t>((int64_t)S.size_ub, (int64_t)c->next_pid))) return rc;
  hipLaunchKernelGGL(k_async_mark<decltype(as_store(c))>, as_grid(c, S.size_ub), dim3(256), 0, c->stream, S.size_ub, as_store(c),
                     (const uint8_t *)S.d_tbl, (const uint32_t *)S.d_rank, S.best.get());
  if ((A.forms[0] = as_ordered(c))) {
    AsScan sc;
    if (int rc = as_scan(c, S.size_ub, (const void *)k_async_gather_ordered<decltype(as_work(c))>, sc)) return rc;
    hipLaunchKernelGGL(k_async_gather_ordered<decltype(as_work(c))>, sc.grid, dim3(256), 0, c->stream, S.size_ub, as_store(c),
                       (const uint8_t *)S.d_tbl, (const uint32_t *)S.d_rank, S.best.get(), as_work(c), sc.slots, sc.epoch, S.d_cnt.get());
  } else {
    hipLaunchKernelGGL(k_async_gather<decltype(as_work(c))>, as_grid(c, S.size_ub), dim3(256), 0, c->stream, S.size_ub, as_store(c),
                       (const uint8_t *)S.d_tbl, (const uint32_t *)S.d_rank, S.best.get(), as_work(c), S.d_cnt.get());
  }
  AS_LAUNCHED("async_gather");
  AsyncCounters h;
  if (int rc = as_counters(c, h)) return rc;  // the one read-back of an advance (also settles the previous one's appends)
  const uint32_t n_work = h.n_work;
  if ((int64_t)n_work > c->cap)
    return as_fail(c, MPMHIP_ECAPACITY, "async: a working set of " + std::to_string(n_work) + " particles exceeds the ctx capacity " + std::to_string(c->cap));
  A.update_counter += n_work;
  // ONE ordinary substep of the working set with this level's dt (:327-329; step() sets base_delta_t / current_t, :405-408)
  if (int rc = as_working_set(c, n_work)) return rc;  // the gather replaced the ctx's particles by the working set
  c->P.dt = A.cfg.unit_delta_t * (float)limit;
  c->t = A.cfg.unit_delta_t * (float)t;
  if (n_work) {
    if (int rc = as_substep(c)) return rc;
  }
  const bool any_clear = A.plan_file(limit);  // update backup_t and particle_t (:331-343), destinations of the results
  if (int rc = as_upload_tbl(c)) return rc;
  if (any_clear)
    hipLaunchKernelGGL(k_async_clear, as_grid(c, S.size), dim3(256), 0, c->stream, S.size, S.tag.get(), (const uint8_t *)S.d_tbl, S.d_cnt.get());
  if (n_work) {
    if (S.wants_compaction(n_work)) {  // (right behind the read-back: S.size and S.live are exact)
      if (int rc = as_compact(c)) return rc;
    }
    if (int rc = as_file(c, n_work, 0)) return rc;
    S.size_ub = AsyncStore::sum(S.size, n_work);  // (the exact size comes with the next read-back)
  }
  AS_LAUNCHED("async_clear");
  S.pending_counters = true;
  return MPMHIP_OK;
}

// AsyncMPM<dim>::step (src/async/async_mpm.cpp:380-421)
template <class Ctx>
int as_step(Ctx *c, float dt) {
  auto &A = c->async;
  if (int rc = as_enter(c)) return rc;
  if (dt < 0) return as_fail(c, MPMHIP_EINVAL, "AsyncMPM::step(dt < 0) is the synchronous substep of the base class");
  if (int rc = as_pool_particles(c)) return rc;  // (drops a view; pools particles added since the last step)
  A.request_t += dt;
  do {
    if (int rc = as_update_dt_limits(c)) return rc;
    for (int64_t d = A.max_delta_t_int; d >= A.min_delta_t_int; d >>= 1)
      if (A.current_t_int % d == 0) {
        if (int rc = as_advance(c, d)) return rc;
      }
    A.finish_round();
  } while (A.current_t < A.request_t);
  if (int rc = as_settle(c)) return rc;
  as_end_step(c);  // the arrays held the last working set: the state is in the pools
  c->t = A.current_t;
  A.step_counter++;
  return MPMHIP_OK;
}

// {current_t_int, update_counter, min_delta_t_int, max_delta_t_int, live containers, store size, compactions, steps}
template <class Ctx>
int as_state(Ctx *c, int64_t out[8]) {
  auto &A = c->async;
  if (int rc = as_enter(c)) return rc;
  if (int rc = as_settle(c)) return rc;
  out[0] = A.current_t_int; out[1] = A.update_counter; out[2] = A.min_delta_t_int; out[3] = A.max_delta_t_int;
  out[4] = A.store.live; out[5] = A.store.size; out[6] = A.store.compactions; out[7] = A.step_counter;
  return MPMHIP_OK;
}

// AsyncMPM<dim>::visualize's particle list (src/async/async_visualize.cpp:17-26,86-96): ALL containers of all particle pools
// become the ctx's particles (each at its block's particle_t; an id can occur more than once, as in the reference), so that
// frame output, downloads, energy and snapshots of the base class see the whole state, not the last working set; d_blk_of gets
// the pool block of each.  The view is dropped by the next step or add.
template <class Ctx>
int as_load_pools(Ctx *c) {
  auto &A = c->async;
  auto &S = A.store;
  if (int rc = as_pool_particles(c)) return rc;  // (drops an earlier view; pools particles added since)
  if (int rc = as_settle(c)) return rc;
  if (int rc = as_make_room(c, (int64_t)S.live)) return rc;
  if (int rc = as_ensure_blk_of(c)) return rc;
  if ((A.forms[2] = as_ordered(c))) {
    AsScan sc;
    if (int rc = as_scan(c, S.size, (const void *)k_async_load_ordered<decltype(as_work(c))>, sc)) return rc;
    hipLaunchKernelGGL(k_async_load_ordered<decltype(as_work(c))>, sc.grid, dim3(256), 0, c->stream, S.size, as_store(c), as_work(c),
                       A.d_blk_of.get(), sc.slots, sc.epoch, S.d_cnt.get());
  } else {
    hipLaunchKernelGGL(k_async_load<decltype(as_work(c))>, as_grid(c, S.size), dim3(256), 0, c->stream, S.size, as_store(c), as_work(c),
                       A.d_blk_of.get(), S.d_cnt.get());
  }
  AS_LAUNCHED("async_load");
  AsyncCounters h;
  if (int rc = as_counters(c, h)) return rc;
  if (int rc = as_working_set(c, h.n_work)) return rc;  // k_async_load replaced the ctx's particles by the view
  S.view = true;
  return MPMHIP_OK;
}

// Every container of every particle pool as rows of Store::ROW floats + the container's block (mpmhip_async_download_pools,
// mpmhip2d_async_download_pools).  rows == NULL: only the count.
template <class Ctx>
int64_t as_download_pools(Ctx *c, int64_t capacity, float *rows, int32_t *block) {
  using Store = decltype(as_store(c));
  auto &A = c->async;
  auto &S = A.store;
  if (int rc = as_enter(c)) return rc;
  if (int rc = as_settle(c)) return rc;
  DevBuf<float> d_rows;
  DevBuf<uint32_t> d_blk;
  const size_t m = std::max<size_t>(S.size, 1);
  AS_CHK(d_rows.alloc(m * Store::ROW));
  AS_CHK(d_blk.alloc(m));
  if ((A.forms[3] = as_ordered(c))) {
    AsScan sc;
    if (int rc = as_scan(c, S.size, (const void *)k_async_export_ordered<Store>, sc)) return rc;
    hipLaunchKernelGGL(k_async_export_ordered<Store>, sc.grid, dim3(256), 0, c->stream, S.size, as_store(c), d_rows.get(), d_blk.get(), sc.slots,
                       sc.epoch, S.d_cnt.get());
  } else {
    as_export_plain(c, as_grid(c, S.size), S.size, d_rows.get(), d_blk.get());
  }
  AS_LAUNCHED("async_export");
  AsyncCounters h;
  if (int rc = as_counters(c, h)) return rc;
  const int64_t n = (int64_t)h.n_work;
  if (!rows || !block || !n) return n;
  if (capacity < n)
    return as_fail(c, MPMHIP_ECAPACITY, "async download: " + std::to_string(n) + " containers, room for " + std::to_string(capacity));
  AS_CHK(hipMemcpy(rows, d_rows, sizeof(float) * Store::ROW * (size_t)n, hipMemcpyDeviceToHost));
  AS_CHK(hipMemcpy(block, d_blk, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
  as_host_bytes(c, n * Store::ROW * 4);
  return n;
}
// {gather, file, load, export} of the most recent launch of each in this session: 0 arrival order, 1 ordered, -1 not launched yet
template <class Ctx>
int as_forms(Ctx *c, int32_t out[4]) {
  if (!c->async.resident) return as_fail(c, MPMHIP_EINVAL, as_begin_first(c));
  for (int k = 0; k < 4; k++) out[k] = c->async.forms[k];
  return MPMHIP_OK;
}

// the reduced table -> the block state machine of AsyncMPM<dim>::update_dt_limits (AsyncSched::limits_from_table)
template <class Ctx>
int async_limits_from_table(Ctx *c) {
  auto &A = c->async;
  const size_t nblk = A.nblk();
  if (A.h_tab_cap < 3 * nblk) {  // pinned staging (a copy into pageable memory is staged by the runtime: ~50 us more)
    AS_CHK(A.h_tab.alloc(3 * nblk));
    A.h_tab_cap = 3 * nblk;
  }
  AS_CHK(hipMemcpyAsync(A.h_tab, A.d_tab, sizeof(uint32_t) * 3 * nblk, hipMemcpyDeviceToHost, c->stream));
  AS_CHK(hipStreamSynchronize(c->stream));
  if (!A.limits_from_table(A.h_tab, c->P.dx)) return as_fail(c, MPMHIP_EINVAL, A.sched_err);
  return MPMHIP_OK;
}

}  // namespace
}  // extern "C++"

static int async_drop_view(mpmhip_ctx *c) { return as_drop_view(c); }
static int async_drop_view(mpmhip2d_ctx *m) { return as_drop_view(m); }

// ------------------------------------------------------------------------------------------------ the 3D entry points
// AsyncMPM<dim>::initialize (src/async/async_mpm.cpp:13-55) on top of mpmhip_async_enable: the pools become device-resident
int mpmhip_async_begin(mpmhip_ctx *c, const mpmhip_async_config *cfg) {
  if (!c || !cfg) return MPMHIP_EINVAL;
  if (rigid_active(c) || c->rigid.enabled) return fail(c, MPMHIP_EINVAL, "asynchronous stepping cannot be combined with rigid bodies");
  if (c->T.enabled) return fail(c, MPMHIP_EINVAL, "asynchronous stepping cannot be combined with the multi-GPU tiling");
  if (!c->P.store_b) return fail(c, MPMHIP_EINVAL, "asynchronous stepping needs a ctx that keeps apic_b (discard_apic_b = 0): the "
                                                   "P2G matrix depends on each advance's dt and is rebuilt from it");
  if (int rc = mpmhip_async_enable(c, cfg)) return rc;
  return as_begin(c, {sizeof(int32_t), 4 * sizeof(float4), 4 * sizeof(float4)});  // lanes: id, g, w (k_async.h: Store3)
}
int mpmhip_async_pool_particles(mpmhip_ctx *c) { return c ? as_pool_particles(c) : MPMHIP_EINVAL; }
int mpmhip_async_step(mpmhip_ctx *c, float dt) { return c ? as_step(c, dt) : MPMHIP_EINVAL; }
int mpmhip_async_state(mpmhip_ctx *c, int64_t out[8]) { return c && out ? as_state(c, out) : MPMHIP_EINVAL; }
// host wall time so far, ms: {update_dt_limits, of which neighbour lists, advance, of which the substep (only meaningful with
// sync != 0: the stream is then synchronised behind every substep), compaction, number of advances}
int mpmhip_async_profile(mpmhip_ctx *c, int32_t sync, double out[6]) {
  if (!c || !out) return MPMHIP_EINVAL;
  for (int k = 0; k < 6; k++) out[k] = c->async.prof_ms[k];
  c->async.profile_sync = sync != 0;
  return MPMHIP_OK;
}
double mpmhip_async_current_time(const mpmhip_ctx *c) { return c ? (double)c->async.current_t : 0.0; }
int64_t mpmhip_host_particle_bytes(const mpmhip_ctx *c) { return c ? c->host_particle_bytes : MPMHIP_EINVAL; }

// per block of the dense table (mpmhip_async_table gives the limits): particle_t, backup_t, local_min_dt_limit
int64_t mpmhip_async_block_times(mpmhip_ctx *c, int64_t capacity, int64_t *particle_t, int64_t *backup_t, int64_t *local_min) {
  if (!c || !c->async.resident) return MPMHIP_EINVAL;
  auto &A = c->async;
  const int64_t n = (int64_t)A.particle_t.size();
  if (capacity < n) return n;
  for (int64_t b = 0; b < n; b++) {
    if (particle_t) particle_t[b] = A.particle_t[b];
    if (backup_t) backup_t[b] = A.backup_t[b];
    if (local_min) local_min[b] = A.local_min[b];
  }
  return n;
}

// Every container of every particle pool (each at its block's particle_t; an id can occur more than once, as in the
// reference) as rows of 27 floats {x3, v3, F9, apic_b9, aux, gid bits, id bits} + the container's block.  rows == NULL:
// only the count.  (Tests and host-side inspection: the stepping itself never calls this.)
int64_t mpmhip_async_download_pools(mpmhip_ctx *c, int64_t capacity, float *rows, int32_t *block) {
  return c ? as_download_pools(c, capacity, rows, block) : MPMHIP_EINVAL;
}
int mpmhip_async_forms(mpmhip_ctx *c, int32_t out[4]) { return c && out ? as_forms(c, out) : MPMHIP_EINVAL; }

// as_load_pools, and each particle of the view gets its pool block's (continuous, strength, cfl) limits for the frame's `limit` attribute
int mpmhip_async_load_pools(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  auto &A = c->async;
  if (int rc = as_load_pools(c)) return rc;
  c->P.dt = c->cfg.dt;  // (the P2G matrices are rebuilt for the configured base step if anybody runs a synchronous substep)
  if (c->n_slots) {
    const size_t nblk = A.nblk();
    std::vector<int32_t> lim(3 * nblk);
    for (size_t b = 0; b < nblk; b++) { lim[3 * b] = (int32_t)A.continuous[b]; lim[3 * b + 1] = (int32_t)A.strength[b]; lim[3 * b + 2] = (int32_t)A.cfl[b]; }
    HIPCHK(c, hipMemcpy(A.d_blk_limits, lim.data(), sizeof(int32_t) * 3 * nblk, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_async_particle_limits, dim3(particle_grid(c->n_slots)), dim3(256), 0, c->stream, c->P,
                       (const uint32_t *)A.d_blk_of, (const int32_t *)A.d_blk_limits, A.d_particle_limits);
    if (int rc = launch_check(c, "async_particle_limits")) return rc;
    A.limits_valid = true;
  }
  return MPMHIP_OK;
}

// ------------------------------------------------------------------------------------------------ the 2D entry points
// AsyncMPM<2>::initialize (src/async/async_mpm.cpp:13-55) on top of mpmhip2d_create
int mpmhip2d_async_begin(mpmhip2d_ctx *m, const mpmhip_async_config *cfg) {
  if (!m || !cfg) return MPMHIP_EINVAL;
  if (!(cfg->unit_delta_t > 0) || cfg->max_units < 1) return fail2d(m, MPMHIP_EINVAL, "unit_delta_t > 0 and max_units >= 1 required");
  if (m->rigid_enabled) return fail2d(m, MPMHIP_EINVAL, "asynchronous stepping cannot be combined with rigid bodies");
  HIPCHK2D(m, hipSetDevice(m->device));
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  auto &A = m->async;
  A.sched_enable(2, m->P.res, *cfg);
  HIPCHK2D(m, A.d_tab.alloc(3 * A.nblk()));
  return as_begin(m, {4 * sizeof(float4)});  // lane: rec (k_async.h: Store2)
}
int mpmhip2d_async_pool_particles(mpmhip2d_ctx *m) { return m ? as_pool_particles(m) : MPMHIP_EINVAL; }
int mpmhip2d_async_step(mpmhip2d_ctx *m, float dt) { return m ? as_step(m, dt) : MPMHIP_EINVAL; }
int mpmhip2d_async_state(mpmhip2d_ctx *m, int64_t out[8]) { return m && out ? as_state(m, out) : MPMHIP_EINVAL; }
double mpmhip2d_async_current_time(const mpmhip2d_ctx *m) { return m ? (double)m->async.current_t : 0.0; }
// as_load_pools: mpmhip2d_download / _num_particles then see the whole state.  Returns the number of containers.
int64_t mpmhip2d_async_load_pools(mpmhip2d_ctx *m) {
  if (!m) return MPMHIP_EINVAL;
  if (int rc = as_load_pools(m)) return rc;
  return m->n;
}

// every container of every particle pool as rows of 16 floats — the container as stored: {x2, v2, F4, apic_b4, aux, gid bits, id bits, -}
// — + its block; rows == NULL: only the count.  (Tests and host-side inspection.)
int64_t mpmhip2d_async_download_pools(mpmhip2d_ctx *m, int64_t capacity, float *rows, int32_t *block) {
  return m ? as_download_pools(m, capacity, rows, block) : MPMHIP_EINVAL;
}
int mpmhip2d_async_forms(mpmhip2d_ctx *m, int32_t out[4]) { return m && out ? as_forms(m, out) : MPMHIP_EINVAL; }

// dense view of the block table: nb[2] blocks per axis (block b = bx nb[1] + by, 8 x 16 nodes each); any output may be NULL.
// capacity < number of blocks: only the number is returned.
int64_t mpmhip2d_async_table(mpmhip2d_ctx *m, int32_t nb[2], int64_t capacity, int64_t *strength, int64_t *cfl, int64_t *continuous,
                             int64_t *count, int64_t *particle_t, int64_t *backup_t, int64_t *local_min) {
  if (!m || !m->async.resident || !nb) return MPMHIP_EINVAL;
  auto &A = m->async;
  nb[0] = A.nb[0]; nb[1] = A.nb[1];
  const int64_t n = (int64_t)A.nblk();
  if (capacity < n) return n;
  for (int64_t b = 0; b < n; b++) {
    if (strength) strength[b] = A.strength[b];
    if (cfl) cfl[b] = A.cfl[b];
    if (continuous) continuous[b] = A.continuous[b];
    if (count) count[b] = A.count[b];
    if (particle_t) particle_t[b] = A.particle_t[b];
    if (backup_t) backup_t[b] = A.backup_t[b];
    if (local_min) local_min[b] = A.local_min[b];
  }
  return n;
}
// the pool block of every particle of the view, in the order mpmhip2d_download lists them
int64_t mpmhip2d_async_view_blocks(mpmhip2d_ctx *m, int64_t capacity, int32_t *block) {
  if (!m || !block) return MPMHIP_EINVAL;
  auto &A = m->async;
  if (!A.resident || !A.store.view) return fail2d(m, MPMHIP_EINVAL, "mpmhip2d_async_load_pools first");
  if (capacity < m->n) return fail2d(m, MPMHIP_ECAPACITY, "block buffer too small");
  HIPCHK2D(m, hipSetDevice(m->device));
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  if (m->n) HIPCHK2D(m, hipMemcpy(block, A.d_blk_of, sizeof(uint32_t) * (size_t)m->n, hipMemcpyDeviceToHost));
  return m->n;
}
