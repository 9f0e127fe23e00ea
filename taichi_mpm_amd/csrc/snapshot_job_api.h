// taichi_mpm_amd/csrc/snapshot_job_api.h — the snapshot of a whole tiled job: ONE MPMHIP01 blob (snapshot_blob.h) whatever the
// bricks, and that blob — or any one-ctx blob — loaded by every rank of a job of any layout, each rank keeping its own brick.
// Included by mpmhip.hip behind tiled_api.h.  Kernels: k_snapshot_job.h, compiled by k_frame.hip and launched through
// snapshot_job_launch.h; the ranking is the frame's (frame_job_api.h: fj_*).  Off the hot path.
//
// The job's blob is the canonical form of the format: no dead slot (n_slots = the job's live particles, n_dead = 0), rows in ascending
// creation id, next_pid = max(the ranks' next_pid, 1 + the largest live id); clocks, grid, dt, store_b and the group table must agree
// on every rank.  mpmhip_snapshot_load on one ctx accepts it unchanged.
//   mpmhip_snapshot_size_group / mpmhip_snapshot_save_group   the K ctx of one process on one device: every ctx's stream drained, then
//       top -> bitmap -> prefix -> every ctx's records into one device image of the three sections, on the first ctx's stream; one copy
//       per section lands behind the header.
//   mpmhip_snapshot_head / mpmhip_snapshot_rows_ranked   a rank per process, collective-free: the caller compares the heads, reduces
//       `top` and the bitmaps (mpmhip_live_id_top / mpmhip_id_bitmap) and places the rows by their numbers.
//   mpmhip_snapshot_load_brick   the blob goes through a staging buffer of bounded size in chunks of records (MPMHIP_SNAP_CHUNK, a
//       test knob read per call; 1 Mi records otherwise), twice: pass 1 counts (k_snap_own_count, k_seed_scan) and may refuse with
//       the ctx untouched, pass 2 emits (k_snap_own_emit) and replaces groups, particles and clocks.
//   mpmhip_snapshot_histogram    k_live_histogram over the staged chunks: what a restart on another rank count cuts its bricks from.
// Every device array is a DevBuf that lives for one call.

extern "C" {

// ------------------------------------------------------------------------------------------------ saving
// RecP.A current (as mpmhip_snapshot_save), apic_b current where the ctx keeps it, the stream drained, the counters read
static int sj_prepare(mpmhip_ctx *c, const char *who, Counters &hc) {
  if (int rc = fj_ctx_ok(c, who)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = read_counters(c, hc)) return rc;
  if (!c->rec.affine_valid()) {
    hipLaunchKernelGGL(k_affine, dim3(particle_grid(c->n_slots)), dim3(256), 0, c->stream, c->P, c->rg, c->rp, c->rb, c->d_groups);
    if (int rc = launch_check(c, "k_affine")) return rc;
    c->rec.affine_rebuilt();
  }
  if (c->P.store_b)
    if (int rc = ensure_b_current(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MPMHIP_OK;
}
// the header of this ctx alone: its own live records, no dead slot
static snap::SnapHeader sj_head(const mpmhip_ctx *c, const Counters &hc) {
  snap::SnapHeader h;
  memset(&h, 0, sizeof h);
  memcpy(h.magic, "MPMHIP01", 8);
  h.abi = MPMHIP_ABI_VERSION; h.n_groups = (uint32_t)c->groups.size();
  h.n_slots = c->n_slots - (int64_t)hc.n_dead; h.substeps = c->substeps; h.next_pid = c->next_pid;
  h.b_stale = c->P.store_b ? 0 : (c->rec.b_stale() ? 1 : 0); h.store_b = c->P.store_b;
  for (int k = 0; k < 3; k++) h.res[k] = c->P.res[k];
  h.t = c->t; h.request_t = c->request_t; h.dx = c->P.dx; h.dt = c->P.dt; h.n_dead = 0;
  return h;
}
// the first field in which rank r differs from rank 0 (nullptr: none)
static const char *sj_differs(const snap::SnapHeader &a, const snap::SnapHeader &b, const std::vector<GroupParams> &ga, const std::vector<GroupParams> &gb) {
  if (a.substeps != b.substeps) return "substeps";
  if (memcmp(&a.t, &b.t, sizeof a.t) != 0) return "t";
  if (memcmp(&a.request_t, &b.request_t, sizeof a.request_t) != 0) return "request_t";
  if (memcmp(&a.dx, &b.dx, sizeof a.dx) != 0) return "dx";
  if (memcmp(&a.dt, &b.dt, sizeof a.dt) != 0) return "dt";
  if (memcmp(a.res, b.res, sizeof a.res) != 0) return "res";
  if (a.store_b != b.store_b) return "store_b";
  if (a.b_stale != b.b_stale) return "b_stale";
  if (ga.size() != gb.size() || (ga.size() && memcmp(ga.data(), gb.data(), ga.size() * sizeof(GroupParams)) != 0)) return "group table";
  return nullptr;
}
static snap::Layout3D sj_layout(uint64_t n_groups, uint64_t n_rows) {
  snap::Counts3D n;
  n.n_groups = n_groups; n.n_slots = n_rows;
  snap::Layout3D L;
  snap::layout3d(n, snap::NO_LIMIT, L);
  return L;
}
// the records of `of` to their ranks in P; with `job` also the number of each row in the job's blob
static int sj_rows(mpmhip_ctx *c, FrameRank &P, uint32_t n_rows, float4 *img, FrameRank *job, uint32_t *row_index, hipStream_t st, mpmhip_ctx *of) {
  if (of->n_slots <= 0 || !n_rows) return MPMHIP_OK;
  snap_launch_rows(st, particle_grid(of->n_slots * 4), (uint32_t)of->n_slots, (const float4 *)of->rg.get(), (const float4 *)of->rp.get(),
                   (const float4 *)of->rb.get(), P.top, (const uint32_t *)P.bits, (const uint32_t *)P.prefix, n_rows, img, img + (size_t)n_rows * 4,
                   img + (size_t)n_rows * 8, (const uint32_t *)(job ? job->bits.get() : nullptr), (const uint32_t *)(job ? job->prefix.get() : nullptr),
                   row_index, reinterpret_cast<int32_t *>(P.small.get() + 2));
  return launch_check(c, "k_snap_rows_ranked");
}

int mpmhip_snapshot_size_group(mpmhip_ctx *const *ctxs, int32_t K, size_t *bytes) {
  int rc = fj_check_group(ctxs, K, "snapshot_size_group");
  if (rc || !bytes) return rc ? rc : MPMHIP_EINVAL;
  int64_t n = 0;
  for (int r = 0; r < K; r++) {
    const int64_t m = mpmhip_num_particles(ctxs[r]);  // (synchronises the ctx)
    if (m < 0) return (int)m;
    n += m;
  }
  *bytes = (size_t)sj_layout(ctxs[0]->groups.size(), (uint64_t)n).total;
  return MPMHIP_OK;
}

int mpmhip_snapshot_save_group(mpmhip_ctx *const *ctxs, int32_t K, void *dst, size_t capacity, size_t *written) {
  int rc = fj_check_group(ctxs, K, "snapshot_save_group");
  if (rc || !dst || !written) return rc ? rc : MPMHIP_EINVAL;
  mpmhip_ctx *c = ctxs[0];
  std::vector<snap::SnapHeader> heads((size_t)K);
  for (int r = 0; r < K; r++) {  // every ctx's records are final before the first ctx's stream reads them
    Counters hc;
    if ((rc = sj_prepare(ctxs[r], "snapshot_save_group", hc))) return rc;
    heads[(size_t)r] = sj_head(ctxs[r], hc);
  }
  for (int r = 1; r < K; r++)
    if (const char *what = sj_differs(heads[0], heads[(size_t)r], c->groups, ctxs[r]->groups))
      return fail(ctxs[r], MPMHIP_EINVAL, "snapshot_save_group: %s of rank %d differs from rank 0's (a job's snapshot has one clock, one grid and one group table)", what, r);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  FrameRank R;
  if ((rc = fj_begin(c, R, st))) return rc;
  for (int r = 0; r < K; r++)
    if ((rc = fj_top(c, R, st, ctxs[r]))) return rc;
  if ((rc = fj_read_top(c, R, st)) || (rc = fj_alloc_bits(c, R, st, R.top, nullptr))) return rc;
  for (int r = 0; r < K; r++)
    if ((rc = fj_mark(c, R, st, ctxs[r]))) return rc;
  if ((rc = fj_prefix(c, R, st)) || (rc = fj_read_small(c, R, st))) return rc;
  if (R.err[FRAME_ERR_TWICE] >= 0)
    return fail(c, MPMHIP_EINVAL, "snapshot_save_group: creation id %d is held twice among the %d ctx (a snapshot has one record per id)", R.err[FRAME_ERR_TWICE], K);
  if (R.err[FRAME_ERR_RANGE] >= 0 || R.set != R.live)
    return fail(c, MPMHIP_EINVAL, "internal: snapshot_save_group marked %u ids of %u live slots below %u (id %d out of range)", R.set, R.live, R.top, R.err[FRAME_ERR_RANGE]);
  if (R.top > 0x7fffffffu) return fail(c, MPMHIP_EINVAL, "snapshot_save_group: the largest creation id leaves no next id");
  const uint32_t n = R.set;
  const snap::Layout3D L = sj_layout(c->groups.size(), n);
  if (L.total > capacity) return fail(c, MPMHIP_ECAPACITY, "snapshot buffer too small: %zu < %zu", capacity, (size_t)L.total);
  DevBuf<float4> img;  // the three sections as the blob has them: rg [n][4] | rp [n][4] | rb [n][3]
  if (n) {
    HIPCHK(c, img.alloc((size_t)n * SNAP_REC_F4));
    for (int r = 0; r < K; r++)
      if ((rc = sj_rows(c, R, n, img, nullptr, nullptr, st, ctxs[r]))) return rc;
    if ((rc = fj_read_small(c, R, st))) return rc;  // (before the first byte reaches dst)
    if (R.err[FRAME_ERR_RANGE] >= 0 || R.err[FRAME_ERR_ABSENT] >= 0)
      return fail(c, MPMHIP_EINVAL, "snapshot_save_group: the particles changed between the ranking and the rows (id %d)",
                  std::max(R.err[FRAME_ERR_RANGE], R.err[FRAME_ERR_ABSENT]));
    char *out = static_cast<char *>(dst);
    HIPCHK(c, hipMemcpyAsync(out + L.rg.off, img.get(), L.rg.len, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(out + L.rp.off, img.get() + (size_t)n * 4, L.rp.len, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(out + L.rb.off, img.get() + (size_t)n * 8, L.rb.len, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
  }
  snap::SnapHeader h = heads[0];
  h.n_slots = (int64_t)n;
  for (int r = 0; r < K; r++) h.next_pid = std::max(h.next_pid, heads[(size_t)r].next_pid);
  h.next_pid = std::max(h.next_pid, (int32_t)R.top);
  snap_put(dst, L.header, &h);
  snap_put(dst, L.groups, c->groups.data());
  *written = (size_t)L.total;
  return MPMHIP_OK;
}

int mpmhip_snapshot_head(mpmhip_ctx *c, void *dst, size_t capacity, size_t *bytes) {
  if (!c || !bytes) return MPMHIP_EINVAL;
  Counters hc;
  if (int rc = sj_prepare(c, "snapshot_head", hc)) return rc;
  const snap::Layout3D L = sj_layout(c->groups.size(), 0);
  *bytes = (size_t)L.total;
  if (!dst) return MPMHIP_OK;  // (the size only)
  if (L.total > capacity) return fail(c, MPMHIP_ECAPACITY, "snapshot_head: %zu bytes, the buffer holds %zu", (size_t)L.total, capacity);
  const snap::SnapHeader h = sj_head(c, hc);
  snap_put(dst, L.header, &h);
  snap_put(dst, L.groups, c->groups.data());
  return MPMHIP_OK;
}

int mpmhip_snapshot_rows_ranked(mpmhip_ctx *c, int64_t top, const uint32_t *union_words_host, void *rows_host, uint32_t *row_index_host,
                                int64_t capacity_rows, int64_t *written) {
  if (!c || !written || capacity_rows < 0 || (top > 0 && !union_words_host)) return MPMHIP_EINVAL;
  FrameRank R, U;
  Counters hc;
  int rc;
  if ((rc = sj_prepare(c, "snapshot_rows_ranked", hc)) || (rc = fj_own_bitmap(c, R, top, true, "snapshot_rows_ranked"))) return rc;
  const uint32_t n = R.n_words ? R.set : 0u;
  *written = 0;
  if ((int64_t)n > capacity_rows) return fail(c, MPMHIP_ECAPACITY, "snapshot_rows_ranked: %u rows, the buffers hold %lld", n, (long long)capacity_rows);
  if (!n) return MPMHIP_OK;
  if (!rows_host || !row_index_host) return MPMHIP_EINVAL;
  if ((rc = fj_alloc_bits(c, U, c->stream, (uint32_t)top, union_words_host)) || (rc = fj_prefix(c, U, c->stream))) return rc;
  DevBuf<float4> img;
  DevBuf<uint32_t> d_index;
  HIPCHK(c, img.alloc((size_t)n * SNAP_REC_F4));
  HIPCHK(c, d_index.alloc(n));
  if ((rc = sj_rows(c, R, n, img, &U, d_index, c->stream, c)) || (rc = fj_read_small(c, R, c->stream))) return rc;
  if (R.err[FRAME_ERR_ABSENT] >= 0 || R.err[FRAME_ERR_RANGE] >= 0)
    return fail(c, MPMHIP_EINVAL, "snapshot_rows_ranked: creation id %d of this ctx is missing from the job's bitmap", std::max(R.err[FRAME_ERR_ABSENT], R.err[FRAME_ERR_RANGE]));
  std::vector<float4> h((size_t)n * SNAP_REC_F4);
  HIPCHK(c, hipMemcpy(h.data(), img, h.size() * sizeof(float4), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(row_index_host, d_index, (size_t)n * 4, hipMemcpyDeviceToHost));
  char *out = static_cast<char *>(rows_host);  // [n][176]: rg | rp | rb of each row
  const size_t row = snap::RECG_BYTES + snap::RECP_BYTES + snap::BROW_BYTES;
  for (size_t j = 0; j < n; j++) {
    memcpy(out + j * row, &h[j * 4], snap::RECG_BYTES);
    memcpy(out + j * row + snap::RECG_BYTES, &h[(size_t)n * 4 + j * 4], snap::RECP_BYTES);
    memcpy(out + j * row + snap::RECG_BYTES + snap::RECP_BYTES, &h[(size_t)n * 8 + j * 3], snap::BROW_BYTES);
  }
  *written = (int64_t)n;
  return MPMHIP_OK;
}

// ------------------------------------------------------------------------------------------------ loading
static int64_t sj_chunk_records() {
  int64_t n = 1ll << 20;
  if (const char *e = getenv("MPMHIP_SNAP_CHUNK")) {
    const long long v = atoll(e);
    if (v >= 1 && v <= (1ll << 24)) n = v;
  }
  return n;
}
static int sj_check_blob(mpmhip_ctx *c, const void *src, size_t size, snap::Blob3D &B) {
  snap::Facts f;
  for (int k = 0; k < 3; k++) f.res[k] = c->P.res[k];
  f.dx = c->P.dx; f.dt = c->P.dt; f.groups_cap = c->groups_cap;
  const snap::Verdict v = snap::check3d_brick(src, size, f, B);
  return v.ok() ? MPMHIP_OK : fail(c, v.rc, "%s", v.msg.c_str());
}
// the staging buffer of a call: `chunk` records of each section
struct SnapStage {
  DevBuf<float4> buf;
  int64_t chunk = 0, n_chunks = 0;
  float4 *rg() const { return buf.get(); }
  float4 *rp() const { return buf.get() + (size_t)chunk * 4; }
  float4 *rb() const { return buf.get() + (size_t)chunk * 8; }
  int64_t first(int64_t k) const { return k * chunk; }
  int64_t count(int64_t k, int64_t n) const { return std::min(chunk, n - k * chunk); }
};
static int sj_stage_alloc(mpmhip_ctx *c, SnapStage &S, int64_t n_slots, bool all_sections) {
  S.chunk = std::max<int64_t>(1, std::min(sj_chunk_records(), n_slots));
  S.n_chunks = (n_slots + S.chunk - 1) / S.chunk;
  HIPCHK(c, S.buf.alloc((size_t)S.chunk * (all_sections ? SNAP_REC_F4 : 4)));
  return MPMHIP_OK;
}
static hipError_t sj_stage(float4 *dev, const void *blob, snap::Sec s, uint64_t each, int64_t first, int64_t count, hipStream_t st) {
  return hipMemcpyAsync(dev, (const char *)blob + s.off + each * (uint64_t)first, each * (uint64_t)count, hipMemcpyHostToDevice, st);
}

int mpmhip_snapshot_load_brick(mpmhip_ctx *c, const void *src, size_t size, int64_t info[4]) {
  if (!c || !src || !info) return MPMHIP_EINVAL;
  for (int k = 0; k < 4; k++) info[k] = 0;
  if (int rc = fj_ctx_ok(c, "snapshot_load_brick")) return rc;
  if (!c->T.enabled) return fail(c, MPMHIP_EINVAL, "snapshot_load_brick: the ctx has no partition (mpmhip_set_partition or mpmhip_tiled_setup first)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  snap::Blob3D B;
  if (int rc = sj_check_blob(c, src, size, B)) return rc;
  const snap::SnapHeader &h = B.h;
  const snap::Layout3D &L = B.L;
  const int64_t n_slots = h.n_slots;
  hipStream_t st = c->stream;
  int rc;
  // ---- pass 1: count (nothing of the ctx is written)
  SnapStage S;
  if ((rc = sj_stage_alloc(c, S, n_slots, true))) return rc;
  const uint32_t spans_per_chunk = snap_spans((uint32_t)S.chunk);
  const uint64_t n_spans = (uint64_t)S.n_chunks * spans_per_chunk;
  if (n_spans >= (1ull << 31)) return fail(c, MPMHIP_EINVAL, "snapshot_load_brick: MPMHIP_SNAP_CHUNK = %lld cuts the blob into too many chunks", (long long)S.chunk);
  DevBuf<uint32_t> totals, small;
  HIPCHK(c, totals.alloc((size_t)n_spans + 1));
  HIPCHK(c, small.alloc(SNAP_WORDS));
  HIPCHK(c, hipMemsetAsync(totals, 0, ((size_t)n_spans + 1) * 4, st));
  uint32_t w[SNAP_WORDS] = {0u, 0u, 0xFFFFFFFFu, 1u << 30, 1u << 30, 1u << 30, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  HIPCHK(c, hipMemcpyAsync(small, w, sizeof w, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipStreamSynchronize(st));  // (w is a stack array)
  for (int64_t k = 0; k < S.n_chunks; k++) {
    const int64_t nk = S.count(k, n_slots);
    HIPCHK(c, sj_stage(S.rg(), src, L.rg, snap::RECG_BYTES, S.first(k), nk, st));
    snap_launch_own_count(st, c->P, c->T, (uint32_t)nk, S.rg(), totals.get() + (size_t)k * spans_per_chunk, small.get());
    if ((rc = launch_check(c, "k_snap_own_count"))) return rc;
  }
  uint32_t kept = 0;
  if (n_spans) {
    hipLaunchKernelGGL(k_seed_scan, dim3(1), dim3(SEED_SCAN_WG), 0, st, totals.get(), (uint32_t)n_spans, totals.get() + n_spans);
    if ((rc = launch_check(c, "k_seed_scan"))) return rc;
    HIPCHK(c, hipMemcpyAsync(&kept, totals.get() + n_spans, 4, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(c, hipMemcpyAsync(w, small, sizeof w, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const int64_t live = w[SNAP_W_LIVE], lost = w[SNAP_W_LOST];
  info[1] = live; info[3] = lost;
  if ((int64_t)kept > c->cap) {
    info[2] = kept;
    return fail(c, MPMHIP_ECAPACITY, "snapshot_load_brick: rank %d owns %u of the snapshot's %lld particles, its capacity is %lld (mpmhip_reserve, then repeat "
                "the call on every rank); nothing was loaded", c->T.rank, kept, (long long)live, (long long)c->cap);
  }
  // ---- pass 2: the blob's groups, this brick's records and the blob's clocks replace the ctx's
  c->groups = snap_groups(src, L.groups);
  HIPCHK(c, snap_to_dev(c->d_groups, src, L.groups));
  for (int64_t k = 0; k < S.n_chunks && kept; k++) {
    const int64_t nk = S.count(k, n_slots);
    HIPCHK(c, sj_stage(S.rg(), src, L.rg, snap::RECG_BYTES, S.first(k), nk, st));
    HIPCHK(c, sj_stage(S.rp(), src, L.rp, snap::RECP_BYTES, S.first(k), nk, st));
    HIPCHK(c, sj_stage(S.rb(), src, L.rb, snap::BROW_BYTES, S.first(k), nk, st));
    snap_launch_own_emit(st, c->P, c->T, (uint32_t)nk, S.rg(), S.rp(), S.rb(), totals.get() + (size_t)k * spans_per_chunk, kept, (float4 *)c->rg.get(),
                         (float4 *)c->rp.get(), (float4 *)c->rb.get(), small.get());
    if ((rc = launch_check(c, "k_snap_own_emit"))) return rc;
  }
  int32_t emit_err = -1;
  HIPCHK(c, hipMemcpyAsync(&emit_err, small.get() + SNAP_W_ERR, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  set_slots(c, kept);
  c->substeps = h.substeps; c->next_pid = h.next_pid;  // (the header's next id on every rank: later brick seeding stays a collective that agrees)
  c->t = h.t; c->request_t = h.request_t;
  if ((rc = clear_block_flags(c, c->rec.snapshot_loaded(h.b_stale != 0 || h.store_b == 0)))) return rc;
  Counters hc;
  memset(&hc, 0, sizeof hc);
  HIPCHK(c, hipMemcpy(c->cnt, &hc, sizeof hc, hipMemcpyHostToDevice));
  if (emit_err >= 0) return fail(c, MPMHIP_EINVAL, "internal: snapshot_load_brick placed a record at slot %d of %u (the blob changed between the passes)", emit_err, kept);
  if (c->P.store_b && c->rec.b_stale())  // this ctx keeps apic_b: rebuild it from A once
    if ((rc = ensure_b_current(c))) return rc;
  info[0] = kept;
  if (c->tn.on) {  // as behind a re-cut (tn_recut_done): the clip box from the joint bounds every rank computed, the plan stale
    auto &N = c->tn;
    if (live - lost > 0) {
      const int s = tplan::clip_slack(c->T.margin);
      for (int a = 0; a < 3; a++) {
        const int lo = std::min(std::max((int)w[SNAP_W_BOUNDS + a], 0), c->P.res[a]), hi = std::min(std::max((int)w[SNAP_W_BOUNDS + 3 + a], lo), c->P.res[a]);
        N.clip_lo[a] = std::max(0, lo - s);
        N.clip_hi[a] = std::min(c->P.res[a] + 1, hi + s + 2);
      }
    }
    N.occ_valid = false;
    return tn_apply_plan(c);  // (synchronises)
  }
  return MPMHIP_OK;
}

int mpmhip_snapshot_histogram(mpmhip_ctx *c, const void *src, size_t size, int64_t *hist_x, int64_t *hist_y, int64_t *hist_z, int32_t lo[3], int32_t hi[3],
                              int64_t *total) {
  if (!c || !src) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  snap::Blob3D B;
  if (int rc = sj_check_blob(c, src, size, B)) return rc;
  const int64_t n_slots = B.h.n_slots;
  hipStream_t st = c->stream;
  const int *res = c->P.res;
  const size_t bins = (size_t)res[0] + res[1] + res[2], words = bins + 1 + 3;  // mpmhip_live_histogram's device words
  DevBuf<unsigned long long> d;
  HIPCHK(c, d.alloc(words));
  std::vector<unsigned long long> h(words, 0ull);
  const int init[6] = {1 << 30, 1 << 30, 1 << 30, -1, -1, -1};
  memcpy(&h[bins + 1], init, sizeof init);
  HIPCHK(c, hipMemcpyAsync(d, h.data(), sizeof(unsigned long long) * words, hipMemcpyHostToDevice, st));
  SnapStage S;
  if (int rc = sj_stage_alloc(c, S, n_slots, false)) return rc;
  const size_t lds = sizeof(int32_t) * bins;
  int *bounds = reinterpret_cast<int *>(d.get() + bins + 1);
  for (int64_t k = 0; k < S.n_chunks; k++) {
    const int64_t nk = S.count(k, n_slots);
    HIPCHK(c, sj_stage(S.rg(), src, B.L.rg, snap::RECG_BYTES, S.first(k), nk, st));
    Params P = c->P;
    P.n_slots = (uint32_t)nk;
    const int grid = std::max(1, std::min(particle_grid(nk), 2 * std::max(1, (int)c->n_cus)));
    if (lds <= 65536 - 256)
      hipLaunchKernelGGL(k_live_histogram<true>, dim3(grid), dim3(256), lds, st, P, (const float4 *)S.rg(), d.get(), bounds);
    else
      hipLaunchKernelGGL(k_live_histogram<false>, dim3(grid), dim3(256), 0, st, P, (const float4 *)S.rg(), d.get(), bounds);
    if (int rc = launch_check(c, "live_histogram (snapshot)")) return rc;
  }
  HIPCHK(c, hipMemcpyAsync(h.data(), d, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  int64_t *out[3] = {hist_x, hist_y, hist_z};
  size_t at = 0;
  for (int a = 0; a < 3; at += (size_t)res[a], a++)
    if (out[a]) for (int i = 0; i < res[a]; i++) out[a][i] = (int64_t)h[at + (size_t)i];
  const int64_t n = (int64_t)h[bins];
  if (total) *total = n;
  int b[6];
  memcpy(b, &h[bins + 1], sizeof b);
  for (int k = 0; k < 3; k++) {
    if (lo) lo[k] = n ? b[k] : 0;
    if (hi) hi[k] = n ? b[3 + k] : 0;
  }
  return MPMHIP_OK;
}

}  // extern "C"
