// taichi_mpm_amd/csrc/frame_job_api.h — the .bgeo frame of a whole tiled job (MPM<dim>::write_partio, src/visualize.cpp:17-100: ONE
// file, the rows of all particles in ascending creation id) from the ctx that hold its ranks — included by mpmhip.hip inside
// extern "C".  Kernels: k_frame.h, compiled by k_frame.hip and launched through frame_launch.h.  Off the hot path.
//   mpmhip_bgeo_size_group / mpmhip_bgeo_encode_group   the K ctx of one process on one device: top -> one bitmap all ctx mark ->
//       one prefix -> every ctx's rows into one device row buffer -> one copy behind the header.  All on the first ctx's stream,
//       after every ctx's own stream has drained.
//   mpmhip_live_id_top / mpmhip_id_bitmap / mpmhip_bgeo_rows_ranked   a rank per process: the same in three collective-free steps;
//       the caller reduces `top` (max) and the bitmaps (or) between them and places the rows by their index.
//   mpmhip_bgeo_envelope   what stands before and behind the rows, host only.
// Every device array is a DevBuf that lives for one call.

struct FrameRank {  // one ranking: the small words, the bitmap, its prefix
  DevBuf<uint32_t> small;  // [0] top, [1] live slots that marked, [2 + FRAME_ERR_*] the error words
  DevBuf<uint32_t> bits, prefix, sums;
  uint32_t top = 0, n_words = 0, n_blocks = 0, live = 0, set = 0;
  int32_t err[FRAME_ERR_WORDS] = {-1, -1, -1};
};
static constexpr int FRAME_SMALL = 2 + FRAME_ERR_WORDS;
static double g_frame_ms[5] = {0, 0, 0, 0, 0};  // top / mark / prefix / rows / copy of the last mpmhip_bgeo_encode_group

static int fj_ctx_ok(mpmhip_ctx *c, const char *who) {
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "%s inside a substep", who);
  if (c->rigid.enabled) return fail(c, MPMHIP_EINVAL, "%s: a ctx with rigid bodies (their boundary particles are rows of mpmhip_bgeo_encode only)", who);
  if (c->async.resident) return fail(c, MPMHIP_EINVAL, "%s: a ctx with a resident asynchronous stepper", who);
  return MPMHIP_OK;
}
static int fj_begin(mpmhip_ctx *c, FrameRank &R, hipStream_t st) {
  HIPCHK(c, R.small.alloc(FRAME_SMALL));
  const uint32_t init[FRAME_SMALL] = {0u, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  HIPCHK(c, hipMemcpyAsync(R.small, init, sizeof init, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipStreamSynchronize(st));  // (init is a stack array)
  return MPMHIP_OK;
}
static int fj_read_small(mpmhip_ctx *c, FrameRank &R, hipStream_t st) {
  uint32_t h[FRAME_SMALL];
  HIPCHK(c, hipMemcpyAsync(h, R.small, sizeof h, hipMemcpyDeviceToHost, st));
  if (R.sums) HIPCHK(c, hipMemcpyAsync(&R.set, R.sums.get() + R.n_blocks, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  R.live = h[1];
  for (int k = 0; k < FRAME_ERR_WORDS; k++) R.err[k] = (int32_t)h[2 + k];
  return MPMHIP_OK;
}
static int fj_top(mpmhip_ctx *c, FrameRank &R, hipStream_t st, mpmhip_ctx *of) {
  if (of->n_slots <= 0) return MPMHIP_OK;
  frame_launch_top(st, particle_grid(of->n_slots), (uint32_t)of->n_slots, (const RecG *)of->rg, R.small.get());
  return launch_check(c, "k_live_id_top");
}
static int fj_read_top(mpmhip_ctx *c, FrameRank &R, hipStream_t st) {
  HIPCHK(c, hipMemcpyAsync(&R.top, R.small, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return MPMHIP_OK;
}
static int fj_alloc_bits(mpmhip_ctx *c, FrameRank &R, hipStream_t st, uint32_t top, const uint32_t *words_host) {
  R.top = top;
  R.n_words = (uint32_t)(((uint64_t)top + 31) / 32);
  R.n_blocks = (R.n_words + FRAME_WG - 1) / FRAME_WG;
  if (!R.n_words) return MPMHIP_OK;
  HIPCHK(c, R.bits.alloc(R.n_words));
  if (words_host) HIPCHK(c, hipMemcpyAsync(R.bits, words_host, (size_t)R.n_words * 4, hipMemcpyHostToDevice, st));
  else HIPCHK(c, hipMemsetAsync(R.bits, 0, (size_t)R.n_words * 4, st));
  return MPMHIP_OK;
}
static int fj_mark(mpmhip_ctx *c, FrameRank &R, hipStream_t st, mpmhip_ctx *of) {
  if (of->n_slots <= 0 || !R.n_words) return MPMHIP_OK;
  frame_launch_mark(st, particle_grid(of->n_slots), (uint32_t)of->n_slots, (const RecG *)of->rg, R.top, R.bits.get(), R.small.get() + 1,
                    reinterpret_cast<int32_t *>(R.small.get() + 2));
  return launch_check(c, "k_id_mark");
}
static int fj_prefix(mpmhip_ctx *c, FrameRank &R, hipStream_t st) {
  if (!R.n_words) return MPMHIP_OK;
  HIPCHK(c, R.sums.alloc((size_t)R.n_blocks + 1));
  HIPCHK(c, R.prefix.alloc(R.n_words));
  frame_launch_prefix(st, R.n_words, R.n_blocks, (const uint32_t *)R.bits, R.sums.get(), R.prefix.get());
  return launch_check(c, "k_id_prefix");
}
// the rows of `of`: placed by P; with `job` also the index of each in the job's file
static int fj_rows(mpmhip_ctx *c, bool verbose, FrameRank &P, uint32_t n_rows, uint32_t *rows, FrameRank *job, uint32_t *row_index, hipStream_t st,
                   mpmhip_ctx *of) {
  if (of->n_slots <= 0 || !n_rows) return MPMHIP_OK;
  const int32_t *limits = of->async.enabled && of->async.limits_valid ? of->async.d_particle_limits.get() : nullptr;
  frame_launch_rows(st, particle_grid(of->n_slots), verbose, (uint32_t)of->n_slots, (const RecG *)of->rg, (const RecP *)of->rp, (const float *)of->rb,
                    (const GroupParams *)of->d_groups, limits, P.top, (const uint32_t *)P.bits, (const uint32_t *)P.prefix, n_rows, rows,
                    (const uint32_t *)(job ? job->bits.get() : nullptr), (const uint32_t *)(job ? job->prefix.get() : nullptr), row_index,
                    reinterpret_cast<int32_t *>(P.small.get() + 2));
  return launch_check(c, "k_bgeo_rows_ranked");
}

static int fj_check_group(mpmhip_ctx *const *ctxs, int32_t K, const char *who) {
  if (!ctxs || K < 1) return MPMHIP_EINVAL;
  for (int r = 0; r < K; r++)
    if (!ctxs[r]) return MPMHIP_EINVAL;
  for (int r = 0; r < K; r++) {
    mpmhip_ctx *c = ctxs[r];
    if (int rc = fj_ctx_ok(c, who)) return rc;
    if (c->device != ctxs[0]->device) return fail(c, MPMHIP_EINVAL, "%s: ctx %d is on device %d, ctx 0 on device %d", who, r, c->device, ctxs[0]->device);
    for (int a = 0; a < 3; a++)
      if (c->P.res[a] != ctxs[0]->P.res[a])
        return fail(c, MPMHIP_EINVAL, "%s: ctx %d has res (%d, %d, %d), ctx 0 (%d, %d, %d)", who, r, c->P.res[0], c->P.res[1], c->P.res[2],
                    ctxs[0]->P.res[0], ctxs[0]->P.res[1], ctxs[0]->P.res[2]);
  }
  return MPMHIP_OK;
}

int mpmhip_bgeo_size_group(mpmhip_ctx *const *ctxs, int32_t K, int32_t verbose, size_t *bytes) {
  int rc = fj_check_group(ctxs, K, "bgeo_size_group");
  if (rc || !bytes) return rc ? rc : MPMHIP_EINVAL;
  int64_t n = 0;
  for (int r = 0; r < K; r++) {
    const int64_t m = mpmhip_num_particles(ctxs[r]);  // (synchronises the ctx)
    if (m < 0) return (int)m;
    n += m;
  }
  if (n > 0x7FFFFFFFll) return fail(ctxs[0], MPMHIP_EINVAL, "bgeo_size_group: %lld particles, a .bgeo file holds 2^31 - 1", (long long)n);
  *bytes = bgeo_bytes((uint32_t)n, verbose != 0);
  return MPMHIP_OK;
}

int mpmhip_bgeo_encode_group(mpmhip_ctx *const *ctxs, int32_t K, int32_t verbose, void *dst, size_t capacity, size_t *written) {
  int rc = fj_check_group(ctxs, K, "bgeo_encode_group");
  if (rc || !dst || !written) return rc ? rc : MPMHIP_EINVAL;
  mpmhip_ctx *c = ctxs[0];
  HIPCHK(c, hipSetDevice(c->device));
  for (int r = 0; r < K; r++) {  // every ctx's records are final before the first ctx's stream reads them
    if (verbose) { if ((rc = ensure_b_current(ctxs[r]))) return rc; }
    HIPCHK(ctxs[r], hipStreamSynchronize(ctxs[r]->stream));
  }
  hipStream_t st = c->stream;
  struct Events {  // phase marks on the stream (mpmhip_debug_frame_phases)
    hipEvent_t e[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~Events() { for (auto v : e) if (v) (void)hipEventDestroy(v); }
  } ev;
  for (auto &v : ev.e) HIPCHK(c, hipEventCreate(&v));
  FrameRank R;
  if ((rc = fj_begin(c, R, st))) return rc;
  HIPCHK(c, hipEventRecord(ev.e[0], st));
  for (int r = 0; r < K; r++)
    if ((rc = fj_top(c, R, st, ctxs[r]))) return rc;
  HIPCHK(c, hipEventRecord(ev.e[1], st));
  if ((rc = fj_read_top(c, R, st)) || (rc = fj_alloc_bits(c, R, st, R.top, nullptr))) return rc;
  for (int r = 0; r < K; r++)
    if ((rc = fj_mark(c, R, st, ctxs[r]))) return rc;
  HIPCHK(c, hipEventRecord(ev.e[2], st));
  if ((rc = fj_prefix(c, R, st))) return rc;
  HIPCHK(c, hipEventRecord(ev.e[3], st));
  if ((rc = fj_read_small(c, R, st))) return rc;
  if (R.err[FRAME_ERR_TWICE] >= 0)
    return fail(c, MPMHIP_EINVAL, "bgeo_encode_group: creation id %d is held twice among the %d ctx (a frame has one row per id)", R.err[FRAME_ERR_TWICE], K);
  if (R.err[FRAME_ERR_RANGE] >= 0 || R.set != R.live)
    return fail(c, MPMHIP_EINVAL, "internal: bgeo_encode_group marked %u ids of %u live slots below %u (id %d out of range)", R.set, R.live, R.top, R.err[FRAME_ERR_RANGE]);
  const uint32_t n = R.set;
  const size_t total = bgeo_bytes(n, verbose != 0);
  if (total > capacity) return fail(c, MPMHIP_ECAPACITY, "bgeo image needs %zu bytes, the buffer holds %zu", total, capacity);
  const size_t W = verbose ? BGEO_W_VERBOSE : BGEO_W_PLAIN;
  const std::vector<uint8_t> head = bgeo_header(n, verbose != 0);
  uint8_t *out = static_cast<uint8_t *>(dst) + head.size();
  DevBuf<uint32_t> d_rows;
  HIPCHK(c, hipEventRecord(ev.e[4], st));
  if (n) {
    HIPCHK(c, d_rows.alloc((size_t)n * W));
    for (int r = 0; r < K; r++)
      if ((rc = fj_rows(c, verbose != 0, R, n, d_rows, nullptr, nullptr, st, ctxs[r]))) return rc;
  }
  HIPCHK(c, hipEventRecord(ev.e[5], st));
  if (n) {
    if ((rc = fj_read_small(c, R, st))) return rc;  // (before the first byte reaches dst)
    if (R.err[FRAME_ERR_RANGE] >= 0 || R.err[FRAME_ERR_ABSENT] >= 0)
      return fail(c, MPMHIP_EINVAL, "bgeo_encode_group: the particles changed between the ranking and the rows (id %d)",
                  std::max(R.err[FRAME_ERR_RANGE], R.err[FRAME_ERR_ABSENT]));
    HIPCHK(c, hipMemcpyAsync(out, d_rows, (size_t)n * W * 4, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(c, hipEventRecord(ev.e[6], st));
  HIPCHK(c, hipStreamSynchronize(st));
  std::memcpy(dst, head.data(), head.size());
  out = bgeo_put_tail(out + (size_t)n * W * 4, n);
  *written = (size_t)(out - static_cast<uint8_t *>(dst));
  if (*written != total) return fail(c, MPMHIP_EINVAL, "internal: bgeo image is %zu bytes, expected %zu", *written, total);
  const int pairs[5][2] = {{0, 1}, {1, 2}, {2, 3}, {4, 5}, {5, 6}};
  for (int k = 0; k < 5; k++) {
    float ms = 0.0f;
    g_frame_ms[k] = hipEventElapsedTime(&ms, ev.e[pairs[k][0]], ev.e[pairs[k][1]]) == hipSuccess ? (double)ms : -1.0;
  }
  return MPMHIP_OK;
}

int mpmhip_debug_frame_phases(double ms[5]) {
  if (!ms) return MPMHIP_EINVAL;
  for (int k = 0; k < 5; k++) ms[k] = g_frame_ms[k];
  return MPMHIP_OK;
}

// ---------------------------------------------------------------------------------------------- a rank per process
static int fj_one_ready(mpmhip_ctx *c, int32_t verbose, const char *who) {
  if (int rc = fj_ctx_ok(c, who)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (verbose)
    if (int rc = ensure_b_current(c)) return rc;
  return MPMHIP_OK;
}
int64_t mpmhip_live_id_top(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  FrameRank R;
  int rc;
  if ((rc = fj_one_ready(c, 0, "live_id_top")) || (rc = fj_begin(c, R, c->stream)) || (rc = fj_top(c, R, c->stream, c)) || (rc = fj_read_top(c, R, c->stream)))
    return rc;
  return (int64_t)R.top;
}
static int fj_own_bitmap(mpmhip_ctx *c, FrameRank &R, int64_t top, bool prefix, const char *who) {
  if (top < 0 || top > (1ll << 31)) return fail(c, MPMHIP_EINVAL, "%s: top = %lld (0 .. 2^31)", who, (long long)top);
  int rc;
  if ((rc = fj_begin(c, R, c->stream)) || (rc = fj_alloc_bits(c, R, c->stream, (uint32_t)top, nullptr)) || (rc = fj_mark(c, R, c->stream, c))) return rc;
  if (prefix && (rc = fj_prefix(c, R, c->stream))) return rc;
  if ((rc = fj_read_small(c, R, c->stream))) return rc;
  if (!R.n_words && c->n_slots > 0) {  // (top = 0: nothing was marked; any live particle is beyond it)
    const int64_t n = mpmhip_num_particles(c);
    if (n < 0) return (int)n;
    if (n > 0) return fail(c, MPMHIP_EINVAL, "%s: the ctx holds %lld particles, top = 0", who, (long long)n);
  }
  if (R.err[FRAME_ERR_RANGE] >= 0) return fail(c, MPMHIP_EINVAL, "%s: the ctx holds creation id %d, top = %lld", who, R.err[FRAME_ERR_RANGE], (long long)top);
  if (R.err[FRAME_ERR_TWICE] >= 0) return fail(c, MPMHIP_EINVAL, "%s: creation id %d is held twice on this ctx", who, R.err[FRAME_ERR_TWICE]);
  if (prefix && R.n_words && R.set != R.live) return fail(c, MPMHIP_EINVAL, "internal: %s marked %u ids of %u live slots", who, R.set, R.live);
  return MPMHIP_OK;
}
int mpmhip_id_bitmap(mpmhip_ctx *c, int64_t top, uint32_t *words_host, int64_t *live) {
  if (!c || !live || (top > 0 && !words_host)) return MPMHIP_EINVAL;
  FrameRank R;
  int rc;
  if ((rc = fj_one_ready(c, 0, "id_bitmap")) || (rc = fj_own_bitmap(c, R, top, false, "id_bitmap"))) return rc;
  if (R.n_words) HIPCHK(c, hipMemcpy(words_host, R.bits, (size_t)R.n_words * 4, hipMemcpyDeviceToHost));
  *live = (int64_t)R.live;
  return MPMHIP_OK;
}
int mpmhip_bgeo_rows_ranked(mpmhip_ctx *c, int32_t verbose, int64_t top, const uint32_t *union_words_host, void *rows_host, uint32_t *row_index_host,
                            int64_t capacity_rows, int64_t *written) {
  if (!c || !written || capacity_rows < 0 || (top > 0 && !union_words_host)) return MPMHIP_EINVAL;
  FrameRank R, U;
  int rc;
  if ((rc = fj_one_ready(c, verbose, "bgeo_rows_ranked")) || (rc = fj_own_bitmap(c, R, top, true, "bgeo_rows_ranked"))) return rc;
  const uint32_t n = R.n_words ? R.set : 0u;
  *written = 0;
  if ((int64_t)n > capacity_rows) return fail(c, MPMHIP_ECAPACITY, "bgeo_rows_ranked: %u rows, the buffers hold %lld", n, (long long)capacity_rows);
  if (!n) return MPMHIP_OK;
  if (!rows_host || !row_index_host) return MPMHIP_EINVAL;
  if ((rc = fj_alloc_bits(c, U, c->stream, (uint32_t)top, union_words_host)) || (rc = fj_prefix(c, U, c->stream))) return rc;
  const size_t W = verbose ? BGEO_W_VERBOSE : BGEO_W_PLAIN;
  DevBuf<uint32_t> d_rows, d_index;
  HIPCHK(c, d_rows.alloc((size_t)n * W));
  HIPCHK(c, d_index.alloc(n));
  if ((rc = fj_rows(c, verbose != 0, R, n, d_rows, &U, d_index, c->stream, c)) || (rc = fj_read_small(c, R, c->stream))) return rc;
  if (R.err[FRAME_ERR_ABSENT] >= 0 || R.err[FRAME_ERR_RANGE] >= 0)
    return fail(c, MPMHIP_EINVAL, "bgeo_rows_ranked: creation id %d of this ctx is missing from the job's bitmap", std::max(R.err[FRAME_ERR_ABSENT], R.err[FRAME_ERR_RANGE]));
  HIPCHK(c, hipMemcpy(rows_host, d_rows, (size_t)n * W * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(row_index_host, d_index, (size_t)n * 4, hipMemcpyDeviceToHost));
  *written = (int64_t)n;
  return MPMHIP_OK;
}

// host only: what bgeo_header writes before n rows, and bgeo_prim_attr with the point numbers and the file's end behind them
int mpmhip_bgeo_envelope(uint32_t n, int32_t verbose, void *head, size_t head_cap, size_t *head_bytes, void *tail, size_t tail_cap, size_t *tail_bytes) {
  if (!head_bytes || !tail_bytes) return MPMHIP_EINVAL;
  const std::vector<uint8_t> h = bgeo_header(n, verbose != 0);
  *head_bytes = h.size();
  *tail_bytes = bgeo_tail_bytes(n);
  if (!head && !tail) return MPMHIP_OK;  // (sizes only)
  if (!head || !tail) return MPMHIP_EINVAL;
  if (h.size() > head_cap || *tail_bytes > tail_cap)
    return fail(nullptr, MPMHIP_ECAPACITY, "bgeo_envelope: head %zu / tail %zu bytes, the buffers hold %zu / %zu", h.size(), *tail_bytes, head_cap, tail_cap);
  std::memcpy(head, h.data(), h.size());
  bgeo_put_tail(static_cast<uint8_t *>(tail), n);
  return MPMHIP_OK;
}
