// taichi_mpm_amd/csrc/fields_api.h — mpmhip_download_dev / mpmhip_upload_dev / mpmhip_download_grid_dev: the particle fields and the
// dense grid view between the ctx and caller-owned DEVICE arrays (include/mpmhip.h) — included by mpmhip.hip inside extern "C", behind
// frame_job_api.h, whose ranking steps (fj_*) give the id order.  Kernels: k_fields.h, compiled by k_frame.hip and launched through
// fields_launch.h.  Off the substep's path.
//   order 0   count per workgroup -> scan (one word read back: the live count, judged before anything is written) -> emit / put
//   order 1   top -> bitmap -> prefix (the small words read back: set bits against live slots = are the ids unique) -> emit / put
// Everything runs on the ctx's stream, which has drained when a call returns.  No record and no row passes through host memory:
// host_particle_bytes stays.  Every device array is a DevBuf that lives for one call.

// what every call refuses before it touches anything; T = the table as the kernels take it
static int fd_ready(mpmhip_ctx *c, const void *const tab[8], int32_t order, const char *who, FieldTable &T) {
  if (!tab) return fail(c, MPMHIP_EINVAL, "%s: the field table is NULL", who);
  bool any = false;
  for (int f = 0; f < 8; f++) {
    T.p[f] = const_cast<void *>(tab[f]);
    any = any || tab[f];
  }
  if (!any) return fail(c, MPMHIP_EINVAL, "%s: the field table names no field (eight NULLs)", who);
  if (order != 0 && order != 1) return fail(c, MPMHIP_EINVAL, "%s: unknown order %d (0 slot order, 1 ascending creation id)", who, order);
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "%s inside a substep", who);
  if (c->async.resident)
    return fail(c, MPMHIP_EINVAL, "%s: a ctx with a resident asynchronous stepper (its records only mirror the pools: use the host calls)", who);
  return MPMHIP_OK;
}
// slot order: offs[w] = live slots before workgroup w, live = all of them
static int fd_count(mpmhip_ctx *c, DevBuf<uint32_t> &offs, uint32_t &live) {
  live = 0;
  if (c->n_slots <= 0) return MPMHIP_OK;
  const uint32_t spans = fields_spans((uint32_t)c->n_slots);
  HIPCHK(c, offs.alloc((size_t)spans + 1));
  fields_launch_count(c->stream, (uint32_t)c->n_slots, (const RecG *)c->rg, offs.get());
  if (int rc = launch_check(c, "k_fields_count")) return rc;
  HIPCHK(c, hipMemcpyAsync(&live, offs.get() + spans, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MPMHIP_OK;
}
// id order: the ranking of the ctx's live ids, R.set of them; refused unless every live slot holds an id of its own
static int fd_rank(mpmhip_ctx *c, FrameRank &R, const char *who) {
  hipStream_t st = c->stream;
  int rc;
  if ((rc = fj_begin(c, R, st)) || (rc = fj_top(c, R, st, c)) || (rc = fj_read_top(c, R, st)) || (rc = fj_alloc_bits(c, R, st, R.top, nullptr)) ||
      (rc = fj_mark(c, R, st, c)) || (rc = fj_prefix(c, R, st)) || (rc = fj_read_small(c, R, st)))
    return rc;
  if (R.err[FRAME_ERR_TWICE] >= 0 || R.set != R.live)
    return fail(c, MPMHIP_EINVAL, "%s: the creation ids are not unique (%u live slots hold %u ids, id %d more than once): order 1 has one row per id",
                who, R.live, R.set, R.err[FRAME_ERR_TWICE]);
  if (R.err[FRAME_ERR_RANGE] >= 0) return fail(c, MPMHIP_EINVAL, "internal: %s marked id %d at or beyond top = %u", who, R.err[FRAME_ERR_RANGE], R.top);
  return MPMHIP_OK;
}

int64_t mpmhip_download_dev(mpmhip_ctx *c, void *const dst[8], int64_t n_capacity, int32_t order) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  FieldTable T;
  int rc = fd_ready(c, dst, order, "download_dev", T);
  if (rc) return rc;
  if (n_capacity < 0) return fail(c, MPMHIP_EINVAL, "download_dev: n_capacity = %lld", (long long)n_capacity);
  if (T.p[MPMHIP_F_B] && (rc = ensure_b_current(c))) return rc;
  const uint32_t n_slots = (uint32_t)c->n_slots;
  const float4 *rg = reinterpret_cast<const float4 *>(c->rg.get()), *rp = reinterpret_cast<const float4 *>(c->rp.get()),
               *rb = reinterpret_cast<const float4 *>(c->rb.get());
  if (order == 0) {
    DevBuf<uint32_t> offs;
    uint32_t live;
    if ((rc = fd_count(c, offs, live))) return rc;
    if ((int64_t)live > n_capacity) return fail(c, MPMHIP_ECAPACITY, "download buffer holds %lld particles, %u are alive", (long long)n_capacity, live);
    if (!live) return 0;
    fields_launch_emit(c->stream, n_slots, rg, rp, rb, offs.get(), live, T);
    if ((rc = launch_check(c, "k_fields_emit"))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return (int64_t)live;
  }
  FrameRank R;
  if ((rc = fd_rank(c, R, "download_dev"))) return rc;
  const uint32_t n = R.n_words ? R.set : 0u;
  if ((int64_t)n > n_capacity) return fail(c, MPMHIP_ECAPACITY, "download buffer holds %lld particles, %u are alive", (long long)n_capacity, n);
  if (!n) return 0;
  fields_launch_emit_ranked(c->stream, n_slots, rg, rp, rb, R.top, (const uint32_t *)R.bits, (const uint32_t *)R.prefix, n, T,
                            reinterpret_cast<int32_t *>(R.small.get() + 2));
  if ((rc = launch_check(c, "k_fields_emit_ranked")) || (rc = fj_read_small(c, R, c->stream))) return rc;
  if (R.err[FRAME_ERR_RANGE] >= 0 || R.err[FRAME_ERR_ABSENT] >= 0)
    return fail(c, MPMHIP_EINVAL, "internal: download_dev: the particles changed between the ranking and the rows (id %d)",
                std::max(R.err[FRAME_ERR_RANGE], R.err[FRAME_ERR_ABSENT]));
  return (int64_t)n;
}

int mpmhip_upload_dev(mpmhip_ctx *c, const void *const src[8], int64_t n, int32_t order) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  FieldTable T;
  int rc = fd_ready(c, src, order, "upload_dev", T);
  if (rc) return rc;
  if (T.p[MPMHIP_F_GID]) return fail(c, MPMHIP_EINVAL, "field %d cannot be uploaded", (int)MPMHIP_F_GID);
  if ((rc = ensure_b_current(c))) return rc;
  DevBuf<uint32_t> offs, small;
  FrameRank R;
  uint32_t live;
  if (order == 0) {
    if ((rc = fd_count(c, offs, live))) return rc;
  } else {
    if ((rc = fd_rank(c, R, "upload_dev"))) return rc;
    live = R.n_words ? R.set : 0u;
  }
  if (n != (int64_t)live) return fail(c, MPMHIP_EINVAL, "upload of %lld records but the ctx holds %u particles", (long long)n, live);
  if (live) {
    HIPCHK(c, small.alloc(FIELDS_WORDS));
    HIPCHK(c, hipMemsetAsync(small.get() + FIELDS_W_TOP, 0, 4, c->stream));
    HIPCHK(c, hipMemsetAsync(small.get() + FIELDS_W_ERR, 0xFF, 4, c->stream));
    fields_launch_put(c->stream, order == 1, (uint32_t)c->n_slots, c->rg.get(), c->rp.get(), c->rb.get(), offs.get(), R.top, (const uint32_t *)R.bits,
                      (const uint32_t *)R.prefix, live, T, small.get());
    if ((rc = launch_check(c, "k_fields_put"))) return rc;
    uint32_t h[FIELDS_WORDS];
    HIPCHK(c, hipMemcpyAsync(h, small.get(), sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((int32_t)h[FIELDS_W_ERR] >= 0)
      return fail(c, MPMHIP_EINVAL, "internal: upload_dev: the particles changed between the count and the rows (row %d of %u)", (int32_t)h[FIELDS_W_ERR], live);
    // the id counter: raised to 1 + the largest uploaded id, never lowered
    if (T.p[MPMHIP_F_ID] && (int64_t)h[FIELDS_W_TOP] > (int64_t)c->next_pid) c->next_pid = (int32_t)std::min<uint32_t>(h[FIELDS_W_TOP], 0x7FFFFFFFu);
  }
  // the transitions of mpmhip_upload, over all the fields of the call
  if (T.p[MPMHIP_F_X] || T.p[MPMHIP_F_V])
    if ((rc = invalidate_keys(c))) return rc;
  if (T.p[MPMHIP_F_B] || T.p[MPMHIP_F_F] || T.p[MPMHIP_F_AUX]) c->rec.affine_inputs_changed();
  if (T.p[MPMHIP_F_ID]) c->rec.ids_changed(c->deterministic);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MPMHIP_OK;
}

int mpmhip_download_grid_dev(mpmhip_ctx *c, int32_t which, float *dst_dev) {
  if (!c || !dst_dev || (which != 0 && which != 1)) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  size_t nodes;
  int rc = ensure_dense(c, nodes);
  if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(c->dense, 0, nodes * sizeof(float4), c->stream));
  if ((rc = do_grid(c, which == 0 ? 1 : 3))) return rc;
  HIPCHK(c, hipMemcpyAsync(dst_dev, c->dense, nodes * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MPMHIP_OK;
}
