// taichi_mpm_amd/csrc/seed2d_api.h — host side of mpmhip2d_seed_particles and mpmhip2d_reserve (kernels: k_seed2d.h; tile:
// poisson_tile2d.h; rules: include/mpmhip.h).  Included by mpmhip.hip inside its extern "C" block, behind async2d_api.h.  A seeding
// call synchronises twice for a few words each: the get-ready box (the number of replicas sizes the candidate passes) and the
// survivors' count (the capacity check comes before anything is written).
#pragma once

int64_t mpmhip2d_poisson_tile(float *out, int64_t capacity) {
  const std::vector<float> &t = poisson_tile2d::tile();
  const int64_t n = (int64_t)(t.size() / 2);
  if (out && capacity > 0) memcpy(out, t.data(), sizeof(float) * 2 * (size_t)std::min(n, capacity));
  return n;
}

// the particle arrays hold at least `capacity` particles; what they hold stays.  The per-particle arrays of the CPIC coupling grow
// with them (a2_grow_particles_any); those of the deterministic mode are scratch of one substep, sized by a capacity of their own
// that det2_reserve compares with the ctx's at every substep: they follow at the next one.
int mpmhip2d_reserve(mpmhip2d_ctx *m, int64_t capacity) {
  if (!m) return MPMHIP_EINVAL;
  if (capacity <= m->cap) return MPMHIP_OK;
  HIPCHK2D(m, hipSetDevice(m->device));
  return a2_grow_particles_any(m, capacity);
}

int64_t mpmhip2d_num_slots(mpmhip2d_ctx *m) { return m ? m->n : (int64_t)MPMHIP_EINVAL; }

#define SEED2_NO_CONTRACT _Pragma("clang fp contract(off)")

// the region of a seeding call as the kernels take it; a sampled field is uploaded into the ctx's buffer
static int seed2_region(mpmhip2d_ctx *m, const mpmhip2d_seed_desc *d, mpm2d::SeedRegion2 &R) {
  memset(&R, 0, sizeof R);
  if (!d->sdf) {
    if (d->n_shapes < 0 || d->n_shapes > MPMHIP_MAX_SHAPES) return fail2d(m, MPMHIP_EINVAL, "seed_particles: n_shapes outside [0, " + std::to_string(MPMHIP_MAX_SHAPES) + "]");
    R.n_shapes = d->n_shapes;
    for (int i = 0; i < d->n_shapes; i++) {  // read in the plane, as mpmhip2d_set_levelset does
      const mpmhip_shape &s = d->shapes[i];
      if (s.type < 0 || s.type > 2) return fail2d(m, MPMHIP_EINVAL, "seed_particles: unknown shape type " + std::to_string(s.type));
      R.s[i].type = s.type;
      R.s[i].inside_out = s.inside_out;
      for (int k = 0; k < 6; k++) R.s[i].p[k] = s.p[k];
      if (s.type == 2) { R.s[i].p[2] = -1e30f; R.s[i].p[5] = 1e30f; }  // a box in the plane: unbounded along z
      else R.s[i].p[2] = 0.0f;
    }
    return MPMHIP_OK;
  }
  const mpmhip2d_sdf_desc *L = d->sdf;
  if (!d->phi) return fail2d(m, MPMHIP_EINVAL, "seed_particles: a sampled region needs its phi array");
  size_t count = 1;
  for (int k = 0; k < 2; k++) {
    if (L->res[k] < 2)
      return fail2d(m, MPMHIP_EINVAL, "seed_particles: res[" + std::to_string(k) + "] = " + std::to_string(L->res[k]) + ", at least 2 samples per axis are needed");
    if (!std::isfinite(L->origin[k])) return fail2d(m, MPMHIP_EINVAL, "seed_particles: origin[" + std::to_string(k) + "] is not finite");
    count *= (size_t)L->res[k];
  }
  if (!(L->spacing > 0.0f) || !std::isfinite(L->spacing)) return fail2d(m, MPMHIP_EINVAL, "seed_particles: spacing must be a finite number > 0");
  if (count > ((size_t)1 << 31)) return fail2d(m, MPMHIP_EINVAL, "seed_particles: more than 2^31 samples");
  mpm2d::SeedWork2 &W = m->seed;
  if (count > W.phi_cap || !W.d_phi) {
    W.phi_cap = 0;
    if (W.d_phi.alloc(count) != hipSuccess)
      return fail2d(m, MPMHIP_ENOMEM, "seed_particles: device allocation of " + std::to_string(count * sizeof(float)) + " bytes failed");
    W.phi_cap = count;
  }
  HIPCHK2D(m, hipMemcpyAsync(W.d_phi, d->phi, sizeof(float) * count, hipMemcpyHostToDevice, m->stream));
  R.sdf.phi = W.d_phi;
  R.sdf.spacing = L->spacing; R.sdf.inv_spacing = 1.0f / L->spacing;
  for (int k = 0; k < 2; k++) { R.sdf.res[k] = L->res[k]; R.sdf.origin[k] = L->origin[k]; }
  return MPMHIP_OK;
}

// get_ready + the replicas (src/poisson_disk_sampler.h:34-69, :166-173) from the box of inside cell centres, in fp32; the replicas
// per axis as floats (a tiny spacing gives more than an int holds: the caller refuses them)
static void seed2_get_ready(const mpmhip2d_ctx *m, const mpmhip2d_seed_desc *d, const int box[4], mpm2d::SeedParams2 &S, float nrep[2]) {
  SEED2_NO_CONTRACT
  const float dx = m->P.dx;
  const double v = (double)dx * (double)dx / (double)d->ppc;
  S.min_distance = (float)std::sqrt(v * 2.0 / 3.0);
  S.region_size = 40.0f * S.min_distance;
  for (int k = 0; k < 2; k++) {
    const float lo = ((float)box[k] + 0.5f) * dx, hi = ((float)box[2 + k] + 0.5f) * dx;
    const float min_corner = lo - dx, max_corner = hi + dx;
    const float size = max_corner - min_corner;
    S.min_corner[k] = min_corner;
    nrep[k] = std::max(1.0f, std::ceil(size / S.region_size));
  }
}

int mpmhip2d_seed_particles(mpmhip2d_ctx *m, int32_t group, const mpmhip2d_seed_desc *d, int64_t *n_added) {
  SEED2_NO_CONTRACT
  using namespace mpm2d;
  if (!m) return MPMHIP_EINVAL;
  if (n_added) *n_added = 0;
  if (!d) return fail2d(m, MPMHIP_EINVAL, "seed_particles: the description is required");
  if (m->async.resident)
    return fail2d(m, MPMHIP_EINVAL, "seed_particles: not on a resident asynchronous stepper (seed before mpmhip2d_async_begin)");
  if (group < 0 || group >= (int)m->groups.size()) return fail2d(m, MPMHIP_EINVAL, "unknown group " + std::to_string(group));
  if (!(d->ppc > 0.0f) || !std::isfinite(d->ppc)) return fail2d(m, MPMHIP_EINVAL, "seed_particles: ppc must be a finite number > 0");
  for (int k = 0; k < 2; k++)
    if (!std::isfinite(d->velocity[k])) return fail2d(m, MPMHIP_EINVAL, "seed_particles: velocity[" + std::to_string(k) + "] is not finite");
  if (!std::isfinite(d->initial_dg)) return fail2d(m, MPMHIP_EINVAL, "seed_particles: initial_dg is not finite");
  if (d->source && !std::isfinite(d->source_delta_t)) return fail2d(m, MPMHIP_EINVAL, "seed_particles: source_delta_t is not finite");
  HIPCHK2D(m, hipSetDevice(m->device));
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  SeedRegion2 R;
  if (int rc = seed2_region(m, d, R)) return rc;
  SeedWork2 &W = m->seed;
  if (!W.d_tile) {
    const std::vector<float> &t = poisson_tile2d::tile();
    if (W.d_tile.alloc(t.size()) != hipSuccess) return fail2d(m, MPMHIP_ENOMEM, "seed_particles: device allocation of the tile failed");
    W.n_tile = (uint32_t)(t.size() / 2);
    HIPCHK2D(m, hipMemcpyAsync(W.d_tile, t.data(), sizeof(float) * t.size(), hipMemcpyHostToDevice, m->stream));
  }
  if (!W.d_box) HIPCHK2D(m, W.d_box.alloc(8));

  SeedParams2 S;
  memset(&S, 0, sizeof S);
  S.res[0] = m->P.res[0]; S.res[1] = m->P.res[1];
  S.dx = m->P.dx; S.idx = m->P.idx;
  // ---- get ready: the box of the cell centres inside the region
  int box[8] = {0x7fffffff, 0x7fffffff, -1, -1, 0, 0, 0, 0};
  HIPCHK2D(m, hipMemcpyAsync(W.d_box, box, sizeof box, hipMemcpyHostToDevice, m->stream));
  const uint32_t cells = (uint32_t)S.res[0] * (uint32_t)S.res[1];
  const uint32_t bounds_wgs = std::min<uint32_t>((cells + SEED_WG - 1) / SEED_WG, 8192u);
  hipLaunchKernelGGL(k2_seed_bounds, dim3(bounds_wgs), dim3(SEED_WG), 0, m->stream, R, S, W.d_box.get());
  HIPCHK2D(m, hipGetLastError());
  HIPCHK2D(m, hipMemcpyAsync(box, W.d_box, sizeof box, hipMemcpyDeviceToHost, m->stream));
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  if (box[2] < 0) return fail2d(m, MPMHIP_EINVAL, "seed_particles: region is empty (no cell centre of the grid lies inside it)");
  float nrep[2];
  seed2_get_ready(m, d, box, S, nrep);
  const double n_rep = (double)nrep[0] * (double)nrep[1];  // (exact: two integers below 2^24 each, or far beyond the limit)
  const double n_cand = n_rep * (double)W.n_tile;
  if (!(n_cand <= 2147483648.0)) {
    char msg[200];
    snprintf(msg, sizeof msg, "seed_particles: more than 2^31 candidates (%u tile points x %.0f replicas): lower ppc or seed the region in parts",
             W.n_tile, n_rep);
    return fail2d(m, MPMHIP_EINVAL, msg);
  }
  S.nrep1 = (uint32_t)nrep[1];
  S.n_rep = (uint32_t)n_rep; S.n_tile = W.n_tile; S.n_cand = (uint32_t)n_cand;
  S.source = d->source != 0;
  const GroupParams &G = m->groups[group];
  const int mat = G.type;
  for (int k = 0; k < 2; k++) {
    S.velocity[k] = d->velocity[k];
    if (S.source) {  // src/mpm.cpp:222-227
      const float dt = d->source_delta_t;
      S.offset[k] = d->velocity[k] * m->t;
      const float a = d->velocity[k] * dt, b = 0.5f * m->P.g[k];
      const float e = b * (dt + m->base_dt);
      S.advection[k] = a + e * dt;
    }
  }
  S.dg = d->initial_dg;
  S.aux = (mat == MPMHIP_SNOW || mat == MPMHIP_WATER) ? 1.0f : (mat == MPMHIP_VISCO ? 1000.0f : 0.0f);  // as mpmhip2d_add_particles
  S.gid = group;
  S.pid0 = m->next_pid;
  // ---- count + scan
  const uint32_t wgs = (uint32_t)(((uint64_t)S.n_cand + SEED_PER_WG - 1) / SEED_PER_WG);
  if (wgs > W.wg_cap || !W.d_words) {
    W.wg_cap = 0;
    if (W.d_words.alloc((size_t)wgs * SEED_WORDS) != hipSuccess || W.d_totals.alloc(wgs) != hipSuccess)
      return fail2d(m, MPMHIP_ENOMEM, "seed_particles: device allocation for " + std::to_string(S.n_cand) + " candidates failed");
    W.wg_cap = wgs;
  }
  uint32_t *d_total = reinterpret_cast<uint32_t *>(W.d_box + 4);
  hipLaunchKernelGGL(k2_seed_count, dim3(wgs), dim3(SEED_WG), 0, m->stream, R, S, (const float *)W.d_tile, W.d_words.get(), W.d_totals.get());
  hipLaunchKernelGGL(mpm::k_seed_scan, dim3(1), dim3(mpm::SEED_SCAN_WG), 0, m->stream, W.d_totals.get(), wgs, d_total);
  HIPCHK2D(m, hipGetLastError());
  uint32_t total = 0;
  HIPCHK2D(m, hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, m->stream));
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  const int64_t n = (int64_t)total;
  if (n_added) *n_added = n;
  if (n == 0) return MPMHIP_OK;
  if ((int64_t)m->next_pid + n > 0x7fffffffll) return fail2d(m, MPMHIP_EINVAL, "seed_particles: creation ids exceed 2^31");
  if (m->n + n > m->cap)
    return fail2d(m, MPMHIP_ECAPACITY, "particle capacity exceeded: " + std::to_string(m->n) + " + " + std::to_string(n) + " > " + std::to_string(m->cap));
  // ---- write the rows behind the resident ones
  const size_t at = (size_t)m->n;
  hipLaunchKernelGGL(k2_seed_write, dim3(wgs), dim3(SEED_WG), 0, m->stream, S, (const float *)W.d_tile, (const unsigned long long *)W.d_words,
                     (const uint32_t *)W.d_totals, reinterpret_cast<float2 *>(m->x + 2 * at), reinterpret_cast<float2 *>(m->v + 2 * at),
                     reinterpret_cast<float4 *>(m->F + 4 * at), reinterpret_cast<float4 *>(m->B + 4 * at), m->aux + at, m->gid + at, m->pid + at);
  HIPCHK2D(m, hipGetLastError());
  m->next_pid += (int32_t)n;
  m->n += n;
  return MPMHIP_OK;
}
#undef SEED2_NO_CONTRACT
