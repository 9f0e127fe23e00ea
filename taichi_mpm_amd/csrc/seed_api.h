// taichi_mpm_amd/csrc/seed_api.h — host side of mpmhip_seed_particles (kernels: k_seed.h; tile: poisson_tile.h; rules: include/mpmhip.h)
// Included by mpmhip.hip inside its extern "C" block.  A call synchronises twice for a few words each: the get-ready box (the number
// of replicas sizes the candidate passes) and the survivors' count (the capacity check comes before anything is written).
#pragma once

int64_t mpmhip_poisson_tile(float *out, int64_t capacity) {
  const std::vector<float> &t = poisson_tile::tile();
  const int64_t n = (int64_t)(t.size() / 3);
  if (out && capacity > 0) memcpy(out, t.data(), sizeof(float) * 3 * (size_t)std::min(n, capacity));
  return n;
}

extern "C++" {
namespace {

#define SEED_NO_CONTRACT _Pragma("clang fp contract(off)")

// the region of a seeding call as the kernels take it; a sampled field is uploaded into the ctx's buffer
int seed_region(mpmhip_ctx *c, const mpmhip_seed_desc *d, SeedRegion &R) {
  memset(&R, 0, sizeof R);
  if (!d->sdf) {
    if (int rc = check_shapes(c, d->n_shapes, d->shapes)) return rc;
    R.n_shapes = d->n_shapes;
    for (int i = 0; i < d->n_shapes; i++) {
      R.s[i].type = d->shapes[i].type;
      R.s[i].inside_out = d->shapes[i].inside_out;
      for (int k = 0; k < 6; k++) R.s[i].p[k] = d->shapes[i].p[k];
    }
    return MPMHIP_OK;
  }
  const mpmhip_sdf_desc *L = d->sdf;
  if (!d->phi) return fail(c, MPMHIP_EINVAL, "seed_particles: a sampled region needs its phi array");
  size_t count = 1;
  for (int k = 0; k < 3; k++) {  // what mpmhip_set_levelset_sdf refuses
    if (L->res[k] < 2) return fail(c, MPMHIP_EINVAL, "seed_particles: res[%d] = %d, at least 2 samples per axis are needed", k, L->res[k]);
    if (!std::isfinite(L->origin[k])) return fail(c, MPMHIP_EINVAL, "seed_particles: origin[%d] is not finite", k);
    count *= (size_t)L->res[k];
  }
  if (!(L->spacing > 0.0f) || !std::isfinite(L->spacing)) return fail(c, MPMHIP_EINVAL, "seed_particles: spacing must be a finite number > 0");
  if (count > ((size_t)1 << 31)) return fail(c, MPMHIP_EINVAL, "seed_particles: more than 2^31 samples");
  SeedWork &W = c->seed;
  if (count > W.phi_cap || !W.d_phi) {
    W.phi_cap = 0;
    if (W.d_phi.alloc(count) != hipSuccess) return fail(c, MPMHIP_ENOMEM, "seed_particles: device allocation of %zu bytes failed", count * sizeof(float));
    W.phi_cap = count;
  }
  HIPCHK(c, hipMemcpyAsync(W.d_phi, d->phi, sizeof(float) * count, hipMemcpyHostToDevice, c->stream));
  R.sdf.phi0 = W.d_phi;
  R.sdf.phi1 = nullptr;
  R.sdf.spacing = L->spacing; R.sdf.inv_spacing = 1.0f / L->spacing;
  R.sdf.t0 = 0.0f; R.sdf.t1 = 1.0f;
  for (int k = 0; k < 3; k++) { R.sdf.res[k] = L->res[k]; R.sdf.origin[k] = L->origin[k]; }
  return MPMHIP_OK;
}

// get_ready + the replicas (src/poisson_disk_sampler.h:34-69, :166-173) from the box of inside cell centres, in fp32
void seed_get_ready(const mpmhip_ctx *c, const mpmhip_seed_desc *d, const int box[6], SeedParams &S) {
  SEED_NO_CONTRACT
  const float dx = c->P.dx;
  const double v = (double)dx * (double)dx * (double)dx / (double)d->ppc;
  S.min_distance = (float)std::cbrt(v * 13.0 / 18.0);
  S.region_size = 40.0f * S.min_distance;
  S.n_rep = 1;
  for (int k = 0; k < 3; k++) {
    const float lo = ((float)box[k] + 0.5f) * dx, hi = ((float)box[3 + k] + 0.5f) * dx;
    const float min_corner = lo - dx, max_corner = hi + dx;
    const float size = max_corner - min_corner;
    S.min_corner[k] = min_corner;
    S.nrep[k] = std::max(1, (int)std::ceil(size / S.region_size));
  }
}

}  // namespace
}  // extern "C++"

int mpmhip_seed_particles(mpmhip_ctx *c, int32_t group, const mpmhip_seed_desc *d, int64_t *n_added) {
  SEED_NO_CONTRACT
  if (!c) return MPMHIP_EINVAL;
  if (n_added) *n_added = 0;
  if (!d) return fail(c, MPMHIP_EINVAL, "seed_particles: the description is required");
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "seed_particles inside a substep");
  if (c->T.enabled || c->tn.on) return fail(c, MPMHIP_EINVAL, "seed_particles on a tiled ctx: seed before the partition is set, or give each rank its positions");
  if (group < 0 || group >= (int)c->groups.size()) return fail(c, MPMHIP_EINVAL, "unknown group %d", group);
  if (!(d->ppc > 0.0f) || !std::isfinite(d->ppc)) return fail(c, MPMHIP_EINVAL, "seed_particles: ppc must be a finite number > 0");
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(d->velocity[k])) return fail(c, MPMHIP_EINVAL, "seed_particles: velocity[%d] is not finite", k);
  if (!std::isfinite(d->initial_dg)) return fail(c, MPMHIP_EINVAL, "seed_particles: initial_dg is not finite");
  if (d->source && !std::isfinite(d->source_delta_t)) return fail(c, MPMHIP_EINVAL, "seed_particles: source_delta_t is not finite");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  SeedRegion R;
  if (int rc = seed_region(c, d, R)) return rc;
  SeedWork &W = c->seed;
  if (!W.d_tile) {
    const std::vector<float> &t = poisson_tile::tile();
    if (W.d_tile.alloc(t.size()) != hipSuccess) return fail(c, MPMHIP_ENOMEM, "seed_particles: device allocation of the tile failed");
    W.n_tile = (uint32_t)(t.size() / 3);
    HIPCHK(c, hipMemcpyAsync(W.d_tile, t.data(), sizeof(float) * t.size(), hipMemcpyHostToDevice, c->stream));
  }
  if (!W.d_box) HIPCHK(c, W.d_box.alloc(8));

  SeedParams S;
  memset(&S, 0, sizeof S);
  for (int k = 0; k < 3; k++) S.res[k] = c->P.res[k];
  S.dx = c->P.dx; S.idx = c->P.idx;
  // ---- get ready: the box of the cell centres inside the region
  int box[8] = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1, -1, -1, 0, 0};
  HIPCHK(c, hipMemcpyAsync(W.d_box, box, sizeof box, hipMemcpyHostToDevice, c->stream));
  const uint64_t cells = (uint64_t)S.res[0] * (uint64_t)S.res[1] * (uint64_t)S.res[2];
  const uint32_t bounds_wgs = (uint32_t)std::min<uint64_t>((cells + SEED_WG - 1) / SEED_WG, (uint64_t)c->n_cus * 32u);
  hipLaunchKernelGGL(k_seed_bounds, dim3(bounds_wgs), dim3(SEED_WG), 0, c->stream, R, S, W.d_box.get());
  if (int rc = launch_check(c, "seed_bounds")) return rc;
  HIPCHK(c, hipMemcpyAsync(box, W.d_box, sizeof box, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (box[3] < 0) return fail(c, MPMHIP_EINVAL, "seed_particles: region is empty (no cell centre of the grid lies inside it)");
  seed_get_ready(c, d, box, S);
  const uint64_t n_rep = (uint64_t)S.nrep[0] * (uint64_t)S.nrep[1] * (uint64_t)S.nrep[2];
  const uint64_t n_cand = n_rep * W.n_tile;
  if (n_cand > (1ull << 31))
    return fail(c, MPMHIP_EINVAL, "seed_particles: more than 2^31 candidates (%u tile points x %llu replicas): lower ppc or seed the region in parts",
                W.n_tile, (unsigned long long)n_rep);
  S.n_rep = (uint32_t)n_rep; S.n_tile = W.n_tile; S.n_cand = (uint32_t)n_cand;
  S.source = d->source != 0;
  const GroupParams &G = c->groups[group];
  const int mat = G.type;
  for (int k = 0; k < 3; k++) {
    S.velocity[k] = d->velocity[k];
    if (S.source) {  // src/mpm.cpp:222-227
      const float dt = d->source_delta_t;
      S.offset[k] = d->velocity[k] * c->t;
      const float a = d->velocity[k] * dt, b = 0.5f * c->P.g[k];
      const float e = b * (dt + c->P.dt);
      S.advection[k] = a + e * dt;
    }
  }
  S.dg = d->initial_dg;
  S.aux = (mat == MPMHIP_SNOW || mat == MPMHIP_WATER) ? 1.0f : (mat == MPMHIP_VISCO ? 1000.0f : 0.0f);  // as mpmhip_add_particles
  S.mass = G.p[0];
  S.gid = (uint32_t)group;
  S.pid0 = c->next_pid;
  // ---- count + scan
  const uint32_t wgs = (uint32_t)((n_cand + SEED_PER_WG - 1) / SEED_PER_WG);
  if (wgs > W.wg_cap || !W.d_words) {
    W.wg_cap = 0;
    if (W.d_words.alloc((size_t)wgs * SEED_WORDS) != hipSuccess || W.d_totals.alloc(wgs) != hipSuccess)
      return fail(c, MPMHIP_ENOMEM, "seed_particles: device allocation for %llu candidates failed", (unsigned long long)n_cand);
    W.wg_cap = wgs;
  }
  uint32_t *d_total = reinterpret_cast<uint32_t *>(W.d_box + 6);
  hipLaunchKernelGGL(k_seed_count, dim3(wgs), dim3(SEED_WG), 0, c->stream, R, S, (const float *)W.d_tile, W.d_words.get(), W.d_totals.get());
  hipLaunchKernelGGL(k_seed_scan, dim3(1), dim3(SEED_SCAN_WG), 0, c->stream, W.d_totals.get(), wgs, d_total);
  if (int rc = launch_check(c, "seed_count")) return rc;
  uint32_t total = 0;
  HIPCHK(c, hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int64_t n = (int64_t)total;
  if (n_added) *n_added = n;
  if (n == 0) return MPMHIP_OK;
  if (int rc = async_drop_view(c)) return rc;  // (resident async stepper: records that only mirror the pools go first)
  if (c->n_slots + n > c->cap)
    return fail(c, MPMHIP_ECAPACITY, "particle capacity exceeded: %lld + %lld > %lld", (long long)c->n_slots, (long long)n, (long long)c->cap);
  if ((int64_t)c->next_pid + n > 0x7fffffffll) return fail(c, MPMHIP_ECAPACITY, "seed_particles: creation ids exceed 2^31");
  if (int rc = ensure_b_current(c)) return rc;  // A of every particle is recomputed from apic_b
  // ---- write the records
  hipLaunchKernelGGL(k_seed_write, dim3(wgs), dim3(SEED_WG), 0, c->stream, S, (const float *)W.d_tile, (const unsigned long long *)W.d_words,
                     (const uint32_t *)W.d_totals, reinterpret_cast<float4 *>(c->rg + c->n_slots), reinterpret_cast<float4 *>(c->rp + c->n_slots),
                     reinterpret_cast<float4 *>(c->rb + (size_t)c->n_slots * BW));
  if (int rc = launch_check(c, "seed_write")) return rc;
  c->next_pid += (int32_t)n;
  set_slots(c, c->n_slots + n);
  return clear_block_flags(c, c->rec.particles_appended());
}
#undef SEED_NO_CONTRACT
