// taichi_mpm_amd/csrc/region_api.h — host side of the region expressions (kernels: k_region.h; checks: region_program.h; rules:
// include/mpmhip.h).  Included by mpmhip.hip inside its extern "C" block, behind seed_api.h.  The seeding entries go through the one
// driver of seed_api.h with RegionExpr<D> as the region; the two ctx-free entries keep their arrays for the length of the call.
// mpmhip_seed_particles_brick and mpmhip_seed_histogram take either kind of region (NULL: the plain one of the seed description) and
// stand here for that reason; mpmhip_set_next_id beside them.
#pragma once

extern "C++" {
namespace {

// the description as the kernels take it; `why` says what a refused description lacks.  The phi arrays go back to back into `buf`
// (grown when `cap` floats do not hold them) on `stream`.
template <int D>
int region_build(const mpmhip_region_desc *r, DevBuf<float> &buf, size_t &cap, hipStream_t stream, RegionExpr<D> &R, std::string &why) {
  size_t counts[MPMHIP_REGION_MAX_FIELDS] = {};
  if (!region_program::check<D>(r, why, counts)) return MPMHIP_EINVAL;
  size_t total = 0;
  for (int f = 0; f < r->n_fields; f++) total += counts[f];
  if (total && (total > cap || !buf)) {
    cap = 0;
    if (buf.alloc(total) != hipSuccess) { why = "device allocation of " + std::to_string(total * sizeof(float)) + " bytes failed"; return MPMHIP_ENOMEM; }
    cap = total;
  }
  memset(&R, 0, sizeof R);
  size_t at = 0;
  for (int f = 0; f < r->n_fields; f++) {
    const hipError_t e = hipMemcpyAsync(buf + at, r->fields[f].phi, sizeof(float) * counts[f], hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) { why = std::string("upload of a phi array failed: ") + hipGetErrorString(e); return MPMHIP_EHIP; }
    sdf_fill<D>(R.field[f], r->fields[f], buf + at, nullptr, 0.0f, 1.0f);  // one frame
    at += counts[f];
  }
  R.n_ops = r->n_ops;
  for (int i = 0; i < r->n_ops; i++) R.ops[i] = r->ops[i].op | (r->ops[i].op == MPMHIP_REGION_PUSH ? r->ops[i].leaf << 2 : 0);
  for (int i = 0; i < r->n_leaves; i++) {
    const mpmhip_region_leaf &L = r->leaves[i];
    RegionLeafDev &o = R.leaf[i];
    o.kind = L.kind; o.field = L.kind ? L.field : 0;
    o.placed = L.placed != 0; o.banded = L.banded != 0;
    if (!L.kind) {
      o.shape.type = L.shape.type; o.shape.inside_out = L.shape.inside_out;
      for (int k = 0; k < 6; k++) o.shape.p[k] = L.shape.p[k];
      if (D == 2) {  // read in the plane, as mpmhip2d_set_levelset does
        if (o.shape.type == 2) { o.shape.p[2] = -1e30f; o.shape.p[5] = 1e30f; }  // a box in the plane: unbounded along z
        else o.shape.p[2] = 0.0f;
      }
    }
    o.scale = o.inv_scale = 1.0f;
    if (o.placed) {
      if (D == 3) {
        for (int k = 0; k < 9; k++) o.rot[k] = L.rot[k];
      } else {
        const float cs = (float)std::cos((double)L.rot[0]), sn = (float)std::sin((double)L.rot[0]);
        o.rot[0] = cs; o.rot[1] = -sn; o.rot[3] = sn; o.rot[4] = cs;
      }
      o.scale = L.scale; o.inv_scale = 1.0f / L.scale;
      for (int k = 0; k < D; k++) { o.t[k] = L.translate[k]; o.p[k] = L.pivot[k]; }
    }
    if (o.banded) { o.lo = L.lo; o.hi = L.hi; }
  }
  return MPMHIP_OK;
}

// `region` == NULL: the plain region of `how` (seed_region); else the expression, and `how` must carry no region of its own
template <class A, SeedCall CALL>
int seed_particles_either(typename A::Ctx *c, int32_t group, const typename A::Desc *how, const mpmhip_region_desc *region, SeedOut &out) {
  if (!region)
    return seed_particles_as<A, typename A::Region, CALL>(c, group, how, out, [&](typename A::Region &R) { return seed_region<A>(c, how, R); });
  if (c && how && (how->n_shapes != 0 || how->sdf))
    return A::fail(c, MPMHIP_EINVAL, "seed_particles_region: the seed description's own region must be empty (n_shapes == 0, sdf == NULL)");
  return seed_particles_as<A, RegionExpr<A::D>, CALL>(c, group, how, out, [&](RegionExpr<A::D> &R) {
    std::string why;
    SeedWork &W = c->seed;
    const int rc = region_build<A::D>(region, W.d_phi, W.phi_cap, c->stream, R, why);
    return rc ? A::fail(c, rc, ("seed_particles_region: " + why).c_str()) : (int)MPMHIP_OK;
  });
}

template <class A>
int seed_particles_region(typename A::Ctx *c, int32_t group, const typename A::Desc *how, const mpmhip_region_desc *region, int64_t *n_added) {
  if (n_added) *n_added = 0;
  if (c && !region) return A::fail(c, MPMHIP_EINVAL, "seed_particles_region: the region description is required");
  SeedOut out;
  const int rc = seed_particles_either<A, SEED_WHOLE>(c, group, how, region, out);
  if (n_added) *n_added = out.here;
  return rc;
}

// what the two ctx-free entries share: the arguments, the device, the description checked (region_build) and on the device
template <int D>
int region_free_setup(const char *who, int32_t device, float delta_x, const mpmhip_region_desc *region, DevBuf<float> &buf, RegionExpr<D> &R) {
  if (!(delta_x > 0.0f) || !std::isfinite(delta_x)) return fail(nullptr, MPMHIP_EINVAL, "%s: delta_x must be a finite number > 0", who);
  std::string why;
  if (!region) return fail(nullptr, MPMHIP_EINVAL, "%s: the region description is required", who);
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
    return fail(nullptr, MPMHIP_EINVAL, "%s: device %d is not one of the %d visible GPUs", who, device, n_dev);
  HIPCHK(nullptr, hipSetDevice(device));
  size_t cap = 0;
  if (int rc = region_build<D>(region, buf, cap, nullptr, R, why)) return fail(nullptr, rc, "%s: %s", who, why.c_str());
  return MPMHIP_OK;
}

template <int D>
int region_sample(int32_t device, float delta_x, const mpmhip_region_desc *region, int64_t n, const float *pos, float *phi_out) {
  if (n < 0 || n > 0x7fffffffll || ((!pos || !phi_out) && n)) return fail(nullptr, MPMHIP_EINVAL, "region_sample: n in [0, 2^31) and both arrays are required");
  DevBuf<float> d_phi, d_pos, d_out;
  RegionExpr<D> R;
  if (int rc = region_free_setup<D>("region_sample", device, delta_x, region, d_phi, R)) return rc;
  if (n == 0) return MPMHIP_OK;
  if (d_pos.alloc((size_t)n * D) != hipSuccess || d_out.alloc((size_t)n) != hipSuccess)
    return fail(nullptr, MPMHIP_ENOMEM, "region_sample: device allocation for %lld points failed", (long long)n);
  HIPCHK(nullptr, hipMemcpyAsync(d_pos, pos, sizeof(float) * D * (size_t)n, hipMemcpyHostToDevice, nullptr));
  hipLaunchKernelGGL(k_region_sample<D>, dim3((uint32_t)((n + REGION_WG - 1) / REGION_WG)), dim3(REGION_WG), 0, nullptr, R, 1.0f / delta_x,
                     (uint32_t)n, (const float *)d_pos, d_out.get());
  if (int rc = launch_check(nullptr, "region_sample")) return rc;
  HIPCHK(nullptr, hipMemcpy(phi_out, d_out, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
  return MPMHIP_OK;
}

template <int D>
int region_bake(int32_t device, float delta_x, const mpmhip_region_desc *region, const mpmhip_sdf_desc *lattice, float band, float *phi_out) {
  if (!lattice || !phi_out) return fail(nullptr, MPMHIP_EINVAL, "region_bake: the lattice and the output array are required");
  std::string why;
  const size_t count = sdf_lattice::check<D>(lattice->res, lattice->origin, lattice->spacing, why);
  if (!count) return fail(nullptr, MPMHIP_EINVAL, "region_bake: %s", why.c_str());
  if (!(band > 0.0f) || !std::isfinite(band)) return fail(nullptr, MPMHIP_EINVAL, "region_bake: band must be a finite number > 0");
  DevBuf<float> d_phi, d_out;
  RegionExpr<D> R;
  if (int rc = region_free_setup<D>("region_bake", device, delta_x, region, d_phi, R)) return rc;
  if (d_out.alloc(count) != hipSuccess) return fail(nullptr, MPMHIP_ENOMEM, "region_bake: device allocation of %zu bytes failed", count * sizeof(float));
  RegionLattice<D> L;
  for (int k = 0; k < D; k++) { L.res[k] = lattice->res[k]; L.origin[k] = lattice->origin[k]; }
  L.spacing = lattice->spacing;
  hipLaunchKernelGGL(k_region_bake<D>, dim3((uint32_t)((count + REGION_WG - 1) / REGION_WG)), dim3(REGION_WG), 0, nullptr, R, L, delta_x,
                     1.0f / delta_x, band, (uint32_t)count, d_out.get());
  if (int rc = launch_check(nullptr, "region_bake")) return rc;
  HIPCHK(nullptr, hipMemcpy(phi_out, d_out, sizeof(float) * count, hipMemcpyDeviceToHost));
  return MPMHIP_OK;
}

}  // namespace
}  // extern "C++"

int mpmhip_seed_particles_region(mpmhip_ctx *c, int32_t group, const mpmhip_seed_desc *how, const mpmhip_region_desc *region, int64_t *n_added) {
  return seed_particles_region<Seed3>(c, group, how, region, n_added);
}
int mpmhip2d_seed_particles_region(mpmhip2d_ctx *m, int32_t group, const mpmhip2d_seed_desc *how, const mpmhip_region_desc *region,
                                   int64_t *n_added) {
  return seed_particles_region<Seed2>(m, group, how, region, n_added);
}
int mpmhip_seed_particles_brick(mpmhip_ctx *c, int32_t group, const mpmhip_seed_desc *how, const mpmhip_region_desc *region, int64_t counts[2]) {
  SeedOut out;
  const int rc = seed_particles_either<Seed3, SEED_BRICK>(c, group, how, region, out);
  if (counts) { counts[0] = out.here; counts[1] = out.job; }
  return rc;
}
int mpmhip_seed_histogram(mpmhip_ctx *c, const mpmhip_seed_desc *how, const mpmhip_region_desc *region, int64_t *hist_x, int64_t *hist_y,
                          int64_t *hist_z, int64_t *total, int32_t cell_bounds[6]) {
  SeedOut out;
  out.hist[0] = hist_x; out.hist[1] = hist_y; out.hist[2] = hist_z;
  out.total = total; out.cell_bounds = cell_bounds;
  if (total) *total = 0;
  return seed_particles_either<Seed3, SEED_HIST>(c, -1, how, region, out);
}
int mpmhip_set_next_id(mpmhip_ctx *c, int32_t id) {
  if (!c) return MPMHIP_EINVAL;
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "set_next_id inside a substep");
  if (id > c->next_pid) c->next_pid = id;
  return c->next_pid;
}
int mpmhip_region_sample(int32_t device, int32_t dim, float delta_x, const mpmhip_region_desc *region, int64_t n, const float *pos, float *phi_out) {
  if (dim == 3) return region_sample<3>(device, delta_x, region, n, pos, phi_out);
  if (dim == 2) return region_sample<2>(device, delta_x, region, n, pos, phi_out);
  return fail(nullptr, MPMHIP_EINVAL, "region_sample: dim must be 2 or 3");
}
int mpmhip_region_bake(int32_t device, int32_t dim, float delta_x, const mpmhip_region_desc *region, const mpmhip_sdf_desc *lattice, float band,
                       float *phi_out) {
  if (dim == 3) return region_bake<3>(device, delta_x, region, lattice, band, phi_out);
  if (dim == 2) return region_bake<2>(device, delta_x, region, lattice, band, phi_out);
  return fail(nullptr, MPMHIP_EINVAL, "region_bake: dim must be 2 or 3");
}
