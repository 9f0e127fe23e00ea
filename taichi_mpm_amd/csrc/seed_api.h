// taichi_mpm_amd/csrc/seed_api.h — host side of mpmhip_seed_particles, mpmhip2d_seed_particles and mpmhip2d_reserve (kernels: k_seed.h;
// tiles: poisson_tile.h; rules: include/mpmhip.h).  Included by mpmhip.hip inside its extern "C" block, behind async_api.h and
// frame2d_api.h: both ctx types are complete here.  One driver (seed_particles) carries the call for both dimensions; what a ctx does
// its own way is in its adapter (Seed3, Seed2).  A sampled region's lattice is judged by sdf_lattice.h and becomes the SdfDev of the
// boundary's sampler (mpmhip.hip: sdf_fill; mpm_math.h).  A call synchronises twice for a few words each: the get-ready box (the number of
// replicas sizes the candidate passes) and the survivors' count (the capacity check comes before anything is written).
// The same driver carries a rank of a tiled job filling its own brick and the histogram call (SeedCall; their entry points stand in
// region_api.h, where both kinds of region are known): what differs is the passes behind the get-ready box.
#pragma once

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
int64_t mpmhip2d_capacity(mpmhip2d_ctx *m) { return m ? m->cap : (int64_t)MPMHIP_EINVAL; }

extern "C++" {
namespace {

#define SEED_NO_CONTRACT _Pragma("clang fp contract(off)")

// which call the driver carries: the whole region on one ctx, this rank's brick of it (mpmhip_seed_particles_brick), or only the
// histograms of the survivors' base cells (mpmhip_seed_histogram: no group, nothing written)
enum SeedCall { SEED_WHOLE, SEED_BRICK, SEED_HIST };

template <int D>
int64_t seed_tile_out(float *out, int64_t capacity) {
  const std::vector<float> &t = poisson_tile::tile<D>();
  const int64_t n = (int64_t)(t.size() / D);
  if (out && capacity > 0) memcpy(out, t.data(), sizeof(float) * D * (size_t)std::min(n, capacity));
  return n;
}

template <class Region, class Desc>
void seed_copy_shapes(Region &R, const Desc *d) {
  R.n_shapes = d->n_shapes;
  for (int i = 0; i < d->n_shapes; i++) {
    R.s[i].type = d->shapes[i].type;
    R.s[i].inside_out = d->shapes[i].inside_out;
    for (int k = 0; k < 6; k++) R.s[i].p[k] = d->shapes[i].p[k];
  }
}

// What the driver asks of a ctx beyond the fields both have under one name (stream, device, P.dx, P.idx, P.res, P.g, t, groups,
// next_pid, seed): how an error is recorded, which calls are refused outright, how shapes become the region, the closed form of
// min_distance from v = dx^D / ppc, the cap on the bounds launch, the base time step, and the commit: its checks in this ctx's order
// with this ctx's codes, the sink, the bookkeeping behind the write.
struct Seed3 {
  static constexpr int D = 3;
  using Ctx = mpmhip_ctx;
  using Desc = mpmhip_seed_desc;
  using Region = SeedRegion;
  static int fail(Ctx *c, int code, const char *msg) { return ::fail(c, code, "%s", msg); }
  static const char *refused(const Ctx *c, SeedCall call) {
    if (c->in_substep) return "seed_particles inside a substep";
    const bool tiled = c->T.enabled || c->tn.on;
    if (call == SEED_WHOLE && tiled)
      return "seed_particles on a tiled ctx: mpmhip_seed_particles_brick fills every rank's own brick (or seed before the partition is set, or give "
             "each rank its positions)";
    if (call == SEED_BRICK && !tiled) return "seed_particles_brick needs a ctx with a partition (mpmhip_set_partition or mpmhip_tiled_setup)";
    return nullptr;
  }
  static int shapes(Ctx *c, const Desc *d, Region &R) {
    if (int rc = check_shapes(c, d->n_shapes, d->shapes)) return rc;
    seed_copy_shapes(R, d);
    return MPMHIP_OK;
  }
  static float min_distance(double v) { return (float)std::cbrt(v * 13.0 / 18.0); }
  static uint32_t max_bounds_wgs(const Ctx *c) { return (uint32_t)c->n_cus * 32u; }
  static float base_dt(const Ctx *c) { return c->P.dt; }
  // n particles are appended here and n_ids creation ids are used up (a rank of a tiled job: the job's count, n only its brick's)
  template <class Write>
  static int commit(Ctx *c, int32_t group, int64_t n, int64_t n_ids, Write write) {
    if (int rc = async_drop_view(c)) return rc;  // (resident async stepper: records that only mirror the pools go first)
    if (c->n_slots + n > c->cap)
      return ::fail(c, MPMHIP_ECAPACITY, "particle capacity exceeded: %lld + %lld > %lld", (long long)c->n_slots, (long long)n, (long long)c->cap);
    if ((int64_t)c->next_pid + n_ids > 0x7fffffffll) return ::fail(c, MPMHIP_ECAPACITY, "seed_particles: creation ids exceed 2^31");
    if (n == 0) { c->next_pid += (int32_t)n_ids; return MPMHIP_OK; }  // (every survivor lies in another rank's brick)
    if (int rc = ensure_b_current(c)) return rc;  // A of every particle is recomputed from apic_b
    if (int rc = write(SeedSink3{reinterpret_cast<float4 *>(c->rg + c->n_slots), reinterpret_cast<float4 *>(c->rp + c->n_slots),
                                 reinterpret_cast<float4 *>(c->rb + (size_t)c->n_slots * BW), c->groups[group].p[0]}))
      return rc;
    c->next_pid += (int32_t)n_ids;
    set_slots(c, c->n_slots + n);
    return clear_block_flags(c, c->rec.particles_appended());
  }
  // A ctx with a native plan (mpmhip_tiled_setup) between two advances: the halo boxes were cut to the particles of the last check and know
  // nothing of the new ones.  The plan goes stale — the next advance begins with the planning scan of a job's first substep, on every
  // rank, since every rank made this call — and until that scan has cut fresh boxes the clip box also holds every node a candidate of
  // this call can touch: the look-back test of tn_mig_c compares against the clip box while there are no occupancy boxes.  (The
  // candidates lie in [min_corner, min_corner + replicas * region_size) per axis; their base cells b reach the nodes b .. b + 2.)
  static void appended_to_job(Ctx *c, const SeedParams<3> &S) {
    if (!c->tn.on) return;  // (the callback path: the plan is the caller's, and so is planning again)
    auto &N = c->tn;
    for (int a = 0; a < 3; a++) {
      const double lo = (double)S.min_corner[a], hi = lo + (double)S.nrep[a] * (double)S.region_size;
      const int blo = (int)std::floor(lo * (double)S.idx - 0.5) - 1, bhi = (int)std::ceil(hi * (double)S.idx - 0.5) + 1;
      N.clip_lo[a] = std::max(0, std::min(N.clip_lo[a], blo));
      N.clip_hi[a] = std::min(c->P.res[a] + 1, std::max(N.clip_hi[a], bhi + 3));
    }
    N.occ_valid = false;
  }
};

struct Seed2 {
  static constexpr int D = 2;
  using Ctx = mpmhip2d_ctx;
  using Desc = mpmhip2d_seed_desc;
  using Region = SeedRegion2;
  static int fail(Ctx *m, int code, const char *msg) { return fail2d(m, code, msg); }
  static const char *refused(const Ctx *m, SeedCall) {
    return m->async.resident ? "seed_particles: not on a resident asynchronous stepper (seed before mpmhip2d_async_begin)" : nullptr;
  }
  static int shapes(Ctx *m, const Desc *d, Region &R) {
    if (d->n_shapes < 0 || d->n_shapes > MPMHIP_MAX_SHAPES) return fail2d(m, MPMHIP_EINVAL, "seed_particles: n_shapes outside [0, " + std::to_string(MPMHIP_MAX_SHAPES) + "]");
    for (int i = 0; i < d->n_shapes; i++)
      if (d->shapes[i].type < 0 || d->shapes[i].type > 2) return fail2d(m, MPMHIP_EINVAL, "seed_particles: unknown shape type " + std::to_string(d->shapes[i].type));
    seed_copy_shapes(R, d);
    for (int i = 0; i < R.n_shapes; i++) {  // read in the plane, as mpmhip2d_set_levelset does
      if (R.s[i].type == 2) { R.s[i].p[2] = -1e30f; R.s[i].p[5] = 1e30f; }  // a box in the plane: unbounded along z
      else R.s[i].p[2] = 0.0f;
    }
    return MPMHIP_OK;
  }
  static float min_distance(double v) { return (float)std::sqrt(v * 2.0 / 3.0); }
  static uint32_t max_bounds_wgs(const Ctx *) { return 8192u; }
  static float base_dt(const Ctx *m) { return m->base_dt; }
  template <class Write>
  static int commit(Ctx *m, int32_t, int64_t n, int64_t, Write write) {
    if ((int64_t)m->next_pid + n > 0x7fffffffll) return fail2d(m, MPMHIP_EINVAL, "seed_particles: creation ids exceed 2^31");
    if (m->n + n > m->cap)
      return fail2d(m, MPMHIP_ECAPACITY, "particle capacity exceeded: " + std::to_string(m->n) + " + " + std::to_string(n) + " > " + std::to_string(m->cap));
    const size_t at = (size_t)m->n;  // the rows behind the resident ones
    if (int rc = write(SeedSink2{reinterpret_cast<float2 *>(m->x + 2 * at), reinterpret_cast<float2 *>(m->v + 2 * at),
                                 reinterpret_cast<float4 *>(m->F + 4 * at), reinterpret_cast<float4 *>(m->B + 4 * at), m->aux + at,
                                 m->gid + at, m->pid + at}))
      return rc;
    m->next_pid += (int32_t)n;
    m->n += n;
    return MPMHIP_OK;
  }
};

template <class A>
__attribute__((format(printf, 3, 4))) int seed_fail(typename A::Ctx *c, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return A::fail(c, code, buf);
}
#define SEED_FAIL(...) return seed_fail<A>(c, MPMHIP_EINVAL, __VA_ARGS__)
#define SEED_HIP(call)                                                                                                  \
  do {                                                                                                                  \
    const hipError_t e_ = (call);                                                                                       \
    if (e_ != hipSuccess) return seed_fail<A>(c, MPMHIP_EHIP, "%s failed: %s", #call, hipGetErrorString(e_));          \
  } while (0)
#define SEED_LAUNCHED(what)                                                                                             \
  do {                                                                                                                  \
    const hipError_t e_ = hipGetLastError();                                                                            \
    if (e_ != hipSuccess) return seed_fail<A>(c, MPMHIP_EHIP, "launch of %s failed: %s", what, hipGetErrorString(e_)); \
  } while (0)

// the region of a seeding call as the kernels take it; a sampled field is uploaded into the ctx's buffer
template <class A>
int seed_region(typename A::Ctx *c, const typename A::Desc *d, typename A::Region &R) {
  constexpr int D = A::D;
  memset(&R, 0, sizeof R);
  if (!d->sdf) return A::shapes(c, d, R);
  const auto *L = d->sdf;
  if (!d->phi) SEED_FAIL("seed_particles: a sampled region needs its phi array");
  std::string why;
  const size_t count = sdf_lattice::check<D>(L->res, L->origin, L->spacing, why);
  if (!count) SEED_FAIL("seed_particles: %s", why.c_str());
  SeedWork &W = c->seed;
  if (count > W.phi_cap || !W.d_phi) {
    W.phi_cap = 0;
    if (W.d_phi.alloc(count) != hipSuccess)
      return seed_fail<A>(c, MPMHIP_ENOMEM, "seed_particles: device allocation of %zu bytes failed", count * sizeof(float));
    W.phi_cap = count;
  }
  SEED_HIP(hipMemcpyAsync(W.d_phi, d->phi, sizeof(float) * count, hipMemcpyHostToDevice, c->stream));
  sdf_fill<D>(R.sdf, *L, W.d_phi, nullptr, 0.0f, 1.0f);  // one frame
  return MPMHIP_OK;
}

// get_ready + the replicas (src/poisson_disk_sampler.h:34-69, :166-173) from the box of inside cell centres, in fp32.  The replicas
// per axis stay floats and their product a double until the candidates are known to fit: a tiny spacing gives more than an integer
// holds.  The product is exact where it counts: up to 2^31 every partial product is an integer a double holds, beyond it the
// rounded value is beyond it too.
template <class A>
double seed_get_ready(const typename A::Ctx *c, float ppc, const int *box, SeedParams<A::D> &S, float nrep[A::D]) {
  SEED_NO_CONTRACT
  constexpr int D = A::D;
  const float dx = c->P.dx;
  double v = (double)dx, n_rep = 1.0;
  for (int k = 1; k < D; k++) v = v * (double)dx;
  S.min_distance = A::min_distance(v / (double)ppc);
  S.region_size = 40.0f * S.min_distance;
  for (int k = 0; k < D; k++) {
    const float lo = ((float)box[k] + 0.5f) * dx, hi = ((float)box[D + k] + 0.5f) * dx;
    const float min_corner = lo - dx, max_corner = hi + dx;
    const float size = max_corner - min_corner;
    S.min_corner[k] = min_corner;
    nrep[k] = std::max(1.0f, std::ceil(size / S.region_size));
    n_rep *= (double)nrep[k];
  }
  return n_rep;
}

// what a call reports beside its code: the particles added here and job-wide (SEED_WHOLE: the same number; on MPMHIP_ECAPACITY what
// is needed here), and for SEED_HIST where the histograms go
struct SeedOut {
  int64_t here = 0, job = 0;
  int64_t *hist[3] = {nullptr, nullptr, nullptr}, *total = nullptr;
  int32_t *cell_bounds = nullptr;
};

// `make(R)` builds the region the kernels take (a plain one: seed_region; an expression: region_api.h) once the call's other
// arguments have passed; the kernels are instantiated for its type.  CALL picks what follows the get-ready pass, which all share:
//   SEED_WHOLE  k_seed_count, k_seed_scan, k_seed_write: every survivor becomes a particle of this ctx
//   SEED_BRICK  k_seed_count_brick, k_seed_scan2, k_seed_write_brick: the survivors of this rank's brick do, with the ids all ranks agree on
//   SEED_HIST   k_seed_hist: nothing is written, no group is read, no counter moves
template <class A, class Region, SeedCall CALL, class Make>
int seed_particles_as(typename A::Ctx *c, int32_t group, const typename A::Desc *d, SeedOut &out, Make make) {
  SEED_NO_CONTRACT
  constexpr int D = A::D;
  static_assert(CALL == SEED_WHOLE || D == 3, "bricks and their histograms: the 3D ctx only");
  if (!c) return MPMHIP_EINVAL;
  if (!d) SEED_FAIL("seed_particles: the description is required");
  if (const char *why = A::refused(c, CALL)) return A::fail(c, MPMHIP_EINVAL, why);
  if (CALL != SEED_HIST && (group < 0 || group >= (int)c->groups.size())) SEED_FAIL("unknown group %d", group);
  if (!(d->ppc > 0.0f) || !std::isfinite(d->ppc)) SEED_FAIL("seed_particles: ppc must be a finite number > 0");
  for (int k = 0; k < D; k++)
    if (!std::isfinite(d->velocity[k])) SEED_FAIL("seed_particles: velocity[%d] is not finite", k);
  if (!std::isfinite(d->initial_dg)) SEED_FAIL("seed_particles: initial_dg is not finite");
  if (d->source && !std::isfinite(d->source_delta_t)) SEED_FAIL("seed_particles: source_delta_t is not finite");
  SEED_HIP(hipSetDevice(c->device));
  SEED_HIP(hipStreamSynchronize(c->stream));
  Region R;
  if (int rc = make(R)) return rc;
  SeedWork &W = c->seed;
  if (!W.d_tile) {
    const std::vector<float> &t = poisson_tile::tile<D>();
    if (W.d_tile.alloc(t.size()) != hipSuccess) return seed_fail<A>(c, MPMHIP_ENOMEM, "seed_particles: device allocation of the tile failed");
    W.n_tile = (uint32_t)(t.size() / D);
    SEED_HIP(hipMemcpyAsync(W.d_tile, t.data(), sizeof(float) * t.size(), hipMemcpyHostToDevice, c->stream));
  }
  if (!W.d_box) SEED_HIP(W.d_box.alloc(2 * D + 2));

  SeedParams<D> S;
  memset(&S, 0, sizeof S);
  uint64_t cells = 1;
  for (int k = 0; k < D; k++) { S.res[k] = c->P.res[k]; cells *= (uint64_t)S.res[k]; }
  S.dx = c->P.dx; S.idx = c->P.idx;
  // ---- get ready: the box of the cell centres inside the region
  int box[2 * D + 2] = {};  // min per axis, max per axis, the survivors' count, a pad
  for (int k = 0; k < D; k++) { box[k] = 0x7fffffff; box[D + k] = -1; }
  SEED_HIP(hipMemcpyAsync(W.d_box, box, sizeof box, hipMemcpyHostToDevice, c->stream));
  const uint32_t bounds_wgs = (uint32_t)std::min<uint64_t>((cells + SEED_WG - 1) / SEED_WG, A::max_bounds_wgs(c));
  hipLaunchKernelGGL((k_seed_bounds<D, Region>), dim3(bounds_wgs), dim3(SEED_WG), 0, c->stream, R, S, W.d_box.get());
  SEED_LAUNCHED("seed_bounds");
  SEED_HIP(hipMemcpyAsync(box, W.d_box, sizeof box, hipMemcpyDeviceToHost, c->stream));
  SEED_HIP(hipStreamSynchronize(c->stream));
  if (box[D] < 0) SEED_FAIL("seed_particles: region is empty (no cell centre of the grid lies inside it)");
  float nrep[D];
  const double n_rep = seed_get_ready<A>(c, d->ppc, box, S, nrep);
  const double n_cand = n_rep * (double)W.n_tile;
  if (!(n_cand <= 2147483648.0))
    SEED_FAIL("seed_particles: more than 2^31 candidates (%u tile points x %.0f replicas): lower ppc or seed the region in parts", W.n_tile, n_rep);
  for (int k = 0; k < D; k++) S.nrep[k] = (uint32_t)nrep[k];
  S.n_rep = (uint32_t)n_rep; S.n_tile = W.n_tile; S.n_cand = (uint32_t)n_cand;
  S.source = d->source != 0;
  const int mat = CALL == SEED_HIST ? 0 : c->groups[group].type;
  for (int k = 0; k < D; k++) {
    S.velocity[k] = d->velocity[k];
    if (S.source) {  // src/mpm.cpp:222-227
      const float dt = d->source_delta_t;
      S.offset[k] = d->velocity[k] * c->t;
      const float a = d->velocity[k] * dt, b = 0.5f * c->P.g[k];
      const float e = b * (dt + A::base_dt(c));
      S.advection[k] = a + e * dt;
    }
  }
  S.dg = d->initial_dg;
  S.aux = (mat == MPMHIP_SNOW || mat == MPMHIP_WATER) ? 1.0f : (mat == MPMHIP_VISCO ? 1000.0f : 0.0f);  // as the ctx's add_particles
  S.gid = group;
  S.pid0 = c->next_pid;
  if constexpr (CALL == SEED_HIST) {
    // ---- the histograms: rows of res[a] words per axis, zeroed, counted on the device, widened on the way out
    uint32_t sum = 0;
    for (int k = 0; k < D; k++) sum += (uint32_t)S.res[k];
    if (sum > W.hist_cap || !W.d_hist) {
      W.hist_cap = 0;
      if (W.d_hist.alloc(sum) != hipSuccess) return seed_fail<A>(c, MPMHIP_ENOMEM, "seed_histogram: device allocation of %u words failed", sum);
      W.hist_cap = sum;
    }
    SEED_HIP(hipMemsetAsync(W.d_hist, 0, sizeof(uint32_t) * sum, c->stream));
    const uint32_t chunks = (uint32_t)(((uint64_t)S.n_cand + SEED_WG - 1) / SEED_WG);
    const size_t lds = sizeof(uint32_t) * sum;
    const int use_lds = lds <= 65536;  // (what a workgroup may ask for without more ado)
    const uint32_t wgs = std::min<uint32_t>(chunks, (uint32_t)c->n_cus * 8u);
    hipLaunchKernelGGL((k_seed_hist<D, Region>), dim3(wgs), dim3(SEED_WG), use_lds ? lds : 0, c->stream, R, S, (const float *)W.d_tile, chunks,
                       use_lds, W.d_hist.get());
    SEED_LAUNCHED("seed_hist");
    std::vector<uint32_t> h(sum);
    SEED_HIP(hipMemcpyAsync(h.data(), W.d_hist, sizeof(uint32_t) * sum, hipMemcpyDeviceToHost, c->stream));
    SEED_HIP(hipStreamSynchronize(c->stream));
    uint32_t at = 0;
    for (int k = 0; k < D; k++) {
      int64_t row = 0;
      int lo = 0x7fffffff, hi = -1;
      for (int i = 0; i < S.res[k]; i++) {
        const uint32_t v = h[at + (uint32_t)i];
        if (out.hist[k]) out.hist[k][i] = (int64_t)v;
        if (v) { lo = std::min(lo, i); hi = i + 1; }
        row += v;
      }
      if (out.cell_bounds) { out.cell_bounds[k] = hi < 0 ? 0 : lo; out.cell_bounds[D + k] = hi < 0 ? 0 : hi; }
      out.here = out.job = row;  // (every survivor counts once per axis)
      at += (uint32_t)S.res[k];
    }
    if (out.total) *out.total = out.job;
    return MPMHIP_OK;
  } else {
    // ---- count + scan
    const uint32_t wgs = (uint32_t)(((uint64_t)S.n_cand + SEED_PER_WG - 1) / SEED_PER_WG);
    if (wgs > W.wg_cap || !W.d_words) {
      W.wg_cap = 0;
      if (W.d_words.alloc((size_t)wgs * SEED_WORDS) != hipSuccess || W.d_totals.alloc(wgs) != hipSuccess)
        return seed_fail<A>(c, MPMHIP_ENOMEM, "seed_particles: device allocation for %u candidates failed", S.n_cand);
      W.wg_cap = wgs;
    }
    if constexpr (CALL == SEED_BRICK) {
      if (wgs > W.wg_cap2 || !W.d_words_mine) {
        W.wg_cap2 = 0;
        if (W.d_words_mine.alloc((size_t)wgs * SEED_WORDS) != hipSuccess || W.d_totals2.alloc((size_t)wgs + 1) != hipSuccess)
          return seed_fail<A>(c, MPMHIP_ENOMEM, "seed_particles: device allocation for %u candidates failed", S.n_cand);
        W.wg_cap2 = wgs;
      }
      SeedBricks K;
      memset(&K, 0, sizeof K);
      K.rank = c->T.rank;
      for (int a = 0; a < 3; a++) {
        K.dims[a] = c->T.dims[a];
        for (int k = 0; k <= c->T.dims[a]; k++) K.cuts[a][k] = c->T.cuts[a][k];
      }
      unsigned long long *d_total = W.d_totals2 + wgs;
      hipLaunchKernelGGL((k_seed_count_brick<D, Region>), dim3(wgs), dim3(SEED_WG), 0, c->stream, R, S, K, (const float *)W.d_tile,
                         W.d_words.get(), W.d_words_mine.get(), W.d_totals2.get());
      hipLaunchKernelGGL(k_seed_scan2, dim3(1), dim3(SEED_SCAN_WG), 0, c->stream, W.d_totals2.get(), wgs, d_total);
      SEED_LAUNCHED("seed_count_brick");
      unsigned long long total = 0;
      SEED_HIP(hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, c->stream));
      SEED_HIP(hipStreamSynchronize(c->stream));
      out.job = (int64_t)(total & 0xffffffffull);
      out.here = (int64_t)(total >> 32);
      if (out.job == 0) return MPMHIP_OK;
      // ---- the ctx's checks, then this brick's survivors go to its sink
      const int rc = A::commit(c, group, out.here, out.job, [&](auto sink) {
        hipLaunchKernelGGL((k_seed_write_brick<D, decltype(sink)>), dim3(wgs), dim3(SEED_WG), 0, c->stream, S, (const float *)W.d_tile,
                           (const unsigned long long *)W.d_words, (const unsigned long long *)W.d_words_mine,
                           (const unsigned long long *)W.d_totals2, sink);
        SEED_LAUNCHED("seed_write_brick");
        return (int)MPMHIP_OK;
      });
      if (!rc) A::appended_to_job(c, S);
      return rc;
    } else {
      uint32_t *d_total = reinterpret_cast<uint32_t *>(W.d_box + 2 * D);
      hipLaunchKernelGGL((k_seed_count<D, Region>), dim3(wgs), dim3(SEED_WG), 0, c->stream, R, S, (const float *)W.d_tile,
                         W.d_words.get(), W.d_totals.get());
      hipLaunchKernelGGL(k_seed_scan, dim3(1), dim3(SEED_SCAN_WG), 0, c->stream, W.d_totals.get(), wgs, d_total);
      SEED_LAUNCHED("seed_count");
      uint32_t total = 0;
      SEED_HIP(hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, c->stream));
      SEED_HIP(hipStreamSynchronize(c->stream));
      const int64_t n = (int64_t)total;
      out.here = out.job = n;
      if (n == 0) return MPMHIP_OK;
      // ---- the ctx's checks, then the survivors go to its sink
      return A::commit(c, group, n, n, [&](auto sink) {
        hipLaunchKernelGGL((k_seed_write<D, decltype(sink)>), dim3(wgs), dim3(SEED_WG), 0, c->stream, S, (const float *)W.d_tile,
                           (const unsigned long long *)W.d_words, (const uint32_t *)W.d_totals, sink);
        SEED_LAUNCHED("seed_write");
        return (int)MPMHIP_OK;
      });
    }
  }
}

// the existing calls' shape: one count out, zero until the call knows better
template <class A, class Region, class Make>
int seed_particles_whole(typename A::Ctx *c, int32_t group, const typename A::Desc *d, int64_t *n_added, Make make) {
  SeedOut out;
  const int rc = seed_particles_as<A, Region, SEED_WHOLE>(c, group, d, out, make);
  if (n_added) *n_added = out.here;
  return rc;
}

template <class A>
int seed_particles(typename A::Ctx *c, int32_t group, const typename A::Desc *d, int64_t *n_added) {
  return seed_particles_whole<A, typename A::Region>(c, group, d, n_added, [&](typename A::Region &R) { return seed_region<A>(c, d, R); });
}

#undef SEED_FAIL
#undef SEED_HIP
#undef SEED_LAUNCHED
#undef SEED_NO_CONTRACT

}  // namespace
}  // extern "C++"

int64_t mpmhip_poisson_tile(float *out, int64_t capacity) { return seed_tile_out<3>(out, capacity); }
int64_t mpmhip2d_poisson_tile(float *out, int64_t capacity) { return seed_tile_out<2>(out, capacity); }

int mpmhip_seed_particles(mpmhip_ctx *c, int32_t group, const mpmhip_seed_desc *d, int64_t *n_added) {
  return seed_particles<Seed3>(c, group, d, n_added);
}
int mpmhip2d_seed_particles(mpmhip2d_ctx *m, int32_t group, const mpmhip2d_seed_desc *d, int64_t *n_added) {
  return seed_particles<Seed2>(m, group, d, n_added);
}
