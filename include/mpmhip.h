/* include/mpmhip.h — C ABI of the MI355X-native MLS-MPM time-stepping core (libmpmhip.so).
 *
 * This is the drop-in boundary for the hot path of yuanming-hu/taichi_mpm: the per-substep
 * sequence  sort -> P2G -> grid normalise + boundary -> G2P -> boundary cleanup  that the
 * reference runs on the CPU inside `MPM<3>::substep()` (src/mpm.cpp:452-575).  The reference has
 * no C ABI (it is a factory-registered C++ class reached through pybind11, src/mpm.cpp:983-988);
 * each entry point below names the reference interface it replaces, and INTEGRATION.md shows the
 * binding a maintainer of the reference would add on top of it.
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; `void* stream` is a hipStream_t.
 *   - every function returns 0 on success or a negative MPMHIP_E* code; it never throws.
 *     `mpmhip_last_error()` returns a human-readable message for the last failure on that ctx
 *     (reference behaviour: TC_ASSERT/TC_ERROR abort, e.g. src/mpm.cpp:41-42,154,162,775).
 *   - host buffers are caller-owned; the `*_dev` variants (mpmhip_download_dev, mpmhip_upload_dev, mpmhip_download_grid_dev)
 *     take caller-owned device pointers of the ctx's device.
 *   - one ctx per GPU; calls on one ctx must be serialised by the caller (reference: not
 *     re-entrant either).
 *   - 3x3 matrices are row-major float[9]; `B` is the reference's `apic_b` (sign/units of
 *     src/transfer.cpp:898-903: B = sum_i w_i v_i (x_p - x_i)^T / dx).
 */
#ifndef MPMHIP_H
#define MPMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPMHIP_ABI_VERSION 3  /* 2: mpmhip_async_config gained left_boundary; 3: the native data plane of tiled runs (mpmhip_tiled_*, mpmhip_comm_*) */

enum {
  MPMHIP_OK = 0,
  MPMHIP_EINVAL = -1,    /* bad argument / unsupported configuration */
  MPMHIP_ENOMEM = -2,    /* device or host allocation failed, or capacity exceeded */
  MPMHIP_EHIP = -3,      /* a HIP runtime call failed (message in last_error) */
  MPMHIP_ECAPACITY = -4, /* more particles / active blocks than the ctx was created for */
  MPMHIP_ENOTIMPL = -5
};

/* material ids == y component of MPMParticle::get_debug_info() (src/particles.cpp:157..839);
 * names are the factory aliases of TC_REGISTER_MPM_PARTICLE (src/particles.cpp:849-856). */
enum {
  MPMHIP_VISCO = 1,
  MPMHIP_SNOW = 2,
  MPMHIP_LINEAR = 3,
  MPMHIP_JELLY = 4,
  MPMHIP_WATER = 5,
  MPMHIP_SAND = 6,
  MPMHIP_VON_MISES = 7,
  MPMHIP_ELASTIC = 8
};

#define MPMHIP_NPARAM 16
/* per-group parameter row float[16] (a "group" = one add_particles() call of the reference,
 * src/mpm.cpp:77-148: same type, same material constants, mass = vol*density):
 *   [0] mass [1] vol
 *   snow      [2] mu_0 [3] lambda_0 [4] hardening [5] theta_c [6] theta_s [7] min_Jp [8] max_Jp ; aux = Jp
 *   linear    [2] mu   [3] lambda
 *   jelly     [2] mu   [3] lambda
 *   water     [2] k    [3] gamma                                                             ; aux = j
 *   sand      [2] mu_0 [3] lambda_0 [4] alpha [5] cohesion [6] beta                           ; aux = logJp
 *   von_mises [2] mu_0 [3] lambda_0 [4] yield_stress
 *   elastic   [2] mu_0 [3] lambda_0 [4] E (reported by get_debug_info() only, src/particles.cpp:838-840)
 *   visco     [2] mu_0 [3] lambda_0 [4] visco_nu [5] visco_kappa [6] base_delta_t                ; aux = visco_tau
 */

/* replaces: Config keys read by MPM<dim>::initialize (src/mpm.cpp:26-75) */
typedef struct {
  int32_t res[3];           /* "res": cells per axis (nodes = res+1) */
  float dx;                 /* "delta_x" (python default 1/res[0], scripts/async/async_mpm.py:40-41) */
  float dt;                 /* "base_delta_t" * "dt_multiplier" */
  float gravity[3];         /* "gravity" (default (0,-10,0)) */
  int32_t particle_gravity; /* "particle_gravity" (default 1): gravity added to particles before P2G */
  float apic_damping;       /* "apic_damping" */
  float rpic_damping;       /* "rpic_damping" */
  int32_t clean_boundary;   /* "clean_boundary" (default 1): src/mpm.cpp:563-565 */
  /* analytic level set (replaces set_levelset(DynamicLevelSet)): up to 8 half-spaces
   * phi(x) = n.x + d in world units (|n| = 1), combined with min(); phi<0 inside the solid */
  int32_t n_planes;
  float planes[8][4];
  float friction;           /* levelset friction code: -1 sticky, <=-2 slip, >=0 separate (README.md:326-330) */
  int64_t max_particles;    /* capacity of the SoA pools (reference: < 2^25, src/mpm.cpp:773-775) */
  int64_t max_blocks;       /* capacity of the active-block table; 0 = choose from max_particles */
  int32_t device;           /* HIP device ordinal */
  int32_t reorder_interval; /* "reorder_interval" (src/mpm.cpp:45,811-813): physical reorder of the particle records
                               into sorted order every this many substeps; 0 = never (the sorted INDEX is rebuilt
                               every substep regardless) */
  int32_t particle_collision; /* "particle_collision" (default 0): particle_collision_resolution after G2P, src/mpm.cpp:414-426,566-569 */
  int32_t discard_apic_b;   /* 1 = G2P does not store apic_b: it lives on folded into the P2G affine matrix
                               A = stress*(-4 inv_dx dt) + apic_b*(4 m) (src/transfer.cpp:521-522), which is the state
                               the next substep consumes (-48 of 180 stored bytes per particle-step).  download(B)
                               then recovers apic_b = (A - stress(F) S)/(4 m) on demand, to ~1e-5..1e-4 relative */
  int32_t generic_path;     /* config "optimized" = false: the reference's generic transfer path (src/transfer.cpp:193-278,
                             * 585-687).  Same arithmetic as the optimised path here (both go through the same kernels); what
                             * differs in the reference is the position clamp into [0, res - eps] after the advection
                             * (:668-670), which this flag turns on */
  int32_t deterministic;    /* 1 = bitwise reproducible runs: every cell's particles are put in ascending creation id behind the sort
                             * (the in-cell ranks of the counting sort come from atomics, so without it the summation order of P2G's
                             * per-cell sums — and the last bits of everything downstream — differs from run to run).  Two runs of one
                             * scene, the packed and the per-block G2P walk, the three- and the four-launch sort, and a tiled job over any
                             * wire then give identical bits; a K-rank job differs from the one-ctx run only by how the <= 8 block tiles of
                             * a halo node are grouped into rank partials.  Costs one more launch per sort (bench.py reports it).
                             * Also covered: the impulse / torque sums of CPIC rigid bodies (per flagged block a row of per-body sums,
                             * added in block order by one more launch per transfer — independent of launch sizes, the second stream and
                             * the slots) and calculate_energy (partial sums per node block / per sorted particle range, added in a fixed
                             * order; both grid walks give the same bits).  Switching the mode on takes effect from the next substep.
                             * The 2D solver has its own form of the mode (mpmhip2d_config.deterministic below: a cell sort and a
                             * gather P2G).  The asynchronous steppers, 2D and 3D, are covered: in the mode their containers are placed by
                             * ordered stream compactions, not by order of arrival (mpmhip_async_forms).
                             * The reference's sort key is unique for the same purpose: (offset >> 5) << 25 | i, src/mpm.cpp:785-795.
                             * env MPMHIP_DETERMINISTIC=0/1 overrides */
  int32_t reserved[2];
} mpmhip_config;

typedef struct mpmhip_ctx mpmhip_ctx;

/* particle fields for upload/download; element = one particle's record of `width` scalars */
enum {
  MPMHIP_F_X = 0,   /* float[3]  position (world units)                MPMParticle::pos      */
  MPMHIP_F_V = 1,   /* float[3]  velocity                              get_velocity()        */
  MPMHIP_F_B = 2,   /* float[9]  apic_b                                MPMParticle::apic_b   */
  MPMHIP_F_F = 3,   /* float[9]  elastic deformation gradient          MPMParticle::dg_e     */
  MPMHIP_F_AUX = 4, /* float[1]  Jp | j | logJp (material state)                             */
  MPMHIP_F_GID = 5, /* int32[1]  group id                                                    */
  MPMHIP_F_ID = 6,  /* int32[1]  creation index (MPMParticle::id semantics for download ordering) */
  MPMHIP_F_STATES = 7 /* int32[1] CPIC colour word (MPMParticle::states, src/particles.h): 2 bits per rigid body */
};

uint32_t mpmhip_abi_version(void);

/* lifecycle — replaces create_instance<Simulation3D>("mpm") + MPM<3>::initialize (src/mpm.cpp:26-75) */
int mpmhip_create(const mpmhip_config *cfg, mpmhip_ctx **out);
void mpmhip_destroy(mpmhip_ctx *ctx);
const char *mpmhip_last_error(const mpmhip_ctx *ctx); /* ctx may be NULL: last create() failure */
int mpmhip_set_stream(mpmhip_ctx *ctx, void *hip_stream); /* NULL = the ctx's own stream */
/* mpmhip_config.deterministic of a live ctx (from the next sort on; no reference counterpart: its scalar path has one order) */
int mpmhip_set_deterministic(mpmhip_ctx *ctx, int32_t enabled);
/* replaces Simulation::set_levelset(DynamicLevelSet) (scripts/async/async_mpm.py:119-127) for analytic half-spaces */
int mpmhip_set_levelset(mpmhip_ctx *ctx, int32_t n_planes, const float *planes /* [n][4] */, float friction);

/* general analytic level set: union of up to MPMHIP_MAX_SHAPES solids, phi = min over shapes, negative inside a
 * solid; replaces the LevelSet the scene scripts build with add_plane / add_sphere / add_cuboid
 * (e.g. scripts/mls-cpic/goo_blocks.py:17-20, scripts/async/sand.py:34-37).  World units.
 *   type 0 plane  p = {nx, ny, nz, d}            phi = n.x + d            (|n| = 1)
 *   type 1 sphere p = {cx, cy, cz, r}            solid ball;  inside_out = 1: the ball is the FREE space
 *   type 2 cuboid p = {lo x,y,z, hi x,y,z}       solid box;   inside_out = 1: the box is a container */
#define MPMHIP_MAX_SHAPES 16
typedef struct {
  int32_t type, inside_out;
  float p[6];
} mpmhip_shape;
int mpmhip_set_levelset_shapes(mpmhip_ctx *ctx, int32_t n, const mpmhip_shape *shapes, float friction);
/* MPM<dim>::rigid_body_levelset_collision (src/mpm_rigid_body.cpp:347-387; config key rigid_body_levelset_collision, run between
 * normalize_grid and the grid boundary condition, src/mpm.cpp:535-538): every boundary particle of a rigid body below the level
 * set gives its body a normal impulse (restitution) and a Coulomb friction impulse (friction0) at once, so that the next boundary
 * particle sees the changed velocity — in the order of the reference's sorted particle list, which the library keeps for the
 * boundary particles (sort key of src/mpm.cpp:785-790, ties by the position in the previous order). */
int mpmhip_set_rigid_levelset_collision(mpmhip_ctx *ctx, int32_t enabled);
/* MPM<3>::apply_dirichlet_boundary_conditions (src/mpm.cpp:401-412; runs behind the grid boundary condition when the config key
 * dirichlet_boundary_radius is > 0, :541-544): grid nodes with y > 0.525 are held at rest (the reference's 3D form ignores the
 * radius and hard-codes the plane) */
int mpmhip_set_dirichlet(mpmhip_ctx *ctx, int32_t enabled);
/* time-dependent level set — replaces DynamicLevelSet::initialize(t0, t1, levelset(t0), levelset(t1)) +
 * Simulation::set_levelset as the python driver calls them before every frame (scripts/async/async_mpm.py:119-127,
 * e.g. the shrinking container of scripts/async/balls.py:38-49): two key frames blended linearly in time; at time t
 * phi = lerp(phi0, phi1), the normal is the normalised lerp of the two gradients, and the grid boundary condition
 * uses boundary_velocity = -(phi1 - phi0)/(t1 - t0) n delta_x (src/mpm.cpp:323-342).  t = the ctx's current time. */
int mpmhip_set_levelset_keyframes(mpmhip_ctx *ctx, float t0, float t1, int32_t n0, const mpmhip_shape *shapes0,
                                  int32_t n1, const mpmhip_shape *shapes1, float friction);

/* Sampled level set: a signed-distance field on a regular lattice instead of shapes — boundaries of any form (the reference's
 * LevelSet IS a sampled array, taichi core; add_plane / add_sphere / add_cuboid only fill it and MPM<dim>::substep reads it
 * through sample(), get_spatial_gradient(), get_temporal_derivative(): src/mpm.cpp:313-368, :414-426).  The taichi core is not
 * vendored, so the sampling rules are this library's own:
 *   lattice   res[k] >= 2 samples per axis, sample (0, 0, 0) at `origin`, one `spacing` > 0 (world units, independent of the
 *             simulation's delta_x); arrays in C order [i][j][k] (k fastest), fp32, WORLD units, negative inside the solid.  The
 *             library keeps its own device copy (4 res[0] res[1] res[2] bytes per key frame).
 *   phi       trilinear interpolation in the cell that holds the point, returned in grid units.  A point outside
 *             [origin, origin + (res - 1) spacing] on any axis has NO level set there: nothing is extrapolated.
 *   gradient  trilinear interpolation of the eight samples' central-difference gradients (one-sided on the array's faces),
 *             normalised; a length below 1e-10 gives the zero vector.
 *   phi1      NULL: static.  Else a second key frame on the same lattice: phi = lerp(phi0, phi1), the normal is the normalised lerp
 *             of the two unit gradients, d phi / dt = (phi1 - phi0) / (t1 - t0) — mpmhip_set_levelset_keyframes for samples.
 * One level set at a time: a sampled set replaces the shapes and shapes replace a sampled set.  friction as above;
 * particle_collision and mpmhip_delete_particles_inside_level_set work with it.  A call with the lattice size of the installed set
 * reuses the device memory (the per-frame update of a dynamic level set allocates nothing).
 * The 2D solver takes a sampled boundary through mpmhip2d_set_levelset_sdf (below, the same rules with one axis fewer).
 * Out of scope: the reference's add_slope, open or self-intersecting meshes (closed triangle meshes are voxelised on the device:
 * mpmhip_set_levelset_mesh below; there is no mesh or outline voxeliser for 2D), and rigid_body_levelset_collision with a sampled
 * set (refused with MPMHIP_EINVAL, here and in mpmhip_set_rigid_levelset_collision; the 2D calls refuse it alike).
 * Tiled jobs and the asynchronous stepper go through the same per-ctx call and substep; they are not tested with it. */
typedef struct {
  int32_t res[3];
  float origin[3];
  float spacing;
} mpmhip_sdf_desc;
int mpmhip_set_levelset_sdf(mpmhip_ctx *ctx, const mpmhip_sdf_desc *desc, const float *phi0, const float *phi1 /* NULL = static */,
                            float t0, float t1, float friction);
/* the DEVICE's level-set evaluation (whatever is installed: a sampled set or shapes) at n host-given points at time t:
 * phi [n] in grid units, grad [n][3] the unit gradient, dphidt [n], hit [n] = 0 where there is no level set (then the rest is 0) */
int mpmhip_debug_levelset_sample(mpmhip_ctx *ctx, int64_t n, const float *pos /* [n][3] */, float t, float *phi, float *grad,
                                 float *dphidt, int32_t *hit);

/* Triangle mesh -> sampled level set, voxelised on the device (the reference's scenes give bowls, cutters and wheels as .obj
 * files; its LevelSet is filled from a mesh by the taichi core, which is not vendored, so the rules are this library's own).
 * Input: n_tri triangles, float [n_tri][3][3] in world units; a lattice as above; band > 0 in world units, +inf allowed.
 * Output per sample: phi = s * min(d, band), fp32, world units, C order.  Sample (i, j, k) sits at fl(origin + fl(index * spacing))
 * per axis, in fp32.
 *   d      the Euclidean distance to the nearest triangle: the exact closest point of each triangle by its regions (three
 *          vertices, three edges, the face), evaluated in fp32.  A triangle's vertices are first put in lexicographic order, so its
 *          orientation and vertex order do not reach any number.  Triangles of zero area (cross product exactly 0) are skipped.
 *   s      -1 iff the ray from the sample towards +k (the array's fastest axis) crosses an odd number of triangles, else +1:
 *          independent of the triangles' orientation and order.  Column (x, y) lies in a triangle's xy-projection iff the ray from
 *          (x, y) towards +x crosses an odd number of its three projected edges.  An edge is crossed iff exactly one end point has
 *          y' > y (half-open: an end point AT y counts as below) and the edge function, taken from the lower end point in fp64 on
 *          differences of the fp32 inputs (differences and products exact, the sign of the result exact), is > 0: a point ON an
 *          edge does not cross it.  The decision depends on the edge and the column only, so the two triangles sharing an edge
 *          always agree and every column of a closed mesh crosses it an even number of times, however vertices, edges and faces
 *          line up with the lattice.  A projection of zero area contributes nothing.  The crossing height is interpolated in fp64
 *          and a sample is below it iff crossing > the sample's own height.
 *   closed a column with an ODD total of crossings means the mesh is not closed: the call fails with MPMHIP_EINVAL, the message
 *          says how many columns were odd, nothing is installed and no output array is written.  (An even column proves nothing: a
 *          hole seen exactly edge-on from +k crosses no column.  Open and self-intersecting meshes are out of scope beyond this.)
 *   band   finite: the field is exact wherever d < band and exactly +-band elsewhere (bitwise the +inf result where that is inside
 *          the band).  What the consumers need: the grid pass reads -3 <= phi <= 0 grid units, plus one interpolation cell, plus
 *          the central-difference neighbours, so band >= 3 delta_x + 2 spacing gives the grid pass the bits an unclamped field
 *          gives.  Where the field is clamped the sampled normal is the zero vector: particle_collision does not push a particle
 *          that is deeper inside than the band.
 * The result is a pure function of the triangle SET and the lattice: two runs, a shuffled list, reversed orientations give the same
 * bits (minimum and parity are order-free; no float atomics).  MPMHIP_EINVAL for: a non-finite vertex, n_tri <= 0 (or > 2^26),
 * band <= 0 or NaN, a lattice mpmhip_set_levelset_sdf refuses, res[2] > 8191, a mesh of zero-area triangles only.
 *
 * mpmhip_mesh_to_sdf: no ctx, voxelises on `device` into the host array phi_out [res0 * res1 * res2] (replaces a point-to-mesh
 * distance written in numpy in front of SampledLevelSet; a cached result goes back in through mpmhip_set_levelset_sdf).  Errors:
 * mpmhip_last_error(NULL), as for mpmhip_create. */
int mpmhip_mesh_to_sdf(int32_t device, const mpmhip_sdf_desc *desc, int32_t n_tri, const float *tri /* [n_tri][3][3] */, float band,
                       float *phi_out);
/* mpmhip_set_levelset_sdf with the key frames given as meshes (replaces host voxelisation + the upload of the arrays, twice per
 * frame for a moving boundary): voxelises on the ctx's stream straight into the ctx's device arrays and installs the set exactly as
 * mpmhip_set_levelset_sdf does — the same refusals (inside a substep, with rigid_body_levelset_collision), the same reuse of the
 * device memory for an unchanged lattice, the same aligned / one-load decision.  tri1 == NULL: static (n_tri1, t0, t1 ignored).
 * The triangle and list buffers are kept between calls too; no lattice-sized host array exists at any point.  Both meshes are
 * judged before the installed level set is touched: a refused call leaves it in force. */
int mpmhip_set_levelset_mesh(mpmhip_ctx *ctx, const mpmhip_sdf_desc *desc, int32_t n_tri0, const float *tri0, int32_t n_tri1,
                             const float *tri1 /* NULL = static */, float t0, float t1, float band, float friction);
/* reads back key frame `frame` (0, or 1 of a two-frame set) of the installed sampled level set, however it was installed:
 * sdf_count floats in C order, world units; capacity = room in dst, in floats.  For caching a voxelisation and for tests. */
int mpmhip_download_levelset_sdf(mpmhip_ctx *ctx, int32_t frame, float *dst, int64_t capacity);

/* A ctx holds at most MPMHIP_MAX_GROUPS groups (k_g2p mirrors the whole group table in LDS). */
#define MPMHIP_MAX_GROUPS 64
/* particles — replaces MPM<3>::add_particles (src/mpm.cpp:77-270) with caller-generated samples.
 * add_group returns the group id (>=0) or a negative error. F/B/aux may be NULL (identity/0/material default). */
int mpmhip_add_group(mpmhip_ctx *ctx, int32_t material, const float params[MPMHIP_NPARAM]);
int mpmhip_add_particles(mpmhip_ctx *ctx, int32_t group, int64_t n, const float *x, const float *v,
                         const float *F, const float *B, const float *aux);

/* Seeding on the device — replaces the reference's default fill, add_particles(density_tex=...) with pd / pd_periodic
 * (PoissonDiskSampler<3>::sample_from_periodic_data and, with pd_source, sample_from_source: src/poisson_disk_sampler.h:157-252,
 * src/mpm.cpp:205-251): a fixed periodic blue-noise tile is scaled to the wanted spacing, repeated over the region's bounding box,
 * and the points inside the region become particles.  No particle record passes through host memory
 * (mpmhip_host_particle_bytes does not change).
 *
 * The tile: mpmhip_poisson_tile writes min(count, capacity) points, 3 floats each, to `out` (NULL allowed) and returns the count.
 * Bridson's algorithm in the periodic box [-20, 20)^3, minimum distance 1, 30 attempts per active point, the first point at the
 * centre (write_periodic_data, :255-324), generated once per process in integer arithmetic: the same bytes on every machine.
 *
 * The region is "where this level set is negative", independent of the ctx's boundary level set (which is not touched):
 *   sdf == NULL   the first n_shapes of `shapes` (phi = min over the shapes, as mpmhip_set_levelset_shapes);
 *   sdf != NULL   a sampled field phi [res0 res1 res2] on the lattice *sdf (host array, uploaded by the call; the rules of
 *                 mpmhip_set_levelset_sdf: trilinear, a point outside the lattice is not in the region).
 * All arithmetic is fp32, in this order, nothing contracted (tests/seed_model.py restates it to the bit):
 *   get ready   over the cell centres fl((i + 0.5) dx) of the grid: min / max per axis of the centres inside the region;
 *               min_corner = min - dx, max_corner = max + dx; no centre inside: MPMHIP_EINVAL "region is empty".
 *               min_distance = (float)cbrt(dx^3 / ppc * 13 / 18) (in double), region_size = fl(40 min_distance),
 *               replicas per axis = ceil((max_corner - min_corner) / region_size).
 *   candidates  c = i * n_replicas + r pairs tile point i with replica r (the replica index in C order, (ind0, ind1, ind2));
 *               q = fl(tile_i * min_distance);  position = fl(fl(q + min_corner) + fl(region_size * (ind + 0.5))).
 *               source = 1 (an emitter called before every frame): q = fl(q + fl(velocity * current_t)), wrapped into the period
 *               q -= fl(floor(fl(fl(q / region_size) + 0.5)) * region_size) — the tile drifts with the jet.
 *   acceptance  inside the region and not within 7 cells of a wall (MPM::near_boundary, src/mpm.h:269-276: X = fl(x * fl(1 / dx)),
 *               min X < 7 or max (X - res) > -7).  source = 1: and position + advection is NOT inside, advection =
 *               velocity * d + 0.5 * gravity * (d + base_delta_t) * d with d = source_delta_t (src/mpm.cpp:222-227): only the shell
 *               the jet vacates within d is filled.
 *   order       the survivors are appended in ascending c with creation ids next_id + rank (the reference's order).
 *   records     velocity as given, F = initial_dg * I, B = 0, aux the material default, mass from the group row.
 * *n_added = the number of new particles.  If they do not fit the ctx, nothing is written, *n_added is the number needed and the
 * call returns MPMHIP_ECAPACITY: mpmhip_reserve and call again.  MPMHIP_EINVAL with a message: inside a substep, on a tiled ctx
 * (there: mpmhip_seed_particles_brick, below the region expressions), an unknown group, ppc <= 0, a lattice mpmhip_set_levelset_sdf would refuse, more than 2^31 candidates.
 * The 2D solver has the same call: mpmhip2d_seed_particles below.  Out of scope: pd_packed, non-uniform densities, pd = False,
 * point_cloud. */
typedef struct {
  int32_t n_shapes;
  mpmhip_shape shapes[MPMHIP_MAX_SHAPES];
  const mpmhip_sdf_desc *sdf; /* NULL: the region is given by the shapes */
  const float *phi;
  float ppc;                  /* particles per cell the spacing is chosen for (> 0) */
  float velocity[3];
  int32_t source;             /* 0 fill, 1 emitter shell */
  float source_delta_t;
  float initial_dg;
  int32_t reserved;
} mpmhip_seed_desc;
int64_t mpmhip_poisson_tile(float *out, int64_t capacity);
int mpmhip_seed_particles(mpmhip_ctx *ctx, int32_t group, const mpmhip_seed_desc *desc, int64_t *n_added);
int64_t mpmhip_num_particles(mpmhip_ctx *ctx); /* synchronises; <0 on error */
int mpmhip_download(mpmhip_ctx *ctx, int32_t field, void *dst, int64_t n_capacity); /* returns n written */
int mpmhip_upload(mpmhip_ctx *ctx, int32_t field, const void *src, int64_t n);
/* The same between the ctx and caller-owned DEVICE arrays (no reference counterpart: its particles live in host memory).  No record
 * and no row passes through host memory: mpmhip_host_particle_bytes does not change.
 * field tables: index = MPMHIP_F_*, NULL = field not wanted; device pointers of the ctx's device; row widths and scalar types as for
 * mpmhip_download (float[3], [3], [9], [9], [1]; int32 gid, id, states).  One call moves any subset of the fields and reads the
 * records once.
 *   order 0   slot order, live slots only: exactly the rows of mpmhip_download, in its order
 *   order 1   ascending creation id: row r holds the particle whose id has rank r among the live ids — the only order that survives a
 *             substep (the sort moves slots).  Needs unique live ids: MPMHIP_EINVAL ("the creation ids are not unique") otherwise,
 *             before a field or a destination is written (the recovery of stale apic_b rows, which mpmhip_upload_dev runs first
 *             as mpmhip_upload does, may have run by then; the same holds for an upload's wrong row count).
 * mpmhip_download_dev returns the rows written.  The live particles are counted first: n_capacity below them is MPMHIP_ECAPACITY
 * and no destination byte is touched; nothing is ever written behind the last row.  B runs the recovery of discard_apic_b first, as
 * the host call does.
 * mpmhip_upload_dev has the value semantics of mpmhip_upload per field (x into both records, a negative id stored as 0, the id
 * counter raised to 1 + the largest uploaded id and never lowered; MPMHIP_F_GID refused; n must be the live count) and changes only
 * the named fields of a record.  With order 1 the rows are matched to the ids the particles held BEFORE the call, also when ids
 * are uploaded.
 * Streams: the work runs on the ctx's stream and the call returns when that stream has drained, so the destinations are ready for any
 * stream; an upload's sources, and whatever else was enqueued on the arrays of either call, must be complete when the call is made.
 * MPMHIP_EINVAL with a message, nothing touched: a NULL table, a table of eight NULLs, an unknown order, inside a substep, a ctx with
 * a resident asynchronous stepper (the records only mirror the pools there: the host calls remain the way in).
 * The 2D solver has no such calls yet. */
int64_t mpmhip_download_dev(mpmhip_ctx *ctx, void *const dst[8], int64_t n_capacity, int32_t order); /* rows written, or < 0 */
int mpmhip_upload_dev(mpmhip_ctx *ctx, const void *const src[8], int64_t n, int32_t order);

/* time stepping — replaces MPM<3>::step / substep (src/mpm.cpp:428-450, 452-575) */
int mpmhip_substep(mpmhip_ctx *ctx);                 /* one substep, asynchronous on the ctx stream */
int mpmhip_run_substeps(mpmhip_ctx *ctx, int32_t n); /* n substeps back to back */
int mpmhip_step(mpmhip_ctx *ctx, float dt);          /* step(dt): dt<0 => one substep; else while (t + base_dt < request_t) substep */
double mpmhip_current_time(const mpmhip_ctx *ctx);   /* get_current_time() */
int mpmhip_synchronize(mpmhip_ctx *ctx);

/* phase-level entry points (parity tests) — each replaces the named reference function */
int mpmhip_sort(mpmhip_ctx *ctx);        /* sort_particles_and_populate_grid  src/mpm.cpp:770-918 (+ clear_boundary_particles :582-633) */
int mpmhip_p2g(mpmhip_ctx *ctx);         /* rasterize_optimized               src/transfer.cpp:361-581 */
int mpmhip_grid_update(mpmhip_ctx *ctx); /* normalize_grid_and_apply_external_force + apply_grid_boundary_conditions  src/mpm.cpp:277-372 */
int mpmhip_g2p(mpmhip_ctx *ctx);         /* resample_optimized                src/transfer.cpp:702-970 */

/* dense grid views, node-major float[(rx+1)(ry+1)(rz+1)][4], z fastest.
 *   which=0: (m*v, m) accumulated by P2G;  which=1: (v, m) after grid_update.
 * upload_grid installs a dense (v, m) field as the input of the next mpmhip_g2p (needs a prior sort). */
int mpmhip_download_grid(mpmhip_ctx *ctx, int32_t which, float *dst);
/* the array of mpmhip_download_grid into device memory of the ctx's device (copied device to device on the ctx's stream, which has
 * drained on return) */
int mpmhip_download_grid_dev(mpmhip_ctx *ctx, int32_t which, float *dst_dev);
int mpmhip_upload_grid(mpmhip_ctx *ctx, const float *src);

/* whole-state snapshots — replaces the TC_IO serialization behind general_action "save" / "load"
 * (src/mpm.cpp:940-960, src/mpm.h:38-54,134-169).  The blob holds the raw particle records (with the P2G affine
 * matrices), the group table and the clocks; it loads into a ctx of the same grid with enough capacity, which then
 * continues exactly where the saved run stopped.  Level set and config are NOT part of it (the reference re-reads
 * them from the scene script too). 
 * A scene with rigid bodies: the blob also carries the bodies' records (pose, velocities, mass properties) and the joints;
 * meshes, boundary particles and scripts come from the scene again — add the same bodies, in the same order, before loading. */
int64_t mpmhip_snapshot_size(mpmhip_ctx *ctx);
int mpmhip_snapshot_save(mpmhip_ctx *ctx, void *dst, size_t capacity);
int mpmhip_snapshot_load(mpmhip_ctx *ctx, const void *src, size_t size);
/* The snapshot of a whole tiled job (3D): ONE blob of the format above, whatever the job's rank count and cuts, in the format's
 * canonical form — no dead slot (n_slots = the job's live particles, n_dead = 0), the records in ascending creation id (the order
 * of the job's .bgeo frame), next_pid = max(the ranks' next ids, 1 + the largest live id).  mpmhip_snapshot_load on one ctx accepts
 * it unchanged; the blob is byte-identical for every partition over the same records.  Before anything is copied every rank makes
 * RecP.A current and, where it keeps apic_b (store_b), apic_b too: b_stale is 0 then, the ctx's own flag otherwise.
 *   mpmhip_snapshot_size_group / mpmhip_snapshot_save_group   the n_ctx ctx of one process on one device.  Ranked and placed on the
 *       device (the kernels of the frame of a job, below), one copy per section behind the header.  *written = the blob's bytes.
 *       MPMHIP_EINVAL, with the field and the rank in the message: substeps, t, request_t, dx, dt, res, store_b, b_stale or the
 *       group table differ between the ranks.  Refused as the frame of a job is: a ctx with rigid bodies, a resident asynchronous
 *       stepper, inside a substep, ctx on different devices or of different res, an id held twice.  A short dst: MPMHIP_ECAPACITY.
 *       dst is untouched on every refusal.
 *   mpmhip_snapshot_head         a rank per process: this rank's header (n_slots = its own live particles) and group table into dst,
 *                                *bytes = their size (dst NULL: the size alone).  The caller compares the ranks' heads.
 *   mpmhip_snapshot_rows_ranked  this ctx's records in ascending id into rows_host — 176 bytes a row: RecG | RecP | apic_b row — and
 *                                into row_index_host the number of each in the job's blob, between mpmhip_live_id_top /
 *                                mpmhip_id_bitmap and the caller's placement, as mpmhip_bgeo_rows_ranked. */
int mpmhip_snapshot_size_group(mpmhip_ctx *const *ctxs, int32_t n_ctx, size_t *bytes);
int mpmhip_snapshot_save_group(mpmhip_ctx *const *ctxs, int32_t n_ctx, void *dst, size_t capacity, size_t *written);
int mpmhip_snapshot_head(mpmhip_ctx *ctx, void *dst, size_t capacity, size_t *bytes);
int mpmhip_snapshot_rows_ranked(mpmhip_ctx *ctx, int64_t top, const uint32_t *union_words_host, void *rows_host, uint32_t *row_index_host,
                                int64_t capacity_rows, int64_t *written);
/* Loading a snapshot into a job of ANY rank count and cuts: every rank calls mpmhip_snapshot_load_brick with the same bytes — a job's
 * blob, or a one-ctx blob with dead slots; one with a rigid section is refused — on a ctx with a partition (mpmhip_set_partition or
 * mpmhip_tiled_setup; MPMHIP_EINVAL without).  The rank keeps exactly the live records whose base cell lies in its brick, by the
 * re-cut's rule to the bit, in slots [0, kept) in blob order: the ctx afterwards is a function of (blob, partition, rank).  The group
 * table, the particles and the clocks are replaced; next_pid is the header's on every rank; no slot is dead.  The blob passes the
 * device in chunks of records (1 Mi; MPMHIP_SNAP_CHUNK=n is a test knob read per call), twice: a rank never holds the whole blob.
 * info = {records kept here, live records of the blob, capacity this rank needs (MPMHIP_ECAPACITY only), live records no rank can
 * place (position not finite, or below 0.5 cells on an axis)}.  MPMHIP_ECAPACITY: the rank owns more records than its capacity;
 * nothing of the ctx was written — mpmhip_reserve, then repeat the call on every rank.  A ctx with the native data plane ends as
 * behind mpmhip_tiled_redistribute: clip box from the joint bounds of the blob's particles (the same on every rank, no message is
 * passed), the next advance begins with the planning scan.
 * mpmhip_snapshot_histogram: the per-axis histograms, cell bounds and number of the blob's live, placeable records — the outputs of
 * mpmhip_live_histogram, counted on the device from the staged chunks — on any ctx of the blob's grid, tiled or not; nothing of the
 * ctx is written.  What a restart on another rank count cuts its bricks from before any rank holds a particle. */
int mpmhip_snapshot_load_brick(mpmhip_ctx *ctx, const void *src, size_t size, int64_t info[4]);
int mpmhip_snapshot_histogram(mpmhip_ctx *ctx, const void *src, size_t size, int64_t *hist_x, int64_t *hist_y, int64_t *hist_z,
                              int32_t lo[3], int32_t hi[3], int64_t *total);

/* replaces MPM<3>::calculate_energy (src/mpm.cpp:1078-1110; general_action "calculate_energy", :936-938): sorts and
 * rasterizes, then kinetic = sum over grid nodes of 1/2 m |v|^2, potential = sum of MPMParticle::potential_energy()
 * (defined for linear, jelly, elastic: src/particles.cpp:323-327,400-407,785-796).  Returns MPMHIP_ENOTIMPL (with a
 * valid *kinetic) if a live particle is of another type, as the reference aborts there.  Synchronises.
 * On a ctx of a tiled job (mpmhip_tiled_setup, wires RCCL / IPC) the call is COLLECTIVE and returns the energy of the whole job:
 * halo exchange after the rasterization, every node's kinetic energy counted by the lowest rank that holds mass on it, the ranks'
 * shares summed by mpmhip_tiled_reduce (MPMHIP_WIRE_LOCAL: mpmhip_calculate_energy_group). */
int mpmhip_calculate_energy(mpmhip_ctx *ctx, double *kinetic, double *potential);

/* replaces general_action "delete_particles_inside_level_set" (src/mpm.cpp:962-974): deletes every particle whose
 * level-set value at its position is negative (the level set last given to mpmhip_set_levelset[_shapes | _sdf]);
 * *deleted = how many.  The next sort rebuilds the keys.  Synchronises. */
int mpmhip_delete_particles_inside_level_set(mpmhip_ctx *ctx, int64_t *deleted);

/* frame output — replaces MPM<dim>::write_bgeo / write_partio (src/mpm.h:333-337, src/visualize.cpp:17-100; called
 * by visualize(), src/visualize.cpp:156-164) including the Partio encoder behind it (external/partio/src/io/BGEO.cpp:
 * 57-194, Houdini .bgeo version 5, big-endian).  Byte-identical to the reference's file for the same particle state:
 * attributes position, type, index, limit[3], v and — verbose (config "verbose_bgeo") — m, boundary_normal[3], debug[3],
 * states, boundary_distance, near_boundary, apic_frobenius_norm; particles in ascending id.  The rows are gathered,
 * interleaved and byte-swapped on the device; the host adds header and trailer.  Fields this library does not track
 * (no rigid bodies, no async stepping) hold the reference's constructor values (src/particles.h:92-99).
 * mpmhip_bgeo_size: bytes of the file for the current state.  mpmhip_bgeo_encode: the file image into caller memory
 * (*written = bytes; MPMHIP_ECAPACITY if `capacity` is too small).  mpmhip_write_bgeo: the same to `path` (plain
 * .bgeo as the reference writes; a ".gz" suffix is MPMHIP_ENOTIMPL).  On a tiled ctx these three encode its own rank's particles; the one file
 * of the whole job comes from the calls under "the frame of a tiled job" below.  All three synchronise. */
int mpmhip_bgeo_size(mpmhip_ctx *ctx, int32_t verbose, size_t *bytes);
int mpmhip_bgeo_encode(mpmhip_ctx *ctx, int32_t verbose, void *dst, size_t capacity, size_t *written);
int mpmhip_write_bgeo(mpmhip_ctx *ctx, const char *path, int32_t verbose);

/* the frame of a tiled job — MPM<dim>::write_partio (src/visualize.cpp:17-100) writes ONE file for all particles: one header, the
 * rows in ascending creation id, one trailer whose point numbers are uint16 up to 65536 rows and int32 above.  The ranks of a tiled
 * job each hold some of the ids, in any slot order, so the row number of a particle is the rank of its id among all live ids of
 * the job.  It is computed on the device: top = 1 + the largest live id, a bitmap of ceil(top / 32) words in which every ctx sets
 * the bits of its ids, the exclusive prefix of the words' popcounts, and row(id) = prefix[id / 32] + popcount of the lower bits
 * of its word.  No id array reaches the host.
 *
 * mpmhip_bgeo_size_group / mpmhip_bgeo_encode_group (src/visualize.cpp:17-100): the n_ctx ctx of ONE process on ONE device (the
 * convention of mpmhip_tiled_advance_group), which need not be connected as a job nor hold a set partition.  The image is, byte
 * for byte, the file one ctx holding the same records would encode; n_ctx = 1 gives that ctx's file.  MPMHIP_EINVAL: ctx on
 * different devices, ctx of different res, a ctx with rigid bodies or a resident asynchronous stepper, a creation id held by two
 * slots (the message, on ctxs[0], names it; nothing has been written to dst).  MPMHIP_ECAPACITY as mpmhip_bgeo_encode.  Both
 * synchronise every ctx. */
int mpmhip_bgeo_size_group(mpmhip_ctx *const *ctxs, int32_t n_ctx, int32_t verbose, size_t *bytes);
int mpmhip_bgeo_encode_group(mpmhip_ctx *const *ctxs, int32_t n_ctx, int32_t verbose, void *dst, size_t capacity, size_t *written);
/* the same for a rank per process (src/visualize.cpp:17-100), in three steps without a collective inside; the caller reduces
 * between them and places the rows:
 *   mpmhip_live_id_top       1 + the largest live creation id of this ctx (0: no particle), or a negative error.  The id counter is
 *                            no substitute: after mpmhip_upload(MPMHIP_F_ID) it may lie below the ctx's largest id (mpmhip_set_next_id).
 *                            The job's top is the maximum over the ranks.
 *   mpmhip_id_bitmap         this ctx's bitmap for the job's `top` into words_host[ceil(top / 32)], *live = its live particles.  An id
 *                            at or beyond top, or held twice on this ctx: MPMHIP_EINVAL.  The job's bitmap is the OR over the ranks
 *                            (the bits of a valid job are disjoint: the popcount of the OR equals the sum of the `live`).
 *   mpmhip_bgeo_rows_ranked  this ctx's rows (12 words each, 23 verbose) in ascending id into rows_host, and into row_index_host for
 *                            each its row number in the job's file, given the job's bitmap; *written = the rows.
 *                            MPMHIP_ECAPACITY when capacity_rows is below the ctx's live particles, MPMHIP_EINVAL when the ctx
 *                            holds an id the job's bitmap lacks.
 * All three synchronise. */
int64_t mpmhip_live_id_top(mpmhip_ctx *ctx);
int mpmhip_id_bitmap(mpmhip_ctx *ctx, int64_t top, uint32_t *words_host, int64_t *live);
int mpmhip_bgeo_rows_ranked(mpmhip_ctx *ctx, int32_t verbose, int64_t top, const uint32_t *union_words_host, void *rows_host,
                            uint32_t *row_index_host, int64_t capacity_rows, int64_t *written);
/* what stands before and behind n rows of a frame (src/visualize.cpp:17-100 through BGEO.cpp:57-194): the header and attribute
 * tables, and the primitive attribute, the point numbers and the file's end — the bytes mpmhip_bgeo_encode writes there, from the
 * same functions.  Host only: no ctx, no device.  head = tail = NULL: the two sizes alone.  MPMHIP_ECAPACITY when a buffer is
 * too small (message: mpmhip_last_error(NULL)). */
int mpmhip_bgeo_envelope(uint32_t n, int32_t verbose, void *head, size_t head_cap, size_t *head_bytes, void *tail, size_t tail_cap,
                         size_t *tail_bytes);

/* profiling — replaces TC_PROFILE / TC_PROFILE_TPE scoped timers (src/mpm.cpp:464-572).
 * level 0: off.  level 1: hipEvents bracket each phase of every substep on the ctx stream (six records per
 * substep; each record costs ~5 us of idle GPU).  level 2 / 3: only k_g2p / only k_p2g is bracketed (two records),
 * for timing the dominant kernel inside a throughput measurement.  level 4: the three parts of a tiled substep are
 * bracketed — substep_begin (sort, boundary P2G, halo pack) -> "p2g", substep_interior -> "grid", substep_end -> "g2p" —
 * with no record INSIDE a part: what one rank computes per substep when nothing is being profiled.
 * mpmhip_profile writes a JSON object: {"substeps":N,"particles":n,"active_blocks":a,"rank_mode":m,
 *   "phases":{"sort":ms,"p2g":ms,"exchange":ms,"grid":ms,"g2p":ms}}  (totals since the last reset; rank_mode = the
 *   in-cell ranking path the next sort will take: 0 per-run atomics, 1 per-batch LDS hash; "exchange" is
 *   the gap between substep_begin and substep_end of a tiled run; phases not bracketed at the level stay 0). */
int mpmhip_set_profiling(mpmhip_ctx *ctx, int32_t level);
/* levels 2 / 3: bracket the kernel only in every `every`-th substep (default 1 = all).  "substeps" of mpmhip_profile then
 * counts the bracketed ones, so phase time / substeps stays the mean launch duration — with a quarter of the ~5 us event
 * bubbles inside a throughput measurement at every = 4. */
int mpmhip_set_profile_sampling(mpmhip_ctx *ctx, int32_t every);
int mpmhip_profile(mpmhip_ctx *ctx, char *json, size_t cap);
int mpmhip_profile_reset(mpmhip_ctx *ctx);

/* ---------------------------------------------------------------------------------------------------------
 * Multi-GPU tiling (one ctx per GPU, each over the WHOLE grid index space but holding only the particles of its
 * brick).  The reference has no multi-process code; this is the sharding SURVEY §8(e) derives from the stencil
 * support (base..base+2 nodes, src/kernel.h:119-121, src/transfer.cpp:59-63).  The library never communicates:
 * the caller moves the device buffers named here with any transport (RCCL, MPI, hipMemcpyPeer).
 *
 *   partition : `dims[a]` bricks per axis with cell cut planes `cuts[a][0..dims[a]]` (cuts[a][0] = 0,
 *               cuts[a][dims[a]] >= res[a]); rank of brick (px,py,pz) = (px*dims[1] + py)*dims[2] + pz.
 *               A particle belongs to the brick containing its base cell int(x/dx - 0.5) (src/kernel.h:119-121);
 *               it may sit up to `margin` cells outside its rank's brick between two migrations.
 *   halo      : node boxes shared with other ranks.  After P2G, mpmhip_halo_pack() writes this rank's partial
 *               (m v, m) sums on every box to `send`; the caller exchanges send<->recv with rank `peer`;
 *               grid_update then forms every node total as the sum over contributors IN RANK ORDER (own partial
 *               at its rank position), so all holders of a node compute bit-identical values.
 *   migration : mpmhip_leaver_counts -> per-destination counts (synchronises); mpmhip_export_leavers packs the
 *               MPMHIP_MIGRATE_FLOATS-float records grouped by destination rank (ascending) into a device buffer
 *               and removes them locally; mpmhip_import_particles appends received records.  On a ctx whose apic_b rows are
 *               behind the affine matrices (discard_apic_b, after a substep) the arrivals' rows are stored as zero: a stale row
 *               says nothing, and its place in the buffer depends on the order of arrival.
 */
#define MPMHIP_MAX_PARTS 16       /* bricks per axis */
#define MPMHIP_MAX_HALO_BOXES 64
#define MPMHIP_MIGRATE_FLOATS 44  /* RecG(16) + RecP(16) + apic_b(12) : 176 bytes per migrating particle */

typedef struct {
  int32_t lo[3], hi[3]; /* node box [lo, hi) in global node coordinates */
  int32_t peer;         /* rank of the other contributor */
  int32_t reserved;
  void *send;           /* device float4[volume], x-major (z fastest): written by mpmhip_halo_pack */
  const void *recv;     /* device float4[volume]: the peer's partial sums, read by grid_update */
} mpmhip_halo_box;

int mpmhip_set_partition(mpmhip_ctx *ctx, int32_t rank, const int32_t dims[3], const int32_t *cuts_x,
                         const int32_t *cuts_y, const int32_t *cuts_z, int32_t margin);
/* boxes must be sorted by ascending peer; n = 0 disables the halo */
int mpmhip_set_halo(mpmhip_ctx *ctx, int32_t n, const mpmhip_halo_box *boxes);
int mpmhip_halo_pack(mpmhip_ctx *ctx);
/* tiled substep = substep_begin (sort, P2G, halo_pack) ; caller exchanges ; substep_end (grid, G2P) */
int mpmhip_substep_begin(mpmhip_ctx *ctx);
int mpmhip_substep_end(mpmhip_ctx *ctx);
/* exchange/compute overlap: with set_overlap(1), substep_begin only rasterizes the blocks that touch a halo box (then
 * packs); the caller starts the exchange asynchronously and calls substep_interior (P2G, grid and G2P of everything
 * that cannot touch a halo node) while it is on the wire, waits for it, and calls substep_end (the boundary part).
 * substep_interior is a no-op when the overlap is off; substep_end runs it if the caller skipped it. */
int mpmhip_set_overlap(mpmhip_ctx *ctx, int32_t enabled);
/* The per-substep loop of a tiled rank in native code: for each of n substeps
 *     substep_begin;  exchange(user, MPMHIP_EXCHANGE_START);  substep_interior;  exchange(user, MPMHIP_EXCHANGE_WAIT);  substep_end
 * — the caller supplies only the transport (START: launch the all-to-all of the halo boxes behind the work enqueued so far,
 * e.g. on a side stream; WAIT: make the ctx's stream wait for it).  A non-zero return of the callback ends the loop and is
 * returned (negative values are taken as they are, positive ones as MPMHIP_EINVAL).  `until_migration` > 0 stops after that
 * many substeps even if n is larger (the caller runs its migration and calls again); returns the number of substeps run. */
enum { MPMHIP_EXCHANGE_START = 0, MPMHIP_EXCHANGE_WAIT = 1 };
typedef int32_t (*mpmhip_exchange_fn)(void *user, int32_t phase);
int64_t mpmhip_tiled_run(mpmhip_ctx *ctx, int64_t n, int64_t until_migration, mpmhip_exchange_fn exchange, void *user);
int mpmhip_substep_interior(mpmhip_ctx *ctx);
/* counts[world]: live particles whose base cell now lies in another rank's brick.  Also raises MPMHIP_ECAPACITY
 * (sticky) if a particle is more than `margin` cells outside this rank's brick. */
int mpmhip_leaver_counts(mpmhip_ctx *ctx, int32_t world, int64_t *counts);
/* the same pass also yields the bounding box [lo, hi) of the base cells of all live particles (lo > hi: none) and
 * the speed of the fastest one in cells per substep (max |v|_inf dt / dx; may be NULL), so one synchronisation per
 * migration serves the counts, the halo-box clipping and the schedule of the next migration (a particle needs
 * margin / speed substeps to cross the margin) */
int mpmhip_migration_scan(mpmhip_ctx *ctx, int32_t world, int64_t *counts, int32_t lo[3], int32_t hi[3],
                          float *max_cells_per_substep);
/* packs every leaver (n_total = sum of the counts just returned) into dev_records, grouped by destination */
int mpmhip_export_leavers(mpmhip_ctx *ctx, int32_t world, const int64_t *counts, void *dev_records);
int mpmhip_import_particles(mpmhip_ctx *ctx, int64_t n, const void *dev_records);
/* ---- Multi-GPU tiling, the native data plane (csrc/tiled_api.h).  With the calls above the CALLER plans the halo boxes, owns
 * the buffers and moves them (the Python / gloo path of taichi_mpm_amd/tiled.py, kept for the CPU tests).  With the calls below
 * the LIBRARY does all of it: it derives the halo boxes from the partition (box R∩S = intersection of the two ranks' node
 * boxes, clipped to the occupied part of the grid — the same on both sides), owns send / receive buffers sized for the worst
 * case (no re-allocation when the boxes follow the particles), runs the per-substep loop, the halo exchange, the migration
 * (scan, table all-gather, record exchange, import), the re-planning and the migration schedule — nothing returns to the
 * host language between mpmhip_tiled_advance's first and last substep.  SURVEY section 8(e) collectives (1)-(3).
 * Wires:
 *   MPMHIP_WIRE_RCCL   ncclGroupStart / per-neighbour ncclSend + ncclRecv / ncclGroupEnd on a side stream of the ctx (fenced to
 *                      the ctx stream by events; on the ctx stream itself when the overlap split is off), ncclAllGather for
 *                      the migration table, grouped ncclSend / ncclRecv for the records.  librccl is dlopen'ed (env
 *                      MPMHIP_RCCL_LIB names it): libmpmhip does not link it.  The caller only carries the ncclUniqueId from
 *                      rank 0 to the other ranks (mpmhip_comm_unique_id / mpmhip_comm_init).
 *   MPMHIP_WIRE_IPC    no collective at all: every rank maps every other rank's receive arena (hipIpcGetMemHandle /
 *                      hipIpcOpenMemHandle); k_halo_pack writes each box straight into the peer's receive buffer (double
 *                      buffered by substep parity) and publishes the substep's epoch in the peer's flag word; the peer's
 *                      stream polls that word (a one-wave kernel with a bounded wait: sticky error instead of a hang) before
 *                      its grid kernel reads the box.  Migration rows and records travel the same way.  The 64-byte handles
 *                      are all-gathered by the caller (mpmhip_tiled_ipc_handle / _connect), or through the ctx's RCCL
 *                      communicator when it has one (_connect with handles == NULL).
 *   MPMHIP_WIRE_LOCAL  the IPC wire between ctx of ONE process (virtual ranks on one device: tests, bench.py --virtual):
 *                      plain pointers instead of mapped ones, driven by mpmhip_tiled_advance_group.
 *   MPMHIP_WIRE_LOCAL_RCCL  a LOCAL job whose HALO BOXES travel through RCCL all the same — the one-GPU pre-flight of the
 *                      MPMHIP_WIRE_RCCL exchange: every ctx of the job has its own ONE-rank communicator
 *                      (mpmhip_comm_init(ctx, id, 0, 1) before mpmhip_tiled_setup), every box is an ncclSend to the rank itself
 *                      whose ncclRecv is aimed at the box's place in the PEER ctx's receive buffer: the same ncclGroupStart / Send
 *                      + Recv per box / ncclGroupEnd, on the same side stream behind the same two event fences when the substep is
 *                      split, with the one receive buffer of that wire — under real RCCL kernels next to the substep's own.
 *                      Migration rows, records and reductions travel as on MPMHIP_WIRE_LOCAL.  The ranks must share one stream.
 * A ctx with a native plan refuses mpmhip_set_halo / mpmhip_tiled_run with a callback, and vice versa. */
enum { MPMHIP_WIRE_RCCL = 1, MPMHIP_WIRE_IPC = 2, MPMHIP_WIRE_LOCAL = 3, MPMHIP_WIRE_LOCAL_RCCL = 4 };
#define MPMHIP_COMM_ID_BYTES 128   /* sizeof(ncclUniqueId) */
#define MPMHIP_IPC_HANDLE_BYTES 64 /* sizeof(hipIpcMemHandle_t) */
typedef struct {
  int32_t rank, world;
  int32_t dims[3];             /* bricks per axis; world = dims[0] dims[1] dims[2] */
  int32_t margin;              /* cells a particle may sit outside its brick between two migrations */
  int32_t clip_lo[3], clip_hi[3]; /* node box the halo boxes are clipped to (occupied part of the grid + slack); the library
                                  * re-wraps it around the particles at every migration (slack max(8, 4 margin + 4) cells) AND, from a
                                  * planning scan in front of the job's first substep on, cuts every rank's node box to that rank's OWN
                                  * occupancy (every rank's particle bounds travel in the migration table): ranks whose particles cannot
                                  * meet before the next check exchange nothing */
  int32_t migrate_interval;    /* > 0: a migration every that many substeps (<= margin); 0: the CFL interval (= margin)
                                  * stretched by the measured top speed, up to migrate_cap substeps */
  int32_t migrate_cap;         /* 0: 64 */
  int32_t wire;                /* MPMHIP_WIRE_* */
  int32_t overlap;             /* boundary / interior split of the substep (mpmhip_set_overlap) */
  int64_t inbox_records;       /* capacity of this rank's migration inbox in records; 0: max(65536, capacity / 8).  Every rank learns
                                * every inbox's capacity with the migration table and all refuse together when one would overflow */
} mpmhip_tiled_config;
/* rank 0: a fresh ncclUniqueId; every rank: ncclCommInitRank on the ctx's device (collective over the ranks) */
int mpmhip_comm_unique_id(uint8_t id[MPMHIP_COMM_ID_BYTES]);
int mpmhip_comm_init(mpmhip_ctx *ctx, const uint8_t id[MPMHIP_COMM_ID_BYTES], int32_t rank, int32_t world);
int mpmhip_comm_destroy(mpmhip_ctx *ctx);
/* loopback check of the binding: world-sized all-gather + a grouped send / receive ring (to self when world == 1) on device
 * buffers, verified on the host; collective over the ranks */
int mpmhip_comm_selftest(mpmhip_ctx *ctx);
/* partition + plan + buffers; replaces mpmhip_set_partition / mpmhip_set_halo.  Synchronises.  A ctx of an IPC job set up again
 * on the IPC wire with an unchanged arena size keeps its arena (zeroed) and its handle; mpmhip_tiled_ipc_connect then keeps
 * the mappings of the peers' arenas whose handles are unchanged. */
int mpmhip_tiled_setup(mpmhip_ctx *ctx, const mpmhip_tiled_config *cfg, const int32_t *cuts_x, const int32_t *cuts_y,
                       const int32_t *cuts_z);
int mpmhip_tiled_ipc_handle(mpmhip_ctx *ctx, uint8_t handle[MPMHIP_IPC_HANDLE_BYTES]);
int mpmhip_tiled_ipc_connect(mpmhip_ctx *ctx, const uint8_t *handles /* [world][64], own entry ignored; NULL: via RCCL */);
int mpmhip_tiled_connect_local(mpmhip_ctx *const *ctxs, int32_t n /* = world, ctxs[r] = rank r */);
/* n substeps of this rank, migrations included when they are due (collective over the ranks: every rank calls it with the
 * same n).  Returns n or a negative error code. */
int64_t mpmhip_tiled_advance(mpmhip_ctx *ctx, int64_t n);
/* the same for all ranks of a MPMHIP_WIRE_LOCAL job: per substep begin of every rank, [interior of every rank,] end of every rank */
int64_t mpmhip_tiled_advance_group(mpmhip_ctx *const *ctxs, int32_t n_ctx, int64_t n);
/* SURVEY section 8(e) collective (3) — a few scalars over all ranks of a tiled job, inside the library: in-place all-reduce of n <=
 * MPMHIP_REDUCE_MAX_VALUES doubles (MPMHIP_WIRE_RCCL: ncclAllReduce on a device row; MPMHIP_WIRE_IPC: every rank writes its row into
 * every rank's table, publishes an epoch, waits for the world's and reduces the table in rank order — the bit-identical result on
 * every rank).  Collective: every rank calls it with the same n and op.  Synchronises. */
enum { MPMHIP_REDUCE_SUM = 0, MPMHIP_REDUCE_MAX = 1, MPMHIP_REDUCE_MIN = 2 };
#define MPMHIP_REDUCE_MAX_VALUES 16
int mpmhip_tiled_reduce(mpmhip_ctx *ctx, double *values, int32_t n, int32_t op);
/* the same for all ranks of a MPMHIP_WIRE_LOCAL job: values = [n_ctx][n], every row receives the result */
int mpmhip_tiled_reduce_group(mpmhip_ctx *const *ctxs, int32_t n_ctx, double *values, int32_t n, int32_t op);
/* MPM<dim>::calculate_energy (src/mpm.cpp:1078-1110) of the WHOLE job of a MPMHIP_WIRE_LOCAL group (on the other wires
 * mpmhip_calculate_energy of a tiled ctx is itself the collective): sort + rasterize + halo exchange on every rank, grid kinetic
 * energy with every node counted by the lowest rank that holds mass on it, the particles' potential energy, summed over the ranks */
int mpmhip_calculate_energy_group(mpmhip_ctx *const *ctxs, int32_t n_ctx, double *kinetic, double *potential);
/* out = {live particles, active blocks, sticky error word (OR over the ranks: bit 0 block table full, 1 a particle beyond the margin,
 * 2 distance-field pages, 4 a peer's epoch timed out), particles migrated so far} of the whole job; collective; synchronises */
int mpmhip_tiled_totals(mpmhip_ctx *ctx, int64_t out[4]);
int mpmhip_tiled_totals_group(mpmhip_ctx *const *ctxs, int32_t n_ctx, int64_t out[4]);
/* out = {substeps run, substep of the next migration, particles migrated out so far, migrations, re-plans, halo boxes,
 *        halo nodes (float4) per exchange, wire} */
int mpmhip_tiled_state(mpmhip_ctx *ctx, int64_t out[8]);
/* the current plan: boxes sorted by peer (send / recv = the library's buffers); returns the number of boxes */
int32_t mpmhip_tiled_plan(mpmhip_ctx *ctx, int32_t capacity, mpmhip_halo_box *out);
/* Re-cutting a running job — the bricks follow the live particles (3D; the 2D solver has no tiling).
 *
 * mpmhip_live_histogram: what the new partition is cut from, on any ctx, tiled or not: the outputs of mpmhip_seed_histogram, counted
 * over the particles the ctx HOLDS.  hist_a[i] = the live particles whose base cell has index i along axis a (res[a] entries each, NULL
 * allowed), *total their number, cell_bounds = lo3, hi3 (exclusive) of those bins (all 0 when *total == 0).
 *   live       creation id >= 0, position finite and >= 0.5 cells on every axis: the set the migration can place.
 *   bin        the base cell b[k] = (int)fl(fl(x[k] * fl(1 / dx)) - 0.5f), nothing contracted — the expression of the brick seeding
 *              above, which tiled.base_cells restates to the bit —, clamped to [0, res[a] - 1].
 * Integer counts: exact, whatever the order.  No particle state is written, no counter moves.  Synchronises.  MPMHIP_EINVAL inside a
 * substep.  The ranks of a job add their histograms and join their bounds; mpmhip_balanced_cuts turns the sums into cuts.
 *
 * mpmhip_balanced_cuts: the cut planes [0, c1, .., res] of one axis for `parts` bricks from that axis's histogram (no ctx: host
 * arithmetic, csrc/tiled_plan.h).  cut k lies behind the first cell whose cumulative count reaches total k / parts; a cut at the edge
 * of an empty stretch moves to its middle; every brick keeps at least one cell; an empty histogram gives the even split.  What
 * tiled.balanced_cuts computes, cut for cut.  MPMHIP_EINVAL: parts outside [1, min(MPMHIP_MAX_PARTS, res)], a negative count.
 *
 * mpmhip_tiled_redistribute[_group]: between two advances of a connected job, typically right after mpmhip_tiled_setup was repeated
 * with new cuts: EVERY live particle moves to the rank that owns its base cell (the expression above) under the partition now in
 * force.  Collective, like mpmhip_tiled_advance.  It is a migration — scan, table exchange, pack, the wire's record transfer (RCCL:
 * grouped ncclSend / ncclRecv; IPC: peer writes + epochs; LOCAL: plain pointers), import, every wait bounded — with three differences:
 *   margin     suspended: a particle any distance from this rank's brick is legal.  The sticky bit 1 of the error word is not raised,
 *              and an error word already set is left as it is (only a peer's epoch that timed out ends the call).
 *   rounds     a destination admits its sources in ascending rank order until its inbox is full (what it offers in a round: the
 *              inbox of the set-up, or its free slots if they are fewer); a leaver beyond the quota stays for the next round; the
 *              rounds repeat until a scan finds no leaver.  The inbox the job was set up with is enough, whatever its size.  A rank
 *              whose free slots do not hold an inbox drops its dead slots (a sort + compaction) before it makes its offer.
 *   capacity   checked before anything moves: from the first table every rank knows every rank's live count after the move, live -
 *              out + in.  If one exceeds its capacity EVERY rank returns MPMHIP_ECAPACITY, nothing has moved, the message names the
 *              first such rank and info[3] = the capacity THIS rank needs (0 where it fits): mpmhip_reserve there and repeat the
 *              call on every rank — the convention of mpmhip_seed_particles_brick.
 * Afterwards every live particle sits on its owner, records are bit for bit what they were (ids included; a rank's slot order is
 * not), and the plan is stale exactly as behind a brick seeding call: the next advance begins with the planning scan, which cuts the
 * halo boxes around the new occupancy; until then the clip box is widened to the joined bounds of all particles.  Should the
 * migration's own (contractible) base-cell expression round differently for a particle at an exact cell face, that particle simply
 * migrates at the next check.  A one-rank job: nothing to do.  MPMHIP_EINVAL: no set-up, not connected, inside a substep, the group
 * form on another wire than MPMHIP_WIRE_LOCAL[_RCCL] (and the single form on a local job of more than one rank). */
int mpmhip_live_histogram(mpmhip_ctx *ctx, int64_t *hist_x, int64_t *hist_y, int64_t *hist_z /* res[a] bins each, NULL allowed */,
                          int64_t *total, int32_t cell_bounds[6] /* lo3, hi3 (exclusive); all 0 when total == 0 */);
int mpmhip_balanced_cuts(int32_t res, int32_t parts, const int64_t *hist, int32_t *cuts /* parts + 1 */);
int mpmhip_tiled_redistribute(mpmhip_ctx *ctx, int64_t info[4]);                             /* RCCL / IPC wire: collective */
int mpmhip_tiled_redistribute_group(mpmhip_ctx *const *ctxs, int32_t n_ctx, int64_t *info);  /* LOCAL / LOCAL_RCCL: info[n_ctx][4] */
/* info = {records sent by this rank, records received, rounds, capacity this rank needs (set on MPMHIP_ECAPACITY, else 0)} */
/* cell bounding box [lo, hi) of the active 4^3-cell blocks of the last sort (lo > hi when there are none);
 * synchronises.  Lets the caller clip the halo boxes to the occupied part of the grid. */
int mpmhip_active_bounds(mpmhip_ctx *ctx, int32_t lo[3], int32_t hi[3]);
int64_t mpmhip_num_slots(mpmhip_ctx *ctx);       /* slots in use (live + dead) — capacity pressure */
int mpmhip_request_compaction(mpmhip_ctx *ctx);  /* physical reorder + drop of dead slots at the next sort */
/* Grows the particle capacity of a live ctx IN PLACE to at least max_particles (never shrinks): the record arrays are
 * re-allocated and copied, an auto-sized block table (max_blocks = 0 at creation) grows with them.  Everything else
 * stays — groups, level set, clocks, stream, rigid bodies and joints, the async block table, partition and halo boxes —
 * so a scene that keeps adding particles (the reference's ParticleAllocator pool grows on demand,
 * src/particle_allocator.h:36-60) needs no max_particles up front, with or without bodies.  Synchronises; the next
 * substep sorts from scratch.  Not between substep_begin and substep_end. */
int mpmhip_reserve(mpmhip_ctx *ctx, int64_t max_particles);
int64_t mpmhip_capacity(mpmhip_ctx *ctx);

/* ---- AsyncMPM, first half — replaces AsyncMPM<dim>::update_dt_limits (src/async/async_mpm.cpp:90-164) and the limit
 * attributes AsyncMPM<dim>::visualize writes (src/async/async_visualize.cpp:17-26).  A scheduler block is the reference's
 * SPGrid block of 4 x 4 x 8 nodes holding the particle's base node.  Per block: strength_dt_limit =
 * int(strength_dt_mul * min get_allowed_dt(dx) / unit_delta_t) (per-material sound-speed bound, src/particles.cpp),
 * cfl_dt_limit = int(cfl_dt_mul * dx / unit_delta_t / sqrt(max |v|^2)), continuous_dt_limit = the power of two that
 * tracks min(cfl, strength, max_units) under the reference's halving / doubling rule.  The per-block reduction runs on
 * the device, the block state machine on the host.  After mpmhip_async_update_dt_limits the `limit` attribute of
 * mpmhip_write_bgeo carries (continuous, strength, cfl) of each particle's block instead of (1, 1, 1).
 * The stepping itself (AsyncMPM<dim>::advance / step) is the second half, mpmhip_async_begin / _step below. */
typedef struct {
  float unit_delta_t;     /* config "unit_delta_t", default 1e-6 (src/async/async_mpm.cpp:24) */
  int64_t max_units;      /* "max_units", default 8192 */
  float cfl_dt_mul;       /* "cfl_dt_mul", default 1 */
  float strength_dt_mul;  /* "strength_dt_mul", default 1 */
  int32_t left_boundary;  /* "left_boundary", default 0: the scheduler blocks whose corner lies in x <= 0.2 of the domain follow
                           * the SMALLEST step in use (src/async/async_mpm.cpp:43-53, 155-163) */
} mpmhip_async_config;
int mpmhip_async_enable(mpmhip_ctx *ctx, const mpmhip_async_config *cfg);
int mpmhip_async_update_dt_limits(mpmhip_ctx *ctx);
int64_t mpmhip_async_blocks(mpmhip_ctx *ctx, int64_t capacity, int32_t *corner_node /* [n][3] */, int64_t *strength,
                            int64_t *cfl, int64_t *continuous, int64_t *count, int64_t min_max_delta_t_int[2]);
int mpmhip_async_set_time_int(mpmhip_ctx *ctx, int64_t current_t_int);
/* dense block table: nb[3] = blocks per axis, block b = (bx nb[1] + by) nb[2] + bz; returns the number of blocks (with
 * capacity < that number nothing is written: size query) */
int64_t mpmhip_async_table(mpmhip_ctx *ctx, int32_t nb[3], int64_t capacity, int64_t *strength, int64_t *cfl,
                           int64_t *continuous, int64_t *count);
/* ---- AsyncMPM, second half — replaces AsyncMPM<dim> itself (TC_IMPLEMENTATION(Simulation3D, AsyncMPM3D, "async_mpm"),
 * src/async/async_mpm.cpp:423-427): initialize (:13-55), add_particles (:57-75), update_dt_limits (:90-253), advance
 * (:255-373), step (:380-421), and the particle list of visualize (src/async/async_visualize.cpp:86-96).
 * The particle pools and backup pools of every scheduler block live in a device-resident store of containers; an advance
 * gathers its working set (first copy of an id wins: smaller-step neighbours' pools, then the pools of the level's blocks,
 * then larger-step neighbours' backups, each in the reference's block order) into the ctx's records with index kernels,
 * runs ONE ordinary substep with dt = unit_delta_t * limit, and files the results back.  Block tables and the level walk
 * are host code as in the reference; no particle data crosses the host boundary during stepping.  The ctx must keep apic_b
 * (discard_apic_b = 0) and hold neither rigid bodies nor a partition.
 *   begin            after mpmhip_create; takes the AsyncMPM config keys
 *   pool_particles   after every mpmhip_add_particles: the new particles move from the ctx's records to their blocks' pools
 *   step(dt)         AsyncMPM::step; dt < 0 (the synchronous single substep of the base class) is refused
 *   load_pools       every container of every particle pool becomes the ctx's records (with its pool block's limits for
 *                    the frame's `limit` attribute), so that mpmhip_write_bgeo / download / calculate_energy / snapshots
 *                    see the whole state; the next step() ignores the records (the pools are the state)
 *   state            out = {current_t_int, update_counter, min_delta_t_int, max_delta_t_int, live containers, store size
 *                    incl. freed containers, compactions so far, step_counter}
 *   block_times      particle_t / backup_t / local_min_dt_limit of every block of the dense table (size query as above)
 *   download_pools   rows of 27 floats {x3, v3, F9, apic_b9, aux, gid bits, id bits} + the pool block of every container
 *                    (an id can occur in more than one pool, as in the reference); rows == NULL: the count */
int mpmhip_async_begin(mpmhip_ctx *ctx, const mpmhip_async_config *cfg);
int mpmhip_async_pool_particles(mpmhip_ctx *ctx);
int mpmhip_async_step(mpmhip_ctx *ctx, float dt);
int mpmhip_async_load_pools(mpmhip_ctx *ctx);
int mpmhip_async_state(mpmhip_ctx *ctx, int64_t out[8]);
double mpmhip_async_current_time(const mpmhip_ctx *ctx);
int64_t mpmhip_async_block_times(mpmhip_ctx *ctx, int64_t capacity, int64_t *particle_t, int64_t *backup_t, int64_t *local_min);
int64_t mpmhip_async_download_pools(mpmhip_ctx *ctx, int64_t capacity, float *rows, int32_t *block);
/* test helper: which form of the four kernels that place containers ran last in this session — out = {gather (the working set of an
 * advance), file (the appends behind the store's end), load (load_pools), export (download_pools)}: 0 = by order of arrival, 1 = the
 * ordered form of the deterministic mode (csrc/k_async.h), -1 = not launched since mpmhip_async_begin.  Nothing is launched.
 * With the mode on a resident stepper is a function of its configuration, its level set and the sequence of calls it receives:
 * filed particles go behind the store's end in ascending working-set slot, working sets, views and exported rows come in ascending
 * store position, so download_pools' raw rows, frames, snapshot blobs and counters are byte-identical between runs, whatever the
 * launch sizes.  The mode may be switched between steps (mpmhip_set_deterministic): the next launch uses the new form, the order
 * the store had until then stays.  TEST KNOB: env MPMHIP_ASYNC_WGS=n (read by mpmhip_async_begin / mpmhip2d_async_begin; results
 * valid) caps the workgroups of every asynchronous launch, so that a small scene carries a scan across several chunks per workgroup. */
int mpmhip_async_forms(mpmhip_ctx *ctx, int32_t out[4]);
/* host wall time spent so far, ms: {update_dt_limits, of which the neighbour lists, advance, of which the substep (meaningful
 * with sync != 0: the stream is then synchronised behind every substep), store compaction, number of advances} */
int mpmhip_async_profile(mpmhip_ctx *ctx, int32_t sync, double out[6]);
/* snapshots of the asynchronous stepper (the reference serialises every pool and the block table, src/async/async_mpm.h:120-172):
 * groups, block table, clocks and every live container of the store.  Loaded into a ctx of the same grid on which
 * mpmhip_async_begin has run with the same unit_delta_t; level set and configuration come from the scene again. */
int64_t mpmhip_async_snapshot_size(mpmhip_ctx *ctx);
int mpmhip_async_snapshot_save(mpmhip_ctx *ctx, void *dst, size_t capacity);
int mpmhip_async_snapshot_load(mpmhip_ctx *ctx, const void *src, size_t size);
/* bytes of particle data copied between host and device by this ctx so far (add_particles, download, upload, snapshots,
 * download_pools): a stepping call must leave it unchanged */
int64_t mpmhip_host_particle_bytes(const mpmhip_ctx *ctx);
/* plumbing of a host-driven stepper (the round-2 asynchronous stepper used these): drop all particles but keep groups /
 * level set / config; change base_delta_t (the P2G matrices are rebuilt) and the clock — AsyncMPM<dim>::advance / step set
 * both before every MPM<dim>::substep (src/async/async_mpm.cpp:405-408) */
int mpmhip_clear_particles(mpmhip_ctx *ctx);
int mpmhip_set_dt(mpmhip_ctx *ctx, float base_delta_t);
int mpmhip_set_time(mpmhip_ctx *ctx, double current_t);
/* the three clocks of a ctx — current_t, the request_t accumulator of step() (src/mpm.cpp:428-439), the substep counter
 * that phases the physical reorder (src/mpm.cpp:811-813): read / restored by a host layer that re-creates a ctx */
int mpmhip_get_clock(const mpmhip_ctx *ctx, double *current_t, double *request_t, int64_t *substeps);
int mpmhip_set_clock(mpmhip_ctx *ctx, double current_t, double request_t, int64_t substeps);
/* MPMParticle::get_allowed_dt(dx) of n particle states of one material (src/particles.cpp:136-155,254-278,480-490,...) */
int mpmhip_debug_allowed_dt(mpmhip_ctx *ctx, int32_t material, const float params[MPMHIP_NPARAM], int64_t n, const float *F,
                            const float *aux, const float *v, float dx, float *out);

/* ---- MPM<2>: the reference's 2D simulation — replaces the object tc_core.create_simulation2('mpm') returns
 * (TC_IMPLEMENTATION(Simulation2D, MPM2D, "mpm"), src/mpm.cpp:983-986).  MPM<2> runs the GENERIC transfer path
 * (rasterize_optimized = rasterize, resample_optimized = resample: src/transfer.cpp:280-283,697-700; bodies :193-278,
 * :585-687, including the position clamp of :668-670) with all eight particle types in their dim = 2 form.  Its own small
 * object: SoA particles, dense (res+1)^2 grid (2D scenes are the reference's small cases).  Matrices row-major float[4].
 * Level-set shapes are mpmhip_shape read in the plane (z ignored); n1 >= 0 adds the key frame at t1 (DynamicLevelSet). */
typedef struct mpmhip2d_ctx mpmhip2d_ctx;
typedef struct {
  int32_t res[2];
  float dx, dt;
  float gravity[2];
  int32_t particle_gravity;
  float apic_damping, rpic_damping;
  int32_t clean_boundary, particle_collision;
  int64_t max_particles;
  int32_t device;
  int32_t deterministic;    /* 1 = bitwise reproducible runs (env MPMHIP_DETERMINISTIC=0/1 overrides).  The default substep scatters
                             * with global float atomics (grid, body impulses), so its last bits depend on arrival order.  With the
                             * mode a substep is a function of the particle set (state + creation id) and the bodies only — not of
                             * slot order, launch sizes or arrival order: the particles are sorted by cell, every cell in ascending
                             * (creation id, slot), each particle's P2G record is stored once, every node of the dense grid sums its
                             * nine cells in a fixed order and is written with one plain store; the impulses particles hand to
                             * bodies are summed per workgroup in a fixed tree and the rows added in a fixed order.  No float atomic
                             * remains on the path.  With duplicate creation ids the run is still valid, but the order inside a cell
                             * — and so the last bits — then depends on the slots.  The asynchronous 2D stepper is covered: its pools, gathers and
                             * appends take the ordered forms (mpmhip_async_forms). */
  int32_t reserved[2];
} mpmhip2d_config;
int mpmhip2d_create(const mpmhip2d_config *cfg, mpmhip2d_ctx **out);
void mpmhip2d_destroy(mpmhip2d_ctx *ctx);
const char *mpmhip2d_last_error(const mpmhip2d_ctx *ctx);
/* mpmhip2d_config.deterministic of a live ctx; takes effect from the next substep */
int mpmhip2d_set_deterministic(mpmhip2d_ctx *ctx, int32_t on);
/* the creation ids of the n resident slots, in slot order (the 2D counterpart of mpmhip_upload(MPMHIP_F_ID): a scene uploaded in
 * another order keeps its particles' names).  n must equal the slot count, every id must be >= 0; a deleted slot stays deleted;
 * the counter new particles take their ids from is raised to max + 1.  Refused on a resident asynchronous stepper. */
int mpmhip2d_upload_ids(mpmhip2d_ctx *ctx, int64_t n, const int32_t *ids);
/* MPM<2>::apply_dirichlet_boundary_conditions (src/mpm.cpp:374-399): grid nodes with x < distance_left move with
 * (velocity_left, 0), nodes with x > 1 - distance_right with (velocity_right, 0) — config keys dirichlet_boundary_radius,
 * dirichlet_distance_left / _right, dirichlet_boundary_velocity, dirichlet_boundary_left / _right */
int mpmhip2d_set_dirichlet(mpmhip2d_ctx *ctx, int32_t enabled, float distance_left, float distance_right, float velocity_left,
                           float velocity_right);
int mpmhip2d_set_levelset(mpmhip2d_ctx *ctx, int32_t n0, const mpmhip_shape *shapes0, int32_t n1, const mpmhip_shape *shapes1,
                          float t0, float t1, float friction);
int mpmhip2d_add_group(mpmhip2d_ctx *ctx, int32_t material, const float params[MPMHIP_NPARAM]);
int mpmhip2d_add_particles(mpmhip2d_ctx *ctx, int32_t group, int64_t n, const float *x, const float *v, const float *F,
                           const float *B, const float *aux);
int mpmhip2d_substep(mpmhip2d_ctx *ctx);          /* MPM<2>::substep, src/mpm.cpp:452-575; asynchronous */
int mpmhip2d_step(mpmhip2d_ctx *ctx, float dt);   /* MPM<dim>::step, src/mpm.cpp:428-439 (dt < 0: one substep) */
double mpmhip2d_current_time(const mpmhip2d_ctx *ctx);
int64_t mpmhip2d_num_particles(mpmhip2d_ctx *ctx); /* synchronises */
int64_t mpmhip2d_download(mpmhip2d_ctx *ctx, int64_t capacity, float *x, float *v, float *F, float *B, float *aux, int32_t *gid,
                          int32_t *id);            /* live particles in slot order; NULL outputs are skipped; returns n */
int mpmhip2d_download_grid(mpmhip2d_ctx *ctx, float *grid /* [(res0+1)(res1+1)][3] = (v.x, v.y, m) */);

/* Seeding the 2D simulation on the device — mpmhip_seed_particles with dim = 2 (PoissonDiskSampler<2>: the same code path of the
 * reference serves both dimensions, src/poisson_disk_sampler.h:157-252; only the spacing formula differs, :60-61).  A pure function
 * of its inputs; no particle row passes through host memory.
 *
 * The tile: mpmhip2d_poisson_tile writes min(count, capacity) points, 2 floats each, to `out` (NULL allowed) and returns the count.
 * Bridson's algorithm in the periodic box [-20, 20)^2, minimum distance 1, 30 attempts per active point, the first point at the
 * centre, generated once per process in integer arithmetic (csrc/poisson_tile.h): the same bytes on every machine.
 *
 * The region is "where this level set is negative", independent of the ctx's boundary level set (which is not touched):
 *   sdf == NULL   the first n_shapes of `shapes`, read in the plane exactly as mpmhip2d_set_levelset reads them (z ignored, a box
 *                 unbounded along z, a sphere a disc; phi = min over the shapes);
 *   sdf != NULL   a sampled field phi [res0][res1] (the last axis fastest, fp32, WORLD units; host array, uploaded by the call) on
 *                 the lattice *sdf: sample (0, 0) at `origin`, one `spacing` > 0.  Read bilinearly with the rules of
 *                 mpmhip_set_levelset_sdf, one axis fewer: u = (x - origin) * fl(1 / spacing); inside the lattice iff
 *                 0 <= u <= res - 1 on both axes (a point outside is not in the region); cell c = clamp((int)u, 0, res - 2),
 *                 f = u - c; lerp(a, b, f) = (1 - f) a + f b, along the last axis first.
 * All arithmetic is fp32, in this order, nothing contracted (tests/seed2d_model.py restates it to the bit):
 *   get ready   over the cell centres fl((i + 0.5) dx) of the res[0] x res[1] grid: min / max per axis of the centres inside the
 *               region; min_corner = min - dx, max_corner = max + dx; no centre inside: MPMHIP_EINVAL "region is empty".
 *               min_distance = (float)sqrt(dx^2 / ppc * 2 / 3) (in double), region_size = fl(40 min_distance),
 *               replicas per axis = max(1, ceil((max_corner - min_corner) / region_size)).
 *   candidates  c = i * n_replicas + r pairs tile point i with replica r (the replica index in C order, (ind0, ind1));
 *               q = fl(tile_i * min_distance);  position = fl(fl(q + min_corner) + fl(region_size * (ind + 0.5))).
 *               source = 1 (an emitter called before every frame): q = fl(q + fl(velocity * current_t)), wrapped into the period
 *               q -= fl(floor(fl(fl(q / region_size) + 0.5)) * region_size) — the tile drifts with the jet.
 *   acceptance  inside the region and not within 7 cells of a wall (MPM::near_boundary, src/mpm.h:269-276: X = fl(x * fl(1 / dx)),
 *               min X < 7 or max (X - res) > -7).  source = 1: and position + advection is NOT inside, advection =
 *               velocity * d + 0.5 * gravity * (d + base_delta_t) * d with d = source_delta_t (src/mpm.cpp:222-227).
 *   order       the survivors are appended in ascending c with creation ids next_id + rank (the reference's order).
 *   rows        x, velocity as given, F = initial_dg * I, B = 0, aux the material default of mpmhip2d_add_particles, the group.
 * *n_added = the number of new particles.  If they do not fit the ctx, nothing is written, *n_added is the number needed and the
 * call returns MPMHIP_ECAPACITY: mpmhip2d_reserve and call again.  MPMHIP_EINVAL with a message: an unknown group; ppc not finite
 * or <= 0; a non-finite velocity, initial_dg or source_delta_t; a lattice with res < 2, a non-finite origin, a spacing that is not
 * a finite number > 0, or phi == NULL; an empty region; more than 2^31 candidates; creation ids past 2^31; a resident asynchronous
 * stepper (seed before mpmhip2d_async_begin).  The call synchronises the ctx's stream twice for a few words each; its work
 * buffers belong to the ctx, only grow, and go with mpmhip2d_destroy.
 * The same array serves as the 2D BOUNDARY through mpmhip2d_set_levelset_sdf below, which decides phi < 0 as this call does.
 * Out of scope: pd_packed, non-uniform densities, pd = False, point_cloud; for the boundary: add_slope,
 * rigid_body_levelset_collision with a sampled set, a mesh voxeliser for 2D.
 *
 * mpmhip2d_reserve: the particle arrays hold at least `capacity` particles afterwards (mpmhip2d_config.max_particles of a live
 * ctx); their contents, the clocks, bodies and groups stay.  MPMHIP_OK at once when the capacity already suffices.
 * mpmhip2d_num_slots: the rows the arrays hold, deleted ones included — what the capacity bounds (no synchronisation). */
typedef struct {
  int32_t res[2];
  float origin[2];
  float spacing;
} mpmhip2d_sdf_desc;
typedef struct {
  int32_t n_shapes;
  mpmhip_shape shapes[MPMHIP_MAX_SHAPES];
  const mpmhip2d_sdf_desc *sdf; /* NULL: the region is given by the shapes */
  const float *phi;
  float ppc;                    /* particles per cell the spacing is chosen for (> 0) */
  float velocity[2];
  int32_t source;               /* 0 fill, 1 emitter shell */
  float source_delta_t;
  float initial_dg;
  int32_t reserved;
} mpmhip2d_seed_desc;
int64_t mpmhip2d_poisson_tile(float *out, int64_t capacity);
int mpmhip2d_seed_particles(mpmhip2d_ctx *ctx, int32_t group, const mpmhip2d_seed_desc *desc, int64_t *n_added);
int mpmhip2d_reserve(mpmhip2d_ctx *ctx, int64_t capacity);
int64_t mpmhip2d_num_slots(mpmhip2d_ctx *ctx);
int64_t mpmhip2d_capacity(mpmhip2d_ctx *ctx); /* particles the arrays hold now: mpmhip2d_reserve may give more than it was asked for */

/* Sampled level set as the boundary of the 2D solver — mpmhip_set_levelset_sdf with one axis fewer:
 *   lattice   res[k] >= 2 samples per axis, sample (0, 0) at `origin`, one `spacing` > 0 (world units, independent of the
 *             simulation's delta_x); arrays in C order [i][j] (j fastest), fp32, WORLD units, negative inside the solid.  The ctx
 *             keeps its own device copy (4 res[0] res[1] bytes per key frame).
 *   phi       u = (x - origin) * fl(1 / spacing); cell c = clamp((int)u, 0, res - 2), f = u - c; bilinear in that cell,
 *             lerp(a, b, f) = (1 - f) a + f b along the LAST axis first, then the first — the order of the seeding's sampled
 *             region (mpmhip2d_seed_particles) — returned in grid units (times fl(1 / delta_x)).  A point outside
 *             [origin, origin + (res - 1) spacing] on either axis has NO level set there: nothing is extrapolated.
 *   gradient  per sample the central difference (phi[+1] - phi[-1]) * (0.5 / spacing), one-sided (weight 1 / spacing) on the array's
 *             edges; the four samples' gradients interpolated like phi, normalised; a length below 1e-10 gives the zero vector.
 *   phi1      NULL: static.  Else a second key frame on the same lattice, blended as in 3D: a = (t - t0) / (t1 - t0),
 *             phi = (1 - a) phi0 + a phi1, the normal is the normalised lerp of the two unit gradients,
 *             d phi / dt = (phi1 - phi0) / (t1 - t0); the grid pass forms the boundary velocity -d phi / dt n delta_x from it.
 *   no contraction   no multiply-add of the sampler is fused: every kernel that inlines it gives the same bits for the same point,
 *             and for one array `phi < 0` here and the seeding's "inside" decide identically at every point (a scene seeds a region
 *             and bounds by its complement).  tests/sdf2d_model.py restates the sampler in numpy.
 * Readers: the grid boundary condition (band -3 <= phi <= 0), particle_collision behind G2P (default and deterministic mode; the
 * asynchronous stepper and the CPIC coupling run the same substep), mpmhip2d_delete_particles_inside_level_set.
 * One level set at a time, in both directions: a sampled set replaces the shapes; mpmhip2d_set_levelset replaces a sampled set and
 * frees its arrays.  A call with the installed lattice's size reuses the device memory (the per-frame update of a dynamic set
 * allocates nothing); a static set after a dynamic one frees the second frame.  mpmhip2d_delete_particles_inside_level_set is refused
 * on a resident asynchronous stepper.  MPMHIP_EINVAL with a message: desc or phi0 NULL, res[k] < 2, a non-finite origin, a spacing that is not a
 * finite number > 0, more than 2^31 samples, t1 <= t0 with two frames, rigid_body_levelset_collision (refused in either order of
 * the two calls: that pass keeps reading shapes).  The 2D substep is one host call that only enqueues work, so there is no "inside
 * a substep" state to refuse; the call waits for the ctx's stream before it touches the arrays.
 * Out of scope: add_slope, rigid_body_levelset_collision with a sampled set, a mesh voxeliser for 2D. */
int mpmhip2d_set_levelset_sdf(mpmhip2d_ctx *ctx, const mpmhip2d_sdf_desc *desc, const float *phi0, const float *phi1 /* NULL = static */,
                              float t0, float t1, float friction);
/* general_action "delete_particles_inside_level_set" of MPM<2> (src/mpm.cpp:962-974): deletes every live particle whose level-set
 * value (shapes or a sampled set, at the ctx's current time) at its position is negative; *deleted = their number */
int mpmhip2d_delete_particles_inside_level_set(mpmhip2d_ctx *ctx, int64_t *deleted);
/* the DEVICE's evaluation of the installed 2D level set (sampled or shapes) at n host-given points at time t: phi [n] in grid
 * units, grad [n][2] the unit gradient, dphidt [n], hit [n] = 0 where there is no level set (then the rest is 0) */
int mpmhip2d_debug_levelset_sample(mpmhip2d_ctx *ctx, int64_t n, const float *pos /* [n][2] */, float t, float *phi, float *grad,
                                   float *dphidt, int32_t *hit);
/* the DEVICE's 2D constitutive math on host-given rows, for parity tests (the 2D twins of mpmhip_debug_force / _plasticity / _svd3):
 * the functions the 2D transfer kernels call (csrc/mpm2d_math.h), one lane per row on the ctx's stream.  Matrices are row-major
 * [a b; c d].  MPMHIP_EINVAL for a NULL ctx or array (force_out may be NULL), n < 0, an unknown material id; n == 0 succeeds
 * without a launch.
 *   force:      out = calculate_force(F, aux) = -vol P(F) F^T
 *   plasticity: (F, aux) <- plasticity(cdg, F, aux) in place (water keeps its F); with force_out also calculate_force of the
 *               updated state, the order in which G2P and the next P2G run them
 *   svd2:       the rotation U = [cu -su; su cu] and the signed singular values S (sign of det F on the smaller one) of
 *               F F^T = U diag(S^2) U^T exactly as the models consume them */
int mpmhip2d_debug_force(mpmhip2d_ctx *ctx, int32_t material, const float params[MPMHIP_NPARAM], int64_t n, const float *F /* [n][4] */,
                         const float *aux /* [n] */, float *out /* [n][4] */);
int mpmhip2d_debug_plasticity(mpmhip2d_ctx *ctx, int32_t material, const float params[MPMHIP_NPARAM], int64_t n,
                              const float *cdg /* [n][4] */, float *F /* [n][4], in/out */, float *aux /* [n], in/out */,
                              float *force_out /* [n][4] or NULL */);
int mpmhip2d_debug_svd2(mpmhip2d_ctx *ctx, int64_t n, const float *F /* [n][4] */, float *cu /* [n] */, float *su /* [n] */,
                        float *S /* [n][2] */);

/* Region expressions — CSG combinations of level sets, evaluated per point on the device (csrc/k_region.h: RegionExpr<D>; checks:
 * csrc/region_program.h; host side: csrc/region_api.h).  A region is "where phi < 0", phi in GRID units (what the samplers and the
 * shape evaluator return).  One description serves D = 3 and D = 2.
 *   leaf       one mpmhip_shape (kind 0; for D = 2 read in the plane exactly as mpmhip2d_seed_particles reads it: z ignored, a box
 *              unbounded along z) or one sampled field (kind 1): a lattice plus `field`, an index into the description's list of phi
 *              arrays (several leaves may share one array; D = 2 uses res[0..1], origin[0..1]).  A sampled leaf evaluated OUTSIDE
 *              its lattice has no level set there: phi = +inf.  That point is not in the leaf — and it IS in the leaf's complement.
 *   placement  (placed != 0) maps the leaf's own space to the world: world = t + s R (local - p), R a rotation (D = 3: rot is the
 *              3x3 matrix, row-major, checked for orthonormality to 1e-4 per entry of R^T R and for a positive determinant — a
 *              reflection is refused; D = 2: rot[0] is the angle in radians
 *              and R = [c -s; s c] with c = (float)cos((double)angle), s = (float)sin((double)angle)), s = scale > 0, t = translate,
 *              p = pivot.  The device goes the other way in fp32, in this order, nothing contracted:
 *                d = x - t;   y_k = ((R_0k d_0 + R_1k d_1) + R_2k d_2)   (D = 2: R_0k d_0 + R_1k d_1);
 *                local_k = fl(fl(y_k * fl(1 / s)) + p_k);   phi = fl(phi_leaf(local) * s).
 *              A leaf without a placement takes no arithmetic on x: the bits of the plain region.
 *   band       (banded != 0) with lo < hi in grid units: phi' = max(lo - phi, phi - hi), the shell lo < phi < hi.
 *   operators  on phi, exact in fp32: UNION = min, INTERSECT = max, NEG = -phi.  A difference a - b is INTERSECT(a, NEG b).
 *   program    postfix: PUSH leaf, UNION, INTERSECT, NEG.  At most MPMHIP_REGION_MAX_LEAVES leaves, _MAX_FIELDS arrays, _MAX_OPS
 *              operations, stack depth _MAX_DEPTH (enough for every tree over 8 leaves when the deeper operand of each operator is
 *              evaluated first).
 * The host validates before anything is uploaded or launched; MPMHIP_EINVAL with a message for: an empty program, more than the
 * limits, an unknown opcode, leaf kind or shape type, a shape leaf the level set would refuse (sphere radius <= 0, cuboid without
 * lo < hi on an axis that is read) or with a non-finite parameter, a leaf or field index out of range, stack underflow, depth above 4, a stack that
 * does not end at exactly one value, a rotation that is not finite, not orthonormal or a reflection, scale <= 0 or not finite, a non-finite
 * translation or pivot, lo >= hi or a NaN band edge, a lattice mpmhip_set_levelset_sdf would refuse, a missing phi array.
 *
 * mpmhip_seed_particles_region / mpmhip2d_seed_particles_region: mpmhip_seed_particles with the region given as an expression.  `how`
 * supplies ppc, velocity, source, source_delta_t, initial_dg; its own region fields must be empty (n_shapes == 0, sdf == NULL).
 * Everything else — the candidate arithmetic, the order, refusals, ECAPACITY, ids — is the existing call's; the phi arrays are
 * uploaded back to back into the ctx's seed buffer.  source = 1 keeps a candidate inside the region whose advected position is not.
 * mpmhip_region_sample: no ctx; the device's phi (grid units, +-inf possible) at n host-given points [n][dim] for a grid of cell
 * size delta_x, on `device`.  mpmhip_region_bake: no ctx; phi at the nodes of `lattice` (node index i sits at
 * fl(origin + fl(i * spacing)) per axis, as the mesh voxeliser defines it; dim = 2: res[0..1], origin[0..1]) in WORLD units,
 * fl(phi * delta_x) clamped to +-band (band > 0 finite, world units: the +inf of a sampled leaf cannot reach the array), C order —
 * an array mpmhip_set_levelset_sdf / mpmhip2d_set_levelset_sdf installs as a composite boundary.  min / max composition keeps the
 * zero set and the sign exact and |grad phi| <= 1; away from the surface it is a lower bound of the true distance, not the distance —
 * what the analytic level set already does with several shapes.  Errors of the two: mpmhip_last_error(NULL). */
#define MPMHIP_REGION_MAX_LEAVES 8
#define MPMHIP_REGION_MAX_FIELDS 4
#define MPMHIP_REGION_MAX_OPS 24
#define MPMHIP_REGION_MAX_DEPTH 4
enum { MPMHIP_REGION_PUSH = 0, MPMHIP_REGION_UNION = 1, MPMHIP_REGION_INTERSECT = 2, MPMHIP_REGION_NEG = 3 };
typedef struct {
  int32_t kind;   /* 0 shape, 1 sampled field */
  int32_t field;  /* kind 1: index into fields */
  mpmhip_shape shape;
  int32_t placed, banded;
  float rot[9];
  float scale, translate[3], pivot[3];
  float lo, hi;
} mpmhip_region_leaf;
typedef struct {
  int32_t op, leaf; /* leaf: of a PUSH */
} mpmhip_region_op;
typedef struct {
  int32_t res[3];
  float origin[3];
  float spacing;
  int32_t reserved;
  const float *phi; /* host array, world units, C order */
} mpmhip_region_field;
typedef struct {
  int32_t n_leaves, n_ops, n_fields, reserved;
  mpmhip_region_leaf leaves[MPMHIP_REGION_MAX_LEAVES];
  mpmhip_region_op ops[MPMHIP_REGION_MAX_OPS];
  mpmhip_region_field fields[MPMHIP_REGION_MAX_FIELDS];
} mpmhip_region_desc;
int mpmhip_seed_particles_region(mpmhip_ctx *ctx, int32_t group, const mpmhip_seed_desc *how, const mpmhip_region_desc *region,
                                 int64_t *n_added);
int mpmhip2d_seed_particles_region(mpmhip2d_ctx *ctx, int32_t group, const mpmhip2d_seed_desc *how, const mpmhip_region_desc *region,
                                   int64_t *n_added);
/* Seeding a tiled job — every rank fills its own brick on the device (3D; the 2D solver has no tiling).
 *
 * mpmhip_seed_particles_brick: mpmhip_seed_particles (region == NULL: the plain region of `desc`) or mpmhip_seed_particles_region
 * (region != NULL, and `desc` carries no region of its own) on a ctx with a partition (mpmhip_set_partition, or mpmhip_tiled_setup, which
 * calls it); on a ctx without one: MPMHIP_EINVAL.  A COLLECTIVE BY CONVENTION: every rank of the job makes the same call with the same
 * description, at the same ctx time and with the same next id.  No message is passed.  Every rank evaluates ALL candidates — the price of
 * one call on one ctx — and keeps the survivors whose base cell lies in its brick:
 *   owner      the brick that holds the base cell b[k] = (int)fl(fl(x[k] * fl(1 / dx)) - 0.5f) under the cuts of the partition: what the
 *              migration computes, here with nothing contracted (tiled.base_cells / Partition.rank_of_cells restate it to the bit).
 *              Should the migration's own expression round differently for a particle at an exact cell face, that particle simply
 *              migrates at the next check.
 *   ids        a survivor's id is next_id + (the survivors of the JOB with a smaller c): the id it gets on one ctx.
 *   slots      it is appended behind the resident records at (the survivors of THIS brick with a smaller c): a rank's new records
 *              ascend in id, as on one ctx.
 *   counts     counts[0] = added on this rank, counts[1] = accepted job-wide.  On EVERY rank the next id advances by counts[1], so
 *              the ranks stay in step.  The job-wide set, the ids and the positions are exactly those of the one-ctx calls.
 *   capacity   MPMHIP_ECAPACITY: nothing was written on this rank, its next id has not moved, counts[0] = the particles needed
 *              HERE.  mpmhip_reserve and repeat the call on this rank alone: the call is pure, the repeat gives the same particles.
 * Everything else is the existing calls': the refusals (inside a substep, an unknown group, ppc, the lattice, more than 2^31 candidates),
 * source, initial_dg, the velocity; mpmhip_host_particle_bytes does not change.
 * On a ctx with a native plan (mpmhip_tiled_setup) the call may come between two mpmhip_tiled_advance[_group] calls — an emitter.  It
 * marks the plan stale: the next advance begins with the planning scan of a job's first substep (one scan + table exchange on every
 * rank), which cuts the halo boxes around the new particles; until then the clip box is widened to hold every candidate of the call.
 * On the callback path (mpmhip_set_halo) the plan is the caller's: the call is allowed, planning again is the caller's business.
 * mpmhip_seed_particles and mpmhip_seed_particles_region keep refusing a tiled ctx.
 *
 * mpmhip_seed_histogram: what the partition of such a job is cut from, on any ctx, tiled or not.  hist_a[i] = the survivors of the
 * call whose base cell has index i along axis a (res[a] entries each, NULL allowed), *total their number, cell_bounds = lo3, hi3
 * (exclusive) of their base cells (all 0 without survivors).  Integer counts: exact, whatever the order.  Nothing is written, no
 * counter moves; the ctx's time, gravity and base_delta_t enter as in the seeding call (source = 1).  An empty region: MPMHIP_EINVAL
 * "region is empty".
 *
 * mpmhip_set_next_id raises the creation-id counter to `id`, never lowers it, and returns the counter (>= 0; id = 0 reads it) or a
 * negative error.  A job whose first particles came through mpmhip_upload(MPMHIP_F_ID) — which leaves each rank's counter behind
 * its own largest id — levels its ranks' counters with it before the first collective seeding call. */
int mpmhip_seed_particles_brick(mpmhip_ctx *ctx, int32_t group, const mpmhip_seed_desc *desc,
                                const mpmhip_region_desc *region /* NULL: the plain region of the desc */,
                                int64_t counts[2] /* [0] added on this rank (ECAPACITY: needed here), [1] accepted job-wide */);
int mpmhip_seed_histogram(mpmhip_ctx *ctx, const mpmhip_seed_desc *desc, const mpmhip_region_desc *region /* or NULL */,
                          int64_t *hist_x, int64_t *hist_y, int64_t *hist_z /* res[a] bins each */, int64_t *total,
                          int32_t cell_bounds[6] /* lo3, hi3 (exclusive) of the survivors' base cells */);
int mpmhip_set_next_id(mpmhip_ctx *ctx, int32_t id);
int mpmhip_region_sample(int32_t device, int32_t dim, float delta_x, const mpmhip_region_desc *region, int64_t n,
                         const float *pos /* [n][dim] */, float *phi_out /* [n] */);
int mpmhip_region_bake(int32_t device, int32_t dim, float delta_x, const mpmhip_region_desc *region, const mpmhip_sdf_desc *lattice,
                       float band, float *phi_out);

/* frame output of the 2D simulation — replaces MPM<2>::write_partio (src/visualize.cpp:17-100): the same .bgeo as the 3D
 * entry points above (z = 0), boundary particles of rigid bodies as rows of type 1; with a resident asynchronous stepper the rows
 * are the containers of every particle pool with their block's limits (src/async/async_visualize.cpp:17-26,86-96) */
int mpmhip2d_bgeo_size(mpmhip2d_ctx *ctx, int32_t verbose, size_t *bytes);
int mpmhip2d_bgeo_encode(mpmhip2d_ctx *ctx, int32_t verbose, void *dst, size_t capacity, size_t *written);
int mpmhip2d_write_bgeo(mpmhip2d_ctx *ctx, const char *path, int32_t verbose);
/* snapshots of the 2D simulation — replaces MPM<2>::general_action(action = 'save' | 'load') (src/mpm.cpp:940-960; AsyncMPM<2>:
 * every pool and the block table, src/async/async_mpm.h:120-172): groups, particles, clocks, the rigid bodies' records and joints,
 * the asynchronous stepper's block tables and containers.  Loaded into an object of the same grid whose scene (level set,
 * configuration, the rigid bodies' outlines and scripts, mpmhip2d_async_begin) has been set up again, as for the 3D snapshots. */
int64_t mpmhip2d_snapshot_size(mpmhip2d_ctx *ctx);
int mpmhip2d_snapshot_save(mpmhip2d_ctx *ctx, void *dst, size_t capacity);
int mpmhip2d_snapshot_load(mpmhip2d_ctx *ctx, const void *src, size_t size);

/* ---- AsyncMPM<2> — replaces create_simulation2('async_mpm') (TC_IMPLEMENTATION(Simulation2D, AsyncMPM2D, "async_mpm"),
 * src/async/async_mpm.cpp:423-427): the asynchronous stepper of mpmhip_async_begin / _step above for the 2D simulation
 * object.  A scheduler block is the reference's 2D SPGrid block, 8 x 16 nodes (SPGrid_Mask<5, 5, 2>); the block scheduler
 * (limits, neighbour lists, the action table of an advance) is the same host code as in 3D (csrc/async_sched.h); the pools
 * and backup pools are a device-resident store of 64-byte containers (csrc/k_async.h), and no particle data crosses the
 * host boundary while stepping.
 *   _begin            initialize (:13-55); not with rigid bodies.  After it mpmhip2d_step IS the asynchronous step (the
 *                     reference's virtual Simulation::step) and mpmhip2d_substep is refused.
 *   _pool_particles   add_particles' tail (:62-75): the particles just added with mpmhip2d_add_particles move to the pools of
 *                     their blocks (also done by the next _step)
 *   _step             step (:380-421): update_dt_limits, then advance(level) for every power-of-two level due
 *   _load_pools       AsyncMPM::visualize's particle list (src/async/async_visualize.cpp:86-96): all containers of all particle
 *                     pools become the object's particles (mpmhip2d_download / _num_particles then see the whole state, each
 *                     particle at its block's time; an id can occur more than once, as in the reference); returns their number.
 *                     _view_blocks: the pool block of each, in download order.
 *   _download_pools   every container of every particle pool without touching the object's particles: rows of 16 floats — the
 *                     container as stored, {x2, v2, F4, apic_b4, aux, gid bits, id bits, -} — + its block; rows == NULL: the count
 *   _forms            as mpmhip_async_forms
 *   _state            {current_t_int, update_counter, min_delta_t_int, max_delta_t_int, live containers, store size,
 *                     compactions, steps}
 *   _table            dense block table (block b = bx nb[1] + by): limits, pool sizes, particle_t, backup_t, local_min_dt_limit;
 *                     capacity < number of blocks returns the number only */
int mpmhip2d_async_begin(mpmhip2d_ctx *ctx, const mpmhip_async_config *cfg);
int mpmhip2d_async_pool_particles(mpmhip2d_ctx *ctx);
int mpmhip2d_async_step(mpmhip2d_ctx *ctx, float dt);
int64_t mpmhip2d_async_load_pools(mpmhip2d_ctx *ctx);
int64_t mpmhip2d_async_view_blocks(mpmhip2d_ctx *ctx, int64_t capacity, int32_t *block);
int64_t mpmhip2d_async_download_pools(mpmhip2d_ctx *ctx, int64_t capacity, float *rows, int32_t *block);
int mpmhip2d_async_forms(mpmhip2d_ctx *ctx, int32_t out[4]);
int mpmhip2d_async_state(mpmhip2d_ctx *ctx, int64_t out[8]);
double mpmhip2d_async_current_time(const mpmhip2d_ctx *ctx);
int64_t mpmhip2d_async_table(mpmhip2d_ctx *ctx, int32_t nb[2], int64_t capacity, int64_t *strength, int64_t *cfl, int64_t *continuous,
                             int64_t *count, int64_t *particle_t, int64_t *backup_t, int64_t *local_min);

/* ---- the 2D dense-grid demo (BASELINE configs[0]) — replaces advance(dt) of mls-mpm88.cpp:16-69 (annotated twin
 * mls-mpm88-explained.cpp:64-197): (n+1)^2 grid, snow model inline (E = 1e4, nu = 0.2, hardening 10, sigma clamp
 * [0.975, 1.0075], Jp in [0.6, 20]), gravity -200 on the grid, sticky side/top walls and a separating floor at 0.05.
 * Particle state as the demo's `Particle` (:11-13): x[2], v[2], F[4] row-major, C[4], Jp.  NULL inputs of
 * mpmhip_mpm88_add take the demo's constructor values (v = 0, F = I, C = 0, Jp = 1); NULL outputs of download are
 * skipped.  `plastic` = the demo's `plastic` flag (:10).  Its own small object: no mpmhip_ctx involved. */
typedef struct mpmhip_mpm88 mpmhip_mpm88;
int mpmhip_mpm88_create(int32_t n_grid, float dt, int32_t plastic, int32_t device, mpmhip_mpm88 **out);
void mpmhip_mpm88_destroy(mpmhip_mpm88 *m);
const char *mpmhip_mpm88_last_error(const mpmhip_mpm88 *m);
int mpmhip_mpm88_add(mpmhip_mpm88 *m, int64_t n, const float *x, const float *v, const float *F, const float *C, const float *Jp);
int64_t mpmhip_mpm88_num_particles(const mpmhip_mpm88 *m);
int mpmhip_mpm88_advance(mpmhip_mpm88 *m, int32_t steps);  /* `steps` x advance(dt); asynchronous */
int mpmhip_mpm88_download(mpmhip_mpm88 *m, float *x, float *v, float *F, float *C, float *Jp);  /* synchronises */
int mpmhip_mpm88_download_grid(mpmhip_mpm88 *m, float *grid /* [(n+1)^2][3] = (v.x, v.y, m>0 ? 1 : 0) after advance */);

/* measurement helper: streams `bytes` (rounded down to 16; two scratch buffers of that size are allocated and freed)
 * through a plain copy kernel `iters` times on the ctx stream and returns the best rate in GB/s, counting the bytes
 * read plus the bytes written.  bench.py reports it next to the nominal HBM peak.  Synchronises. */
int mpmhip_debug_copy_bandwidth(mpmhip_ctx *ctx, size_t bytes, int32_t iters, double *gb_per_s);
/* measurement helper: 1 when the next substep's G2P is k_g2p_packed (chunks of 256 consecutive sorted positions; large
 * one-material problems without rigid bodies or tiling), 0 when it is k_g2p (chunks inside one block) */
int mpmhip_debug_g2p_is_packed(const mpmhip_ctx *ctx);
/* test helper: what plan_g2p / plan_p2g (csrc/launch_plan.h) answer for the ctx as it stands, i.e. which instantiations of the
 * transfer kernels the next substep launches.  Nothing is launched.  out[0] packed (k_g2p_packed instead of k_g2p), [1] material set
 * of k_g2p / k_g2p_packed: 0 ONE, 1 NO_VISCO, 2 ALL, [2] its bit 1 << material when ONE, else 0, [3] STORE_B, [4] RIGID (k_p2g_rigid
 * and k_g2p_rigid take the blocks near a body), [5] material set of those two: 0 ONE, 2 ALL, 3 ALL_DET, [6] its bit when ONE, [7] 1 when
 * P2G's colour-aware kernel runs, on the set of [5] / [6] */
int mpmhip_debug_transfer_plan(const mpmhip_ctx *ctx, int32_t out[8]);
/* the launch bound of the single-pass (chained) scans of the sort as a function of the occupancy API's answer: `limit` = workgroups
 * the host launches at most, `resident` = workgroups the device certainly keeps resident (one per CU below the API's number, at most
 * 7).  Pure host arithmetic (no device): mpmhip_create checks limit <= resident for every such kernel; the waits are bounded besides. */
/* measurement helper: census of cond(F) = sigma_max / sigma_min over the live particles of the ctx (the state as stored: elastic
 * deformation gradients after the last return mapping).  out[0] live particles, [1] particles with cond > 8 — the ones the
 * eigen-solve of the transfer kernels finishes on F itself —, [2] waves of 64 consecutive slots, [3] waves
 * holding such a particle, [4] max cond, [8 + b] histogram over b = floor(8 log2 cond) (eighth-octave bins, clamped to 255).
 * Synchronises.  (What decides whether the device's fp32 tolerances hold: they do to cond 1e2) */
#define MPMHIP_COND_CENSUS_WORDS 264
int mpmhip_debug_cond_census(mpmhip_ctx *ctx, double out[MPMHIP_COND_CENSUS_WORDS]);
int mpmhip_debug_scan_grid(int32_t n_cus, int32_t per_cu, int32_t env_request, uint32_t *limit, uint32_t *resident);
/* test helpers: a read-only view of what the last sort built, while the particles are still sorted (behind mpmhip_sort, before the next
 * G2P, upload or deletion) — tests/test_gpu_sort_tables.py holds every table against a numpy model.  Both synchronise the ctx
 * stream, launch nothing, and fail with MPMHIP_EINVAL unless the particles are sorted.
 * mpmhip_debug_sort_info: out[0] n_slots, [1..6] the device counters n_sorted, n_active, n_dead, error (reported, not raised),
 * rank_mode (the path of k_rank in the NEXT sort), n_own; what the plan chose: [7] 1 the keyed two-launch front / 0 the four launches,
 * [8] 1 the cell table with neighbour rows + owner list / 0 the plain one, [9] blocks per chunk of the cell table, [10] form of the
 * in-cell ordering (0 a lane per cell, 1 a wave per block; -1 the deterministic mode was off), [11] 1 that ordering read cached ids /
 * 0 the records; [12] list_valid, [13] bitmap words, [14] max_blocks, [15] Morton bits per axis.
 * mpmhip_debug_sort_array: copies array `which` to dst; returns the bytes written, or MINUS the bytes needed when capacity_bytes is
 * too small (nothing is written; the sizes are multiples of 4, the errors MPMHIP_EINVAL and MPMHIP_EHIP are not).  All are 32-bit words.  na = min(n_active, max_blocks):  SLOT_ID [n_slots] creation id per slot, -1
 * for a deleted slot; BITS, WPREFIX [bitmap words]; ACT_BLK [na]; ACT_START [na + 1]; CELL_START [64 na + 1]; PERM [n_sorted] the
 * sorted index as the transfer kernels read it; NBR [32 na] and OWN_LIST [n_own] (empty unless list_valid); CHUNK_BLK
 * [ceil(n_sorted / 256)] the block holding sorted position 256 k. */
#define MPMHIP_SORT_INFO_WORDS 16
enum { MPMHIP_SORT_SLOT_ID = 0, MPMHIP_SORT_BITS = 1, MPMHIP_SORT_WPREFIX = 2, MPMHIP_SORT_ACT_BLK = 3, MPMHIP_SORT_ACT_START = 4,
       MPMHIP_SORT_CELL_START = 5, MPMHIP_SORT_PERM = 6, MPMHIP_SORT_NBR = 7, MPMHIP_SORT_OWN_LIST = 8, MPMHIP_SORT_CHUNK_BLK = 9 };
int mpmhip_debug_sort_info(mpmhip_ctx *ctx, int64_t out[MPMHIP_SORT_INFO_WORDS]);
int64_t mpmhip_debug_sort_array(mpmhip_ctx *ctx, int32_t which, void *dst, int64_t capacity_bytes);
/* 64-byte record gather of KNOWN size — the access pattern of k_p2g / k_g2p (a lane fetches one whole record with four
 * 16-byte loads through an index): n (a power of two) records, index pattern 0 identity / 1 shuffled runs of 8 /
 * 2 fully shuffled.  Reads exactly (64 + 4) n bytes per launch: the yardstick rocprofv3's FETCH_SIZE is calibrated
 * against for this access width (profiles/calibrate_fetch.py). */
int mpmhip_debug_gather_bandwidth(mpmhip_ctx *ctx, int64_t n_records, int32_t mode, int32_t iters, double *gb_per_s);
/* device and pinned arrays this process's objects hold right now (arrays, not bytes; every ctx, 2D object and mpm88 object
 * together; the halo arena of a tiled ctx is not counted).  An object gives back what it took when the number after its destroy
 * is the number before its create.  No device call. */
int64_t mpmhip_debug_live_buffers(void);
/* milliseconds of the phases of the last mpmhip_bgeo_encode_group of this process, between events on its stream (src/visualize.cpp:
 * 17-100 has no counterpart: a measuring aid): top, mark, prefix, rows, copy to the host. */
int mpmhip_debug_frame_phases(double ms[5]);

/* debug/parity helpers running the device math on host arrays (n items each) */
int mpmhip_debug_svd3(mpmhip_ctx *ctx, int64_t n, const float *F, float *U, float *S, float *V);
int mpmhip_debug_force(mpmhip_ctx *ctx, int32_t material, const float params[MPMHIP_NPARAM], int64_t n,
                       const float *F, const float *aux, float *out);
/* next_force == NULL: plasticity(cdg) alone; else the fused "plasticity + next substep's calculate_force" of k_g2p */
int mpmhip_debug_plasticity(mpmhip_ctx *ctx, int32_t material, const float params[MPMHIP_NPARAM], int64_t n,
                            const float *cdg, float *F, float *aux, float *next_force);

/* CPIC rigid coupling of MPM<2> (bodies made of segments; same semantics as the 3D entry points below).  A script
 * returns the position in out[0..1] resp. the angle in degrees in out[0]. */
typedef void (*mpmhip_script_fn)(void *user, float t, float out[3]);
typedef struct mpmhip2d_rigid_config {
  int32_t codimensional, recenter, reverse_vertices, reserved0;
  float density;            /* <= 0: 40 (codimensional) / 400 */
  float friction[2], restitution;
  float scale[2];
  float initial_position[2], initial_rotation /* degrees */, initial_velocity[2], initial_angular_velocity;
  float linear_damping, angular_damping;
  mpmhip_script_fn scripted_position; void *position_user;
  mpmhip_script_fn scripted_rotation; void *rotation_user;
} mpmhip2d_rigid_config;
int mpmhip2d_set_rigid_coupling(mpmhip2d_ctx *ctx, float penalty, float pushing_force);
/* MPM<2>::rigid_body_levelset_collision (src/mpm_rigid_body.cpp:347-387, config key rigid_body_levelset_collision): see
 * mpmhip_set_rigid_levelset_collision */
int mpmhip2d_set_rigid_levelset_collision(mpmhip2d_ctx *ctx, int32_t enabled);
int mpmhip2d_add_rigid_body(mpmhip2d_ctx *ctx, const mpmhip2d_rigid_config *cfg, int64_t n_segments, const float *segments /* n x 4 */);
/* joints in 2D: type = MPMHIP_JOINT_ROTATION only (scripts/mls-cpic/sand_wheel_2D.py:88); struct below, in the CPIC section */
struct mpmhip_joint_config;
int mpmhip2d_add_articulation(mpmhip2d_ctx *ctx, const struct mpmhip_joint_config *cfg);
int mpmhip2d_set_articulation_iterations(mpmhip2d_ctx *ctx, int32_t n);
int mpmhip2d_rigid_get_state(mpmhip2d_ctx *ctx, int32_t id, float *out /* [10]: pos 2, angle, vel 2, omega, mass, inv_mass, inertia, inv_inertia */);
int64_t mpmhip2d_rigid_get_samples(mpmhip2d_ctx *ctx, int32_t id, int64_t capacity, float *position);
int64_t mpmhip2d_rigid_get_mesh(mpmhip2d_ctx *ctx, int32_t id, int64_t capacity_segments, float *segments /* n x 4, world space */);
int mpmhip2d_cdf_phase(mpmhip2d_ctx *ctx); /* rasterize_rigid_boundary + gather_cdf (parity tests) */
int mpmhip2d_download_cdf(mpmhip2d_ctx *ctx, uint32_t *states, float *distance); /* dense (res+1)^2 */
int64_t mpmhip2d_download_colours(mpmhip2d_ctx *ctx, int64_t capacity, uint32_t *states, float *distance, float *normal, int32_t *near);

/* ---------------------------------------------------------------------------------------------------------------------
 * CPIC rigid coupling (3D) — replaces add_particles(type='rigid', ...) (src/mpm.cpp:80-83 -> MPM::add_rigid_particle,
 * src/mpm_rigid_body.cpp:130-252), rasterize_rigid_boundary / gather_cdf (src/rigid_transfer.cpp), the rigid branches of
 * the transfers (block_op_rigid, src/transfer.cpp:367-463,706-835) and advect_rigid_bodies (src/mpm_rigid_body.cpp:255-286).
 * Once a body exists, every substep runs: sort | rasterize_rigid_boundary | gather_cdf | P2G | grid | G2P | advect.
 * Rigid-rigid collisions (rigidify) are an opt-in pass: mpmhip_set_rigid_collision at the end of this section; joints:
 * mpmhip_add_articulation below.  Rigid bodies cannot be combined with asynchronous stepping; on a tiled job: "Bodies on a job".
 * ------------------------------------------------------------------------------------------------------------------ */
/* scripted_position(t) -> world position; scripted_rotation(t) -> Euler angles in degrees (applied X * Y * Z):
 * tc.function13 objects in the scene scripts (scripts/mls-cpic/sand_paddles.py:27, src/mpm_rigid_body.cpp:79-92) */
typedef struct mpmhip_rigid_config {
  int32_t codimensional;     /* a shell (cuts the material) instead of a solid; mandatory key of the reference */
  int32_t recenter;          /* 1 (reference default): the mesh is moved so that its centre of mass is the body origin */
  int32_t reverse_vertices;  /* flip the orientation of every triangle */
  int32_t reserved0;
  float density;             /* <= 0: the reference's default, 40 (codimensional) / 400 */
  float friction[2];         /* friction0 / friction1: the two sides of the surface ('friction' sets both) */
  float restitution;
  float scale[3];            /* 0 = 1 */
  float initial_position[3], initial_rotation[3] /* Euler, degrees */, initial_velocity[3], initial_angular_velocity[3];
  float rotation_axis[3];    /* angular velocity restricted to this (world) axis when max |axis| > 0.1 */
  float linear_damping, angular_damping;
  mpmhip_script_fn scripted_position; void *position_user;  /* null: a free body */
  mpmhip_script_fn scripted_rotation; void *rotation_user;
} mpmhip_rigid_config;

/* 'penalty' and 'pushing_force' of MPM::initialize (src/mpm.cpp:35,40); defaults 0 and 20000 */
int mpmhip_set_rigid_coupling(mpmhip_ctx *ctx, float penalty, float pushing_force);
/* triangles: n_triangles x 9 floats (mesh space, before `scale`).  Returns the body's index (>= 1; 0 = background) —
 * the string add_particles returns for type='rigid' (src/mpm.cpp:82) */
int mpmhip_add_rigid_body(mpmhip_ctx *ctx, const mpmhip_rigid_config *cfg, int64_t n_triangles, const float *triangles);
int32_t mpmhip_num_rigid_bodies(const mpmhip_ctx *ctx); /* including the background body: rigids.size() */
/* out[33]: position 3, rotation quaternion (w,x,y,z) 4, velocity 3, angular velocity 3, mass, inv_mass,
 * inertia 9 (body frame, row-major), inv_inertia 9 */
int mpmhip_rigid_get_state(mpmhip_ctx *ctx, int32_t id, float *out);
int mpmhip_rigid_set_velocity(mpmhip_ctx *ctx, int32_t id, const float *velocity, const float *angular_velocity);
/* A digest of the bodies as this ctx holds them: the device records of all bodies (pose, velocities, mass properties), the numeric
 * part of their configs, the boundary particles with their creation ids, the elements, the joints and the coupling's settings.
 * Every rank of a tiled job holds ALL bodies ("Bodies on a job", below): ranks compare digests instead of shipping records.
 * Synchronises the ctx's stream. */
int mpmhip_rigid_digest(mpmhip_ctx *ctx, uint64_t out[2]);
/* the boundary particles sampled on the body's triangles (RigidBoundaryParticle, src/boundary_particle.h): world
 * position, offset from the centre of mass in the body frame, body index; id < 0: all bodies.  Returns the count. */
int64_t mpmhip_rigid_get_samples(mpmhip_ctx *ctx, int32_t id, int64_t capacity, float *position, float *offset, int32_t *body);
/* the body's triangles in world space, 9 floats each (write_rigid_body, src/visualize.cpp:102-154: the rigid_%03d_%04d.obj
 * next to every .bgeo frame).  Returns the triangle count. */
int64_t mpmhip_rigid_get_mesh(mpmhip_ctx *ctx, int32_t id, int64_t capacity_triangles, float *triangles);
/* phases (parity tests; mpmhip_substep runs them itself): rasterize_rigid_boundary, gather_cdf (needs a sort),
 * advect_rigid_bodies(base_delta_t) */
int mpmhip_rasterize_rigid_boundary(mpmhip_ctx *ctx);
int mpmhip_gather_cdf(mpmhip_ctx *ctx);
int mpmhip_advect_rigid_bodies(mpmhip_ctx *ctx);
/* joints between rigid bodies — replaces general_action(action='add_articulation', type=..., obj0=..., obj1=...)
 * (src/mpm.cpp:923-933; the Articulation classes of src/articulation.cpp; mpm.add_articulation(...) in
 * scripts/mls-cpic/robot.py:103, water_wheel.py:81).  obj1 = 0 links to the background body.  The joint is set up on the
 * bodies' poses at the time of the call; MPM::articulate (src/mpm.h:278-319) then runs inside every substep between the
 * sort and rasterize_rigid_boundary: apply(dt), articulation_iterations (100) Gauss-Seidel sweeps of project(), penalize(dt). */
enum {
  MPMHIP_JOINT_ROTATION = 0,  /* 'rotation': both bodies share one angular velocity (their total angular momentum)        */
  MPMHIP_JOINT_FROZEN = 1,    /* 'frozen': obj0 keeps angular velocity z and velocity x, y only                           */
  MPMHIP_JOINT_DISTANCE = 2,  /* 'distance': anchors offset0 / offset1 (world-frame offsets from the centres) at target_distance */
  MPMHIP_JOINT_AXIAL_ROTATION = 3, /* 'axial_rotation': hinge about `axis` through obj0's centre + offset0                */
  MPMHIP_JOINT_MOTOR = 4,     /* 'motor': hinge + torque `power` about the axis                                           */
  MPMHIP_JOINT_STEPPER = 5    /* 'stepper': hinge + relative angular velocity about the axis held at `angular_velocity`   */
};
typedef struct mpmhip_joint_config {
  int32_t type, obj0, obj1;
  int32_t has_offset1;          /* 'offset1' given (mandatory for a distance joint to the background body)        */
  int32_t has_target_distance;  /* 'target_distance' given; otherwise the anchors' distance at the time of the call */
  float offset0[3], offset1[3];
  float target_distance;
  float penalty;                /* < 0: the reference's default 1e3 */
  float axis[3];
  float axis_length;            /* < 0: the reference's default 0.1 */
  float power, angular_velocity;
} mpmhip_joint_config;
int mpmhip_add_articulation(mpmhip_ctx *ctx, const mpmhip_joint_config *cfg);
int32_t mpmhip_num_articulations(const mpmhip_ctx *ctx);
int mpmhip_set_articulation_iterations(mpmhip_ctx *ctx, int32_t n); /* config key 'articulation_iterations', default 100 */
int mpmhip_articulate(mpmhip_ctx *ctx); /* phase (parity tests): MPM::articulate(base_delta_t) */
/* dense (res+1)^3 views of the grid's colored distance field: GridState::states (24 colour bits | body id + 1 << 24,
 * src/mpm_fwd.h:69-105) and GridState::distance */
int mpmhip_download_cdf(mpmhip_ctx *ctx, uint32_t *states, float *distance);
/* gather_cdf's per-particle results, live particles in slot order, 5 floats each: boundary_normal 3, boundary_distance,
 * near_boundary.  Valid between mpmhip_gather_cdf and the next G2P (a G2P moves the records). */
int64_t mpmhip_download_boundary(mpmhip_ctx *ctx, float *out, int64_t n_capacity);

/* Bodies on a job — CPIC rigid bodies on a tiled ctx with the native data plane (mpmhip_tiled_setup; csrc/tiled_api.h, csrc/k_rigid_rows.h).
 * Every rank of the job holds ALL bodies: add the same bodies (and joints), in the same order, on every rank BEFORE mpmhip_tiled_setup
 * (mpmhip_set_partition alone may come first).  The set-up sizes the arena for the bodies' impulse rows; a body added afterwards is
 * refused (add the bodies first, or set the job up again).  The records of the bodies are byte-identical on all ranks at every
 * substep boundary: compare mpmhip_rigid_digest across the ranks.
 *   Per substep everything that acts on the bodies alone (joints, the colored distance field of all bodies, the level-set collision,
 *   the advection, the scripts) runs replicated on every rank.  What a rank's colour-aware transfer kernels hand the bodies is the
 *   rank's impulse ROW, 12 bodies (the most a simulation holds, the background included) x 6 floats = 288 bytes: twice a substep — behind the rigid P2G and behind the rigid
 *   G2P — the rows of all ranks reach every rank, which adds them in RANK ORDER and applies the sum.  Peer wires (IPC, LOCAL): peer
 *   writes and epoch words of their own, behind the same bounded wait as the halo boxes (MPMHIP_TILE_WAIT_S; error bit 16).  RCCL:
 *   one send / receive pair per peer (MPMHIP_WIRE_LOCAL_RCCL: the same pairs as self-sends).  No host synchronisation per substep.
 *   mpmhip_set_overlap(1) is accepted and ignored: a ctx with bodies runs its substeps unsplit.
 *   mpmhip_config.deterministic: the rows are fixed-order sums; two runs of a job end byte-identical.
 * Refused, each with a message and the ctx untouched: the callback path (mpmhip_set_halo, mpmhip_tiled_run) on a ctx with bodies;
 * rigid_body_collision (mpmhip_set_rigid_collision) on a tiled ctx; the asynchronous stepper; mpmhip_tiled_redistribute(_group), the
 * frames and snapshots of a job (mpmhip_bgeo_*_group, mpmhip_bgeo_rows_ranked, mpmhip_snapshot_*_group, mpmhip_snapshot_load_brick)
 * and mpmhip_calculate_energy(_group) of a job with bodies.  mpmhip_seed_particles_brick keeps working (an emitter onto a wheel).
 * The multi-rank RCCL transport of the rows has not been on more than one GPU: on one it is reached through
 * MPMHIP_WIRE_LOCAL_RCCL and the one-rank case. */

/* ---- rigid-rigid collisions: MPM::rigidify (src/mpm_rigid_body.cpp:306-345), 3D only as in the reference
 * (RigidSolver<2>::detect_rigid_collision is TC_NOT_IMPLEMENTED, src/rigid_body_solver.h:154-158).
 * Detection replaces RigidSolver<3>::detect_rigid_collision (src/rigid_body_solver.h:160-198): libccd's ccdMPRPenetration on the convex
 * hulls of the bodies' mesh vertices (supportRigid, :120-147) for every pair i > j >= 1 that is not fully scripted on both sides
 * (:174-176) — convex hulls only, as there; a concave mesh collides as its hull.  The device reproduces libccd's single-precision
 * arithmetic bit for bit (taichi_mpm_amd/csrc/k_rigid_collide.h).  The collision list is in (i, j) order; the reference's is in the
 * order its TBB threads arrive (:167, :191-195).  Resolution replaces Collision::project_velocity / project_position (:39-87) and
 * the loops of rigidify (src/mpm_rigid_body.cpp:325-344).
 *
 * mpmhip_set_rigid_collision: the config keys rigid_body_collision (src/mpm_rigid_body.cpp:308; OFF by default here, on in the
 * reference), rigid_body_iterations (5), rigid_penalty (1e3), rigid_body_position_iterations (true) (:327-330).  MPMHIP_EINVAL on a
 * ctx that takes no bodies (tiled, asynchronous) and for iterations < 0.  With the pass on and at least two bodies beside the
 * background, every substep starts its rigid block with rigidify (src/mpm.cpp:468); with it off a substep issues what it issued
 * before this entry point existed.  Snapshots carry the four settings. */
int mpmhip_set_rigid_collision(mpmhip_ctx *ctx, int32_t enabled, int32_t iterations, float rigid_penalty, int32_t position_iterations);
int mpmhip_rigidify(mpmhip_ctx *ctx); /* phase, like mpmhip_articulate: MPM::rigidify(base_delta_t) */
/* the collisions the last rigidify resolved: 9 floats per row — body i, body j (i > j), depth, dir[3], pos[3] (Collision<3>, :20-37).
 * Returns the length of the list; rows beyond cap are not written. */
int64_t mpmhip_rigid_get_collisions(mpmhip_ctx *ctx, int64_t cap, float *out);
/* the hull vertices of body id as the support mapping walks them (supportRigid, :136-146): body frame, three per triangle in
 * element order, 3 floats each.  Returns the body's vertex count; vertices beyond cap_vertices are not written. */
int64_t mpmhip_rigid_get_hull(mpmhip_ctx *ctx, int32_t id, int64_t cap_vertices, float *out);
/* The detection kernel alone, no ctx (as mpmhip_debug_levelset_sample is for the sampler): pair q is cloud 2q against cloud 2q + 1;
 * cloud k has the vertices [offsets[k], offsets[k + 1]) of verts [][3] (offsets[0] = 0, 2 n_pairs + 1 entries), the rotation
 * rotations[9 k] (row-major; NULL: none, the vertices are used as they are) and the centre centres[3 k].  out: 9 floats per pair —
 * hit (1 where ccdMPRPenetration returns 0), depth, dir[3], pos[3], the number of support calls.  MPMHIP_EHIP when a loop bound
 * expired (libccd's max_iterations is unlimited).  Errors: mpmhip_last_error(NULL). */
int mpmhip_rigid_mpr_test(int32_t device, int32_t n_pairs, const float *verts, const int64_t *offsets, const float *rotations,
                          const float *centres, float *out);

#ifdef __cplusplus
}
#endif
#endif /* MPMHIP_H */
