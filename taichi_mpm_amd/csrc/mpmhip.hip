// taichi_mpm_amd/csrc/mpmhip.hip — MI355X (gfx950) MLS-MPM time-stepping core: the C ABI (include/mpmhip.h) and
// the host side of the ctx.  The kernels live next to this file, one header per phase:
//   mpm_common.h (records, parameter blocks, Morton keys)   mpm_math.h (3x3 math, constitutive models, level set)
//   k_sort.h  k_p2g.h  k_grid.h  k_g2p.h  k_tiling.h  k_particles.h  k_debug.h
//   k_seed.h (particle seeding from the periodic Poisson-disk tiles, poisson_tile.h; both dimensions)
//   k_region.h (region expressions: CSG programs over level-set leaves, the region of a seeding call or sampled on a lattice)
//   k_bgeo.h (.bgeo frame rows)   k_frame.h (the rows of a whole job, ranked by id: its own translation unit, k_frame.hip)   k_mpm88.h (the 2D dense-grid demo, its own small object)
//   k_fields.h (particle fields to and from caller-owned device arrays; in k_frame.hip too; host driver fields_api.h)
// host_mem.h: DevBuf / PinnedBuf, the owners of every device and pinned array of the objects below (a new array needs a field and
// its allocation, nothing else); what a kernel takes by value keeps raw pointers into them.
// record_state.h: RecordState, the owner of the ctx's validity flags (which arrays describe the current particles); the host code
// changes them through its named transitions only.
// launch_plan.h: Knobs (the tuning switches of the substep path, from the environment), Facts and the pure plan_sort / plan_p2g /
// plan_grid / plan_g2p: which kernel instantiation a phase launches and with how many workgroups.  do_sort / do_p2g / do_grid /
// do_g2p compute their plan, map it to a kernel pointer and launch; they decide nothing themselves.
//
// One substep (reference: MPM<3>::substep, src/mpm.cpp:452-575):
//
//   sort   (index sort; replaces sort_particles_and_populate_grid src/mpm.cpp:770-918 and
//           clear_boundary_particles :582-633 — dead particles simply drop out of the index)
//          [k_build_keys]  key = Morton(block) << 6 | cell-in-block per particle (normally produced by the
//                          previous substep's k_g2p, which knows the new position)
//          k_sort_front   ONE launch, two roles (grids up to 508 nodes per axis; do_sort):
//            block table  byte flags -> active-block bitmap + popcount prefix (dense slot of every active block)
//                         + active-block list, one single-pass chained scan
//            ranks        rank of each particle in its cell on counters indexed by the KEY (one global atomic per run of equal
//                         keys, or — when the particle order has decayed — an LDS hash per 1024 slots and one atomic per distinct
//                         cell), four consecutive slots per thread, one packed (rank, key) word per slot
//                         (larger grids: k_block_table, then k_rank on counters indexed by the block's dense slot)
//          k_cell_table   per-cell counts -> start of every cell / block in the sorted index (single pass); with the owner list
//                         of the grid pass where that pass walks it (small problems, tiled contexts)
//          k_perm_keyed   sorted position -> particle slot (k_perm after k_rank)
//   P2G    k_p2g   one wavefront per active 4x4x4-cell block, ONE LANE PER CELL: register accumulation of the
//                  27x4 node contributions over the cell's particles (the wave loads two particles of every cell
//                  at a time, whole records per load instruction, into LDS, one window ahead),
//                  ordered non-atomic float4 merge into the block's 6^3-node LDS tile, tile written out whole
//                                                                                (src/transfer.cpp:467-569)
//   grid   k_grid  sums the <=8 overlapping block tiles of every touched grid block, normalises,
//                  gravity + level-set boundary                                  (src/mpm.cpp:277-372)
//   G2P    k_g2p   6^3 velocity tile in LDS, 27-tap gather, F update, plasticity AND the next substep's stress
//                  from one eigen-solve, advection, next key                     (src/transfer.cpp:837-954)
//
// Data layout (fp32, resident in HBM for the life of the ctx):
//   particles  two arrays of 64-byte records indexed by a stable particle slot (the reference's
//              ParticleAllocator pool index, src/particle_allocator.h:36):
//                RecG {x3, aux, F9, gid, pid, -}   what G2P reads and rewrites
//                RecP {x3, v3, A9, mass}           what P2G reads;  A = stress*(-4 inv_dx dt) + apic_b*(4 m)
//              (src/transfer.cpp:521-522) is produced by G2P, so P2G carries no constitutive work, and
//              apic_b itself goes to a side array (it is only ever consumed through A).
//              Particles never move in memory between substeps: `perm` (sorted position -> slot) is rebuilt
//              every substep and both transfer kernels gather whole 64-byte records through it, one record per
//              lane.  This mirrors the reference's own structure — sorted index array every substep
//              (mpm.cpp:785-807) + physical reorder only every `reorder_interval` substeps (:811-813).
//   blocks     an "active" block = 4x4x4 cells holding >=1 particle; bitmap over the Morton block space +
//              per-word popcount prefix -> dense slot = rank in Morton order, no pass over the whole grid.
//   tiles      float4[216] per active block: its private (4+2)^3-node P2G result.
//   gridv      float4[64] per touched grid block (v.xyz, m); slot = 8a+o of the owning (active block a,
//              corner offset o); `fat_slot` maps Morton block -> slot.
// No float atomics anywhere (LDS float atomics cost ~2 cycles per lane on gfx950; global ones leave the L2).

#include <hip/hip_runtime.h>

#include <immintrin.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include <hipcub/hipcub.hpp>  // one plain device sort (the reference's order of the rigid boundary particles, rigid_api.h)
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only (tiled_api.h): librccl is dlopen'ed, this library does not link it


#include "host_mem.h"
#include "record_state.h"
#include "launch_plan.h"
#include "tiled_plan.h"
#include "sdf_lattice.h"
#include "region_program.h"
#include "snapshot_blob.h"
#include "rigid_setup.h"
#include "mpm_common.h"
#include "k_sort.h"
#include "k_particles.h"
#include "k_async.h"
#include "k_p2g.h"
#include "k_grid.h"
#include "k_tiling.h"
#include "k_g2p.h"
#include "k_g2p_packed.h"
#include "k_rigid_transfer.h"
#include "k_rigid_collide.h"
#include "k_debug.h"
#include "k_sdf.h"
#include "k_mesh_sdf.h"
#include "k_seed.h"
#include "k_region.h"
#include "poisson_tile.h"
#include "k_bgeo.h"
#include "frame_launch.h"
#include "snapshot_job_launch.h"
#include "rigid_rows_launch.h"
#include "fields_launch.h"
#include "k_mpm88.h"
#include "k_mpm2d.h"
#include "k_mpm2d_det.h"
#include "k_debug2d.h"
#include "k_sdf2d.h"


// ================================================================================================ host side
using namespace mpm;

// __launch_bounds__ waves/SIMD of k_g2p.  (256, 3) states the 168-VGPR budget explicitly but was measured 3 % slower
// (profiles/r03_h_ab_refactor.txt: w2 against default); the budget is guarded by tests/test_kernel_budget_cpu.py instead
constexpr int G2P_MIN_WAVES = 2;
// One material in the ctx (mask = 1u << t): the instantiation of a transfer kernel that carries only that material's
// calculate_force(), pick(std::integral_constant<uint32_t, 1u << t>()); several materials: fallback.  The materials in SKIP keep the
// fallback and are not instantiated.
template <uint32_t SKIP, class K, class Pick, int... T>
static K one_material(uint32_t mask, K fallback, Pick pick, std::integer_sequence<int, T...>) {
  K k = fallback;
  auto one = [&](auto bit) {
    if constexpr ((decltype(bit)::value & MAT_ALL & ~SKIP) != 0u) { if (mask == bit.value) k = pick(bit); }
  };
  (one(std::integral_constant<uint32_t, 1u << T>()), ...);
  return k;
}
template <uint32_t SKIP = 0, class K, class Pick>
static K one_material(uint32_t mask, K fallback, Pick pick) {
  return one_material<SKIP>(mask, fallback, pick, std::make_integer_sequence<int, 32>());
}

// ---- a launch plan (launch_plan.h) -> the kernel it names: one function per kernel family, the only places that spell instantiations out
// k_cell_table (neighbour rows + owner list) / k_cell_table_plain at the plan's chunk size, on the key-indexed or the per-block counters
template <class K> static K by_chunk(int ct, K k16, K k32, K k64) { return ct == 16 ? k16 : (ct == 32 ? k32 : k64); }
static auto cell_table_kernel(const lp::SortPlan &p) {
  return p.keyed ? by_chunk(p.ct, k_cell_table<16, true>, k_cell_table<32, true>, k_cell_table<64, true>)
                 : by_chunk(p.ct, k_cell_table<16, false>, k_cell_table<32, false>, k_cell_table<64, false>);
}
static auto cell_table_plain_kernel(const lp::SortPlan &p) {
  return p.keyed ? by_chunk(p.ct, k_cell_table_plain<16, true>, k_cell_table_plain<32, true>, k_cell_table_plain<64, true>)
                 : by_chunk(p.ct, k_cell_table_plain<16, false>, k_cell_table_plain<32, false>, k_cell_table_plain<64, false>);
}
// the colour-aware transfer kernels of a plan's material set (deterministic mode: the all-material form with the impulse rows, summed
// by do_rigid_apply_tmp)
static auto rigid_p2g_kernel(lp::MatSet m) {
  if (m.kind == lp::MatSet::ALL_DET) return k_p2g_rigid<MAT_ALL | MAT_DET>;
  return one_material(m.kind == lp::MatSet::ONE ? m.bit : 0u, k_p2g_rigid<MAT_ALL>, [](auto b) { return k_p2g_rigid<b.value>; });
}
static auto rigid_g2p_kernel(lp::MatSet m) {
  if (m.kind == lp::MatSet::ALL_DET) return k_g2p_rigid<MAT_ALL | MAT_DET>;
  return one_material(m.kind == lp::MatSet::ONE ? m.bit : 0u, k_g2p_rigid<MAT_ALL>, [](auto b) { return k_g2p_rigid<b.value>; });
}
// the grid pass's kernels: the owner-list walk (modes 0, 4, 5) and the walks per block / per (block, candidate) (every mode)
static auto grid_list_kernel(const lp::GridPlan &p, int mode) {
  return mode == 0 ? (p.sampled ? k_grid_list<0, true> : k_grid_list<0>) : (mode == 4 ? k_grid_list<4> : k_grid_list<5>);
}
static auto grid_blocks_kernel(const lp::GridPlan &p, int mode) {
  if (mode == 0) {
    if (p.walk == lp::GridWalk::PER_CAND) return p.sampled ? k_grid_blocks<0, true, true> : k_grid_blocks<0, true>;
    return p.sampled ? k_grid_blocks<0, false, true> : k_grid_blocks<0, false>;
  }
  return mode == 1 ? k_grid_blocks<1, false>
                   : (mode == 2 ? k_grid_blocks<2, false>
                                : (mode == 3 ? k_grid_blocks<3, false> : (mode == 4 ? k_grid_blocks<4, false> : k_grid_blocks<5, false>)));
}
// k_g2p of a plan's material set (launch_plan.h: plan_g2p).
// __launch_bounds__(256, 2) only PERMITS 256 VGPRs; what decides the speed is whether the allocation stays <= 168, i.e.
// whether THREE workgroups fit a CU's register file (512 per SIMD lane): 168 VGPRs 0.303 ms, 180 VGPRs 0.347 ms on the same
// box (profiles/r03_b_ab_vgpr.txt).  Forcing the bound (256, 3) makes the ALL-material kernel spill (its scratch reloads
// wait on the prefetched records: vmcnt is shared and in-order) and costs the others 3 % (profiles/r03_h_ab_refactor.txt),
// so the budget is met by specialising instead and guarded by tests/test_kernel_budget_cpu.py:
// the kernel is instantiated per material SET (k_g2p.h: MATS): one material in the whole ctx (the benchmark configurations,
// most scene scripts) -> the kernel that carries only that material's constitutive code (sand: 2 833 instructions and 153
// VGPRs against 5 552 / 180 for all eight); no visco group -> the set without it (161 VGPRs: visco, with two eigen-solves
// and a matrix exponential, is what pushes the full kernel over the budget).
template <bool STORE_B, bool RIGID>
static auto g2p_kernel_of(lp::MatSet m) {
  constexpr uint32_t NO_VISCO = MAT_ALL & ~(1u << MPMHIP_VISCO);
  auto kern = m.kind == lp::MatSet::ALL ? k_g2p<256, 2, true, STORE_B, RIGID> : k_g2p<256, G2P_MIN_WAVES, true, STORE_B, RIGID, NO_VISCO>;
  if constexpr (!STORE_B)  // (the one-material kernels exist only without apic_b)
    if (m.kind == lp::MatSet::ONE) kern = one_material(m.bit, kern, [](auto b) { return k_g2p<256, G2P_MIN_WAVES, true, false, RIGID, b.value>; });
  return kern;
}
static auto g2p_kernel(const lp::G2PPlan &p) {
  return p.store_b ? (p.rigid ? g2p_kernel_of<true, true>(p.mats) : g2p_kernel_of<true, false>(p.mats))
                   : (p.rigid ? g2p_kernel_of<false, true>(p.mats) : g2p_kernel_of<false, false>(p.mats));
}
// k_g2p_packed: one-material instantiations only, none for visco (launch_plan.h: plan_g2p picks the walk for no other ctx)
static auto g2p_packed_kernel(const lp::G2PPlan &p) {
  decltype(&k_g2p_packed<256, G2P_MIN_WAVES, false, 1u << MPMHIP_SAND>) none = nullptr;
  return one_material<1u << MPMHIP_VISCO>(p.mats.bit, none, [](auto b) { return k_g2p_packed<256, G2P_MIN_WAVES, false, b.value>; });
}

static thread_local std::string g_create_error;

enum { PH_SORT = 0, PH_P2G = 1, PH_EXCH = 2, PH_GRID = 3, PH_G2P = 4, PH_COUNT = 5 };

// A ctx's device copies of its sampled level set's key frames (mpmhip_set_levelset_sdf, mpmhip2d_set_levelset_sdf), [count] floats
// each.  They live until the lattice's size changes, shapes replace the set, or the ctx goes; the ctx's LS.sdf points at them while
// the set is installed.
struct SdfFrames {
  DevBuf<float> frame[2];
  size_t count = 0;
  void release() {
    frame[0].reset(); frame[1].reset();
    count = 0;
  }
  // arrays for a set of n samples: a set of the installed one's size keeps its memory; any other takes S, which points into the old
  // arrays, down with them first.  The stream must be idle (kernels in flight read the arrays).
  hipError_t reserve(SdfDev &S, size_t n, bool two) {
    if (n != count) {
      release();
      memset(&S, 0, sizeof S);
      if (hipError_t e = frame[0].alloc(n); e != hipSuccess) return e;
      count = n;
    }
    return two && !frame[1] ? frame[1].alloc(n) : hipSuccess;
  }
};

// the lattice of a description (mpmhip_sdf_desc: D = 3, mpmhip2d_sdf_desc: D = 2) and its key frames as the kernels read them; a set
// in the plane has res[2] = 1.  `aligned` and `off` are left as they are: only the 3D grid pass knows them (sdf_install).
template <int D, class Desc>
static void sdf_fill(SdfDev &S, const Desc &d, const float *phi0, const float *phi1, float t0, float t1) {
  S.phi0 = phi0; S.phi1 = phi1;
  for (int k = 0; k < 3; k++) {
    S.res[k] = k < D ? d.res[k] : 1;
    if (k < D) S.origin[k] = d.origin[k];
  }
  S.spacing = d.spacing; S.inv_spacing = 1.0f / d.spacing;
  S.t0 = phi1 ? t0 : 0.0f; S.t1 = phi1 ? t1 : 1.0f;
}

// The container store of a resident asynchronous stepper (driver: async_api.h; kernels and layouts: k_async.h), for both ctx types.
// The payload of a container is a short list of LANES — bytes per container, the array, its compaction twin — so that growing,
// compacting and the snapshots loop over lanes instead of naming arrays: 3D {id 4 B, g 64 B, w 64 B}, 2D {rec 64 B}.
struct AsyncStore : AsyncStoreCount {
  struct Lane { size_t bytes = 0; DevBuf<uint8_t> a, b; };
  Lane lane[3];
  int n_lanes = 0;
  DevBuf<uint32_t> tag, tag2;
  DevBuf<unsigned long long> best, d_scan;  // one dedup word per creation id; the slots of the compaction's chained scan
  int64_t best_cap = 0;
  uint32_t scan_cap = 0, scan_epoch = 0;
  DevBuf<uint8_t> d_tbl;
  PinnedBuf<uint8_t> h_tbl_pin;  // four pinned images of the action table (as_upload_tbl)
  uint32_t pin_next = 0;
  DevBuf<uint32_t> d_rank;
  DevBuf<AsyncCounters> d_cnt;
  PinnedBuf<AsyncCounters> h_cnt;
  bool pending_counters = false;  // an advance left appends / frees on the device that the host has not folded in yet
  bool view = false;              // the ctx's particles are copies of the pools (load_pools), not new particles
  int64_t compactions = 0;

  // Every call below wants the device set and the ctx's stream idle.
  // an empty store for a block table of rank_of.size() blocks: whatever an earlier session left is released
  hipError_t reset(std::initializer_list<size_t> lane_bytes, const std::vector<uint32_t> &rank_of) {
    *this = AsyncStore();
    for (size_t b : lane_bytes) lane[n_lanes++].bytes = b;
    const size_t nblk = rank_of.size();
    hipError_t e = hipSuccess;
    auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    A(d_tbl.alloc(nblk)); A(d_rank.alloc(nblk)); A(d_cnt.alloc(1)); A(h_tbl_pin.alloc(4 * nblk)); A(h_cnt.alloc(1));
    if (e == hipSuccess) A(hipMemcpy(d_rank, rank_of.data(), sizeof(uint32_t) * nblk, hipMemcpyHostToDevice));
    if (e == hipSuccess) A(hipMemset(d_cnt, 0, sizeof(AsyncCounters)));
    return e;
  }
  hipError_t reserve(uint32_t need) {  // room for `need` containers in total; the containers in use stay
    if (need <= cap) return hipSuccess;
    const uint32_t ncap = grown(need), keep = std::min(size_ub, cap);
    hipError_t e = tag.regrow(keep, ncap, false);
    for (int l = 0; l < n_lanes && e == hipSuccess; l++) e = lane[l].a.regrow(keep * lane[l].bytes, ncap * lane[l].bytes, false);
    // (kernels walk [0, upper bound of the size): every tag behind the containers in use says FREE)
    if (e == hipSuccess) e = hipMemset(tag + keep, 0xFF, sizeof(uint32_t) * (size_t)(ncap - keep));
    drop_twins();  // (the compaction targets are re-allocated when a compaction runs)
    if (e == hipSuccess) cap = ncap;
    return e;
  }
  void drop_twins() {
    tag2.reset();
    for (int l = 0; l < n_lanes; l++) lane[l].b.reset();
  }
  hipError_t reserve_twins() {
    if (tag2) return hipSuccess;
    hipError_t e = tag2.alloc(cap);
    for (int l = 0; l < n_lanes && e == hipSuccess; l++) e = lane[l].b.alloc(cap * lane[l].bytes);
    if (e != hipSuccess) drop_twins();
    return e;
  }
  void swap_twins() {
    std::swap(tag, tag2);
    for (int l = 0; l < n_lanes; l++) std::swap(lane[l].a, lane[l].b);
  }
  // the containers of a snapshot blob <-> the store, section by section (snapshot_blob.h: LayoutStore — the tags, then lane after lane)
  hipError_t save(char *blob, const snap::LayoutStore &L) const {
    if (!fits(L) || L.tags.len > sizeof(uint32_t) * (size_t)size) return hipErrorInvalidValue;
    hipError_t e = L.tags.len ? hipMemcpy(blob + L.tags.off, tag, L.tags.len, hipMemcpyDeviceToHost) : hipSuccess;
    for (int l = 0; l < n_lanes && e == hipSuccess && L.lane[l].len; l++) e = hipMemcpy(blob + L.lane[l].off, lane[l].a, L.lane[l].len, hipMemcpyDeviceToHost);
    return e;
  }
  hipError_t load(const char *blob, const snap::LayoutStore &L) {  // (into a store reserved for them: it then holds exactly these, all counted live)
    const size_t n = L.tags.len / sizeof(uint32_t);
    if (!fits(L) || n > cap) return hipErrorInvalidValue;
    hipError_t e = hipMemset(tag, 0xFF, sizeof(uint32_t) * (size_t)cap);
    if (e == hipSuccess && n) e = hipMemcpy(tag, blob + L.tags.off, L.tags.len, hipMemcpyHostToDevice);
    for (int l = 0; l < n_lanes && e == hipSuccess && n; l++) e = hipMemcpy(lane[l].a, blob + L.lane[l].off, L.lane[l].len, hipMemcpyHostToDevice);
    AsyncCounters z;
    memset(&z, 0, sizeof z);
    z.size = (uint32_t)n;
    if (e == hipSuccess) e = hipMemcpy(d_cnt, &z, sizeof z, hipMemcpyHostToDevice);
    size = size_ub = live = (uint32_t)n;
    pending_counters = false; view = false;
    return e;
  }
  bool fits(const snap::LayoutStore &L) const {  // the layout's lanes are this store's, for one number of containers
    bool ok = L.n_lanes == n_lanes;
    for (int l = 0; l < n_lanes && ok; l++) ok = L.lane[l].len == lane[l].bytes * (L.tags.len / sizeof(uint32_t));
    return ok;
  }
};
// what both ctx types keep for the asynchronous stepper: the block scheduler (async_sched.h), the reduction table of
// update_dt_limits with its pinned image, the pool block of every particle of a view, and the store
struct AsyncResident : AsyncSched {
  bool resident = false;
  DevBuf<uint32_t> d_tab, d_blk_of;
  int64_t blk_of_cap = 0;
  PinnedBuf<uint32_t> h_tab;
  size_t h_tab_cap = 0;
  AsyncStore store;
  int32_t forms[4] = {-1, -1, -1, -1};  // {gather, file, load, export} of the latest launch: 0 by arrival, 1 ordered (mpmhip_async_forms)
  uint32_t test_wgs = 0;                // TEST KNOB (env MPMHIP_ASYNC_WGS, results valid): workgroups of every asynchronous launch at most; 0 = off
};

struct mpmhip_ctx {
  mpmhip_config cfg;
  Params P;
  int device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  std::string err;
  // particles
  int64_t cap = 0;
  int64_t n_slots = 0;  // slots in use (live + deleted)
  int32_t next_pid = 0;
  DevBuf<RecG> rg, rg2;
  DevBuf<RecP> rp, rp2;
  DevBuf<float> rb, rb2;
  DevBuf<uint32_t> key, rank, perm;
  // blocks
  uint32_t NB = 0;
  DevBuf<uint8_t> blk_flag;
  DevBuf<uint32_t> bits, wprefix, act_blk, act_start;
  DevBuf<uint32_t> cell_cnt, cell_start, fat_slot;
  bool deterministic = false;  // mpmhip_config.deterministic (env MPMHIP_DETERMINISTIC): in-cell order by creation id behind every sort (do_sort)
  DevBuf<uint32_t> cellcnt_key;  // [64 NB] cell counters indexed by KEY (Morton block << 6 | cell): the two-launch front of the sort (do_sort); nullptr on grids beyond 2^21 blocks
  DevBuf<uint32_t> nbr, own_list;  // k_cell_table -> k_grid: 32-word neighbour row per active block, list of owned (block, candidate) pairs
  FillStats *d_stats = nullptr;  // device address of the pinned page's statistics words (h_pinned + FILL_STATS_WORD): k_cell_table stores there
  lp::Knobs knobs;               // the tuning switches of the substep path (launch_plan.h), read from the environment by mpmhip_create
  bool list_valid = false;       // the last sort built neighbour rows + owner list (do_sort -> do_grid)
  struct LastSort {              // what the last do_sort launched (mpmhip_debug_sort_info: the tests of the sort's tables)
    bool keyed = false, build_list = false, ids_cached = false, deterministic = false;
    int ct = 0, cell_order_form = 0;
  } last_sort;
  DevBuf<unsigned long long> scan_slots;  // [256] k_block_table + [ct_grid] k_cell_table: {epoch, chunk sum}
  uint32_t list_clear_epoch = 0;  // sort epoch at which the scan words of the list form of k_cell_table were last zeroed (do_sort)
  uint32_t sort_epoch = 0, bt_slots = 0, ct_slots = 0;  // scan_slots: [bt_slots] k_block_table | [ct_slots] k_cell_table_plain | [ct_slots] k_cell_table
  uint32_t scan_grid = 256;  // workgroups of the single-pass scan kernels: three eighths of what the device keeps resident (the lowest
                             // of the plain kernels; scan_limit() answers per kernel)
  std::map<const void *, uint32_t> scan_limits;  // kernel -> three eighths of its resident workgroups
  DevBuf<float4> tiles, gridv, dense;
  DevBuf<Counters> cnt;
  std::vector<GroupParams> groups;
  DevBuf<GroupParams> d_groups;
  int groups_cap = G2P_LDS_GROUPS;  // k_g2p mirrors the whole table in LDS
  RecordState rec;            // which arrays describe the current particles (record_state.h)
  DevBuf<uint32_t> pidc;      // creation id per slot beside key[] (Params::pidc points here while the deterministic mode is on)
  int n_cus = 256;            // compute units of the device
  DevBuf<uint32_t> chunk_blk;  // per 256 positions of the sorted index: the block holding the first (k_cell_table -> k_g2p_packed)
  int reorder_interval = 0;   // physical reorder every this many substeps (0 = never); env MPMHIP_REORDER_INTERVAL
  float t = 0.0f, request_t = 0.0f;  // `real` accumulators, as in the reference (src/mpm.h:99, mpm.cpp:573)
  int64_t substeps = 0;
  // profiling
  int profiling = 0;  // 0 off, 1 every phase, 2 only G2P, 3 only P2G (two events per substep instead of six),
                      // 4 the parts of a tiled substep: begin / interior / end, nothing recorded INSIDE a part
  struct Ev { hipEvent_t e[PH_COUNT + 1]; bool ov; };  // ov: the substep ran split (boundary / interior)
  std::vector<Ev> ev_pool;
  size_t ev_used = 0;
  double phase_ms[PH_COUNT] = {0, 0, 0, 0, 0};
  int64_t prof_substeps = 0;
  int ev_level = 0;  // level the pooled events were recorded with
  int prof_every = 1;  // levels 2 / 3: bracket the kernel in every prof_every-th substep only (mpmhip_set_profile_sampling)
  Ev *cur_ev = nullptr;  // events of the substep between substep_begin and substep_end
  // tiling
  LevelSetDev LS;
  DevBuf<LevelSetDev> d_LS;  // device copy for k_g2p (k_grid takes it by value)
  SdfFrames sdf;            // mpmhip_set_levelset_sdf / _mesh: the installed sampled level set's key frames
  SeedWork seed;            // mpmhip_seed_particles: the tile and the work buffers, kept between calls (seed_api.h)
  MeshSdfWork mesh_work[2];  // mpmhip_set_levelset_mesh: the voxeliser's buffers per key frame, kept between calls
  int particle_collision_cfg = 0;  // the config's particle_collision.  P.particle_collision is 0 while a sampled set is installed:
                                   // the G2P kernels then leave the push to k_sdf_collide (do_sdf_collide)
  Tiling T;
  DevBuf<DevBox> d_boxes;
  DevBuf<uint32_t> d_counts;
  DevBuf<int> d_bounds;
  DevBuf<unsigned long long> d_live_hist;  // mpmhip_live_histogram: rows | total | bounds (res0 + res1 + res2 + 4 words: fixed for the ctx)
  PinnedBuf<uint32_t> h_pinned;  // 64 KiB of pinned host memory for small readbacks (counters, migration table)
  static constexpr int FILL_STATS_WORD = 16368;  // word offset of the block-fill statistics in that page (do_sort, facts)
  DevBuf<double> d_energy;
  DevBuf<double> d_energy_parts;  // deterministic mode: [8 energy_parts_cap + POT_WAVES] the partial sums of calculate_energy (energy_end_det)
  size_t energy_parts_cap = 0;
  int counts_cap = 0;
  bool compact_requested = false;
  bool in_substep = false;
  struct AsyncState : AsyncResident {  // + the first half (mpmhip_async_enable), the frame's `limit` attribute, the profile
    bool enabled = false, limits_valid = false;
    DevBuf<int32_t> d_blk_limits, d_particle_limits;
    double prof_ms[6] = {0, 0, 0, 0, 0, 0};
    bool profile_sync = false;
  } async;
  int64_t host_particle_bytes = 0;  // particle data copied between host and device so far (uploads, downloads, snapshots)
  // CPIC rigid coupling (rigid_api.h): bodies 1.. (0 = background), their boundary particles, the colored distance field
  struct RigidState {
    bool enabled = false;
    rigid_setup::Store<3> store;  // the bodies' host records, boundary particles (+ creation ids) and elements
    DevBuf<RigidBodyDev> d_rb;
    DevBuf<RigidSample> d_smp;
    DevBuf<float> d_elems;
    uint32_t n_smp = 0;
    CdfDev cdf{};  // what the kernels take by value: slot / page_key / mind / tags / rpage point into the five arrays below (rigid_enable)
    DevBuf<uint32_t> cdf_slot, cdf_page_key, cdf_tags, cdf_rpage;
    DevBuf<unsigned long long> cdf_mind;
    DevBuf<BndRec> d_bnd;
    DevBuf<uint8_t> d_blk_rigid;
    hipStream_t side = nullptr;          // the colour-aware transfer kernels run here, next to the plain ones on the ctx stream
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    DevBuf<uint32_t> d_rigid_list;  // [max_blocks + 1] the flagged blocks as a list; its length is d_counters[CDF_POOLS + 1]
    DevBuf<float> d_imp_rows;       // deterministic mode only: [imp_rows_cap][IMP_ROW] per flagged block its impulse sums (k_rigid.h)
    size_t imp_rows_cap = 0;
    DevBuf<uint32_t> d_counters;  // [0, CDF_POOLS) pages handed out per sub-pool, [CDF_POOLS] cutting_counter
    uint32_t max_pages = 0;
    uint32_t gather_epoch = 0;  // stamps the boundary records of the particles the last gather_cdf visited
    size_t rpage_words = 0;
    float penalty = 0.0f, pushing_force = 20000.0f;  // MPM::initialize defaults, src/mpm.cpp:35,40
    bool ls_collision = false;       // config key rigid_body_levelset_collision (src/mpm.cpp:535-538)
    DevBuf<uint32_t> d_smp_rank;  // position of every boundary particle in the reference's sorted particle list (among the boundary particles)
    uint32_t n_ranked = 0, ls_cap = 0;
    DevBuf<unsigned long long> d_ls_keys[2];
    DevBuf<uint32_t> d_ls_vals[2];
    DevBuf<uint8_t> d_ls_tmp;
    size_t ls_tmp_bytes = 0;
    std::vector<JointDev> joints;    // MPM::articulations, in the order they were added
    DevBuf<JointDev> d_joints;
    int joint_iterations = 100;      // 'articulation_iterations' (src/mpm.h:279-280)
    // rigid-rigid collisions (MPM::rigidify; rigid_collide_api.h): opt-in, the device arrays come with the first run
    struct Collide {
      bool on = false;                 // config key rigid_body_collision
      int iterations = 5;              // rigid_body_iterations
      float penalty = 1e3f;            // rigid_penalty
      bool position_iterations = true; // rigid_body_position_iterations
      size_t n_verts = 0;              // what the arrays below were built for
      int n_bodies = 0;
      DevBuf<int> d_body, d_first, d_count;  // per hull vertex its body; per body its vertices in RigidState::d_elems
      DevBuf<float4> d_r, d_p;               // per hull vertex R v and R v + pos of this substep
      DevBuf<float> d_ctr;
      DevBuf<MprPair> d_pairs;
      DevBuf<RigidCollision> d_cols, d_hits; // per pair what the MPR found; the hits in (i, j) order
      DevBuf<int> d_nhits;
    } col;
  } rigid;
  bool overlap = false;        // mpmhip_set_overlap: split tiled substeps into boundary / interior work
  bool ov_active = false, interior_done = false;  // state of the substep in flight
  const DevBox *d_boxes_cur = nullptr;  // the box table the pack / grid kernels of the substep in flight read
  bool dirichlet = false;      // mpmhip_set_dirichlet
  // the native data plane of a tiled run (tiled_api.h): plan, arena, wire, migration state
  struct TiledNative {
    struct Peer {  // a rank's arena as THIS process addresses it
      uint32_t *flags = nullptr, *table[2] = {nullptr, nullptr};
      float4 *recv[2] = {nullptr, nullptr}, *inbox = nullptr;
      double *red[2] = {nullptr, nullptr};  // reduction tables (tiled_api.h: tn_reduce_*)
      void *ipc_base = nullptr;  // mapped with hipIpcOpenMemHandle (closed on destroy)
      uint8_t handle[MPMHIP_IPC_HANDLE_BYTES] = {};  // the handle ipc_base was opened from
    };
    tplan::Mig mig;        // the migration table of the migration in flight, decoded
    bool on = false, connected = false, exch_on_side = false;
    bool defer_signal = false, signal_deferred = false;  // local job: the ranks' epochs are published by ONE launch of the group (tiled_api.h)
    bool loop_rccl = false;               // MPMHIP_WIRE_LOCAL_RCCL: a local job whose halo boxes travel by RCCL self-sends (tiled_api.h)
    std::vector<mpmhip_ctx *> local_ctx;  // the ranks of a local job (mpmhip_tiled_connect_local)
    bool wait_merged = false;  // IPC wire, no overlap split: signal + wait of a substep in one launch
    int world = 1, wire = 0;
    int clip_lo[3] = {0, 0, 0}, clip_hi[3] = {0, 0, 0};
    std::vector<int> occ;  // [world][6]: every rank's occupancy box (lo3, hi3, nodes): node_box(r) is cut to it (tiled_plan.h: plan)
    bool occ_valid = false, initial_scan = false;  // (until the scan in front of the first substep: the global clip box only)
    tplan::Plan plan;       // this rank's halo boxes
    tplan::Arena lay;       // the layout of every rank's arena, with the two capacities it was computed from
    std::vector<int> halo_peers, all_ranks;
    size_t mig_send_cap = 0;
    char *arena = nullptr;  // raw on purpose: one of two allocation calls, mapped by other processes; released in tn_free
    uint8_t handle[MPMHIP_IPC_HANDLE_BYTES] = {};  // the arena's IPC handle, made once per arena (mpmhip_tiled_ipc_handle)
    bool handle_valid = false;
    uint32_t *flags = nullptr, *table[2] = {nullptr, nullptr};             // views into the arena
    float4 *recv[2] = {nullptr, nullptr}, *inbox = nullptr;  // ditto
    DevBuf<uint32_t> row, d_done, d_recut;  // (d_recut: cursors and quota ends of a redistribution round's pack)
    DevBuf<float4> send, mig_send;
    DevBuf<DevBox> d_boxes[2];
    DevBuf<int> d_halo_idx, d_all_idx;
    std::vector<Peer> peers;
    uint32_t epoch = 0, mig_epoch = 0, red_epoch = 0;
    DevBuf<double> d_red;  // this rank's row of a reduction (+ room for the all-reduced row)
    unsigned long long timeout_ticks = 2000000000ull;  // of the 100 MHz wall clock
    void *comm = nullptr;  // ncclComm_t
    int comm_rank = 0, comm_world = 1;
    hipStream_t side = nullptr;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    int64_t k = 0, next_migration = 0, migrated_out = 0, migrations = 0, replans = 0;
    int migrate_interval = 4, adaptive_cap = 64;
    // CPIC rigid bodies on the job (tiled_plan.h: impulse rows): set by mpmhip_tiled_setup on a ctx that holds bodies
    bool rows = false;
    bool defer_finish = false;        // mpmhip_tiled_advance_group: substep_end stops behind G2P, the group finishes every rank
    uint32_t row_epoch[tplan::ROW_EXCHANGES] = {0, 0};
    DevBuf<float> d_row_stage;        // the RCCL wires send the row from here
  } tn;
  bool rows_substep = false;  // the substep in flight hands its impulse rows to the job instead of applying them (tn.rows)
};
namespace {
void tn_free(mpmhip_ctx *c);
void tn_begin_substep(mpmhip_ctx *c);
int tn_row_out(mpmhip_ctx *c, int exchange);
int tn_rows_apply(mpmhip_ctx *c, int exchange);
}

// what Params mirrors of the ctx: the slot count, and the id cache beside key[] while the deterministic mode is on
static void set_slots(mpmhip_ctx *c, int64_t n) {
  c->n_slots = n;
  c->P.n_slots = (uint32_t)n;
}
static void sync_pidc(mpmhip_ctx *c) { c->P.pidc = c->deterministic ? c->pidc.get() : nullptr; }

static int fail(mpmhip_ctx *c, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_create_error = buf;
  return code;
}

#define HIPCHK(c, call)                                                                      \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) return fail((c), MPMHIP_EHIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

static int particle_grid(int64_t n) {
  int64_t b = (n + 255) / 256;
  if (b < 1) b = 1;
  if (b > 8192) b = 8192;
  return (int)b;
}

static int launch_check(mpmhip_ctx *c, const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, MPMHIP_EHIP, "launch of %s failed: %s", what, hipGetErrorString(e));
  return MPMHIP_OK;
}

template <typename K, typename... Args>
static int run_debug(mpmhip_ctx *c, K kernel, Args... args) {
  hipLaunchKernelGGL(kernel, dim3(256), dim3(256), 0, c->stream, args...);
  int rc = launch_check(c, "debug kernel");
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MPMHIP_OK;
}

// ---------------------------------------------------------------------------------------------- .bgeo frames
// Houdini .bgeo v5 as Partio writes it (external/partio/src/io/BGEO.cpp:57-194) with write_partio's attribute table
// (src/visualize.cpp:24-38).  Big-endian throughout.
namespace {
struct BgeoAttr { const char *name; uint16_t count; int32_t houdini_type; };  // 0 float, 1 int, 5 vector
const BgeoAttr BGEO_PLAIN[] = {{"type", 1, 1}, {"index", 1, 1}, {"limit", 3, 1}, {"v", 3, 5}};
const BgeoAttr BGEO_VERBOSE[] = {{"m", 1, 5}, {"boundary_normal", 3, 5}, {"debug", 3, 5}, {"states", 1, 1},
                                 {"boundary_distance", 1, 0}, {"near_boundary", 1, 1}, {"apic_frobenius_norm", 1, 0}};
void put32(std::vector<uint8_t> &o, uint32_t v) { for (int s = 24; s >= 0; s -= 8) o.push_back((uint8_t)(v >> s)); }
void put16(std::vector<uint8_t> &o, uint16_t v) { o.push_back((uint8_t)(v >> 8)); o.push_back((uint8_t)v); }
void put_str(std::vector<uint8_t> &o, const char *s) {
  const size_t n = std::strlen(s);
  put16(o, (uint16_t)n);
  o.insert(o.end(), s, s + n);
}
std::vector<uint8_t> bgeo_header(uint32_t n, bool verbose) {
  std::vector<uint8_t> o;
  put32(o, 0x4267656fu);  // "Bgeo"
  o.push_back('V');
  put32(o, 5);
  put32(o, n); put32(o, 1); put32(o, 0);  // points, one primitive, point groups
  put32(o, 0); put32(o, verbose ? 11 : 4); put32(o, 0); put32(o, 1); put32(o, 0);  // prim groups, point / vertex / prim / detail attributes
  auto table = [&](const BgeoAttr *a, int m) {
    for (int i = 0; i < m; i++) {
      put_str(o, a[i].name);
      put16(o, a[i].count);
      put32(o, (uint32_t)a[i].houdini_type);
      for (int k = 0; k < a[i].count; k++) put32(o, 0);  // defaults
    }
  };
  table(BGEO_PLAIN, 4);
  if (verbose) table(BGEO_VERBOSE, 7);
  return o;
}
std::vector<uint8_t> bgeo_prim_attr() {  // the "generator" = "papi" primitive attribute and the primitive's head
  std::vector<uint8_t> o;
  put_str(o, "generator");
  put16(o, 1); put32(o, 4); put32(o, 1);
  put_str(o, "papi");
  put32(o, 0x8000);
  return o;
}
// what follows the rows: the primitive attribute, the particle system's point numbers and the file's end
size_t bgeo_tail_bytes(uint32_t n) { return bgeo_prim_attr().size() + 4 + (size_t)n * (n > (1u << 16) ? 4 : 2) + 4 + 2; }
uint8_t *bgeo_put_tail(uint8_t *out, uint32_t n) {
  const std::vector<uint8_t> prim = bgeo_prim_attr();
  std::memcpy(out, prim.data(), prim.size());
  out += prim.size();
  auto w32 = [&](uint32_t v) { for (int s = 24; s >= 0; s -= 8) *out++ = (uint8_t)(v >> s); };
  w32(n);
  if (n > (1u << 16)) {  // BGEO.cpp:175-180: point numbers as int32 above 65536 points, uint16 otherwise
    for (uint32_t i = 0; i < n; i++) w32(i);
  } else {
    for (uint32_t i = 0; i < n; i++) { *out++ = (uint8_t)(i >> 8); *out++ = (uint8_t)i; }
  }
  w32(0);
  *out++ = 0x00;
  *out++ = 0xff;
  return out;
}
size_t bgeo_bytes(uint32_t n, bool verbose) {
  const size_t w = verbose ? BGEO_W_VERBOSE : BGEO_W_PLAIN;
  return bgeo_header(n, verbose).size() + (size_t)n * w * 4 + bgeo_tail_bytes(n);
}
}  // namespace

// live particles in ascending creation id (write_partio sorts by id, src/visualize.cpp:39-43) -> slot list
static int bgeo_order(mpmhip_ctx *c, std::vector<uint32_t> &order, std::vector<int32_t> *ids_out = nullptr) {
  order.clear();
  const size_t ns = (size_t)c->n_slots;
  if (!ns) return MPMHIP_OK;
  DevBuf<int32_t> d_ids;
  HIPCHK(c, d_ids.alloc(ns));
  hipLaunchKernelGGL(k_bgeo_ids, dim3(particle_grid(c->n_slots)), dim3(256), 0, c->stream, c->P, (const RecG *)c->rg, d_ids);
  std::vector<int32_t> ids(ns);
  HIPCHK(c, hipMemcpyAsync(ids.data(), d_ids, ns * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  order.reserve(ns);
  bool ascending = true;
  int32_t last = -1, max_id = -1;
  for (size_t s = 0; s < ns; s++) {
    if (ids[s] < 0) continue;
    order.push_back((uint32_t)s);
    ascending = ascending && ids[s] > last;
    last = ids[s];
    max_id = std::max(max_id, ids[s]);
  }
  auto finish = [&]() { if (ids_out) { ids_out->resize(order.size()); for (size_t j = 0; j < order.size(); j++) (*ids_out)[j] = ids[order[j]]; } return MPMHIP_OK; };
  if (ascending) return finish();  // slots are handed out in creation order: true until the first physical reorder
  if ((size_t)max_id < 16 * order.size() + 1024) {  // ids are unique: a direct table, swept in id order
    std::vector<uint32_t> slot_of(max_id + 1, 0xFFFFFFFFu);
    for (uint32_t s : order) slot_of[ids[s]] = s;
    size_t m = 0;
    for (uint32_t s : slot_of)
      if (s != 0xFFFFFFFFu) order[m++] = s;
  } else {
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return ids[a] < ids[b]; });
  }
  return finish();
}

extern "C" {

static uint32_t scan_limit(mpmhip_ctx *c, const void *kernel);   // (defined with do_sort, below)

uint32_t mpmhip_abi_version(void) { return MPMHIP_ABI_VERSION; }

const char *mpmhip_last_error(const mpmhip_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int mpmhip_create(const mpmhip_config *cfg, mpmhip_ctx **out) {
  if (!cfg || !out) return fail(nullptr, MPMHIP_EINVAL, "null argument");
  *out = nullptr;
  for (int k = 0; k < 3; k++)
    if (cfg->res[k] < 8 || cfg->res[k] > 1000) return fail(nullptr, MPMHIP_EINVAL, "res[%d]=%d outside [8,1000]", k, cfg->res[k]);
  if (!(cfg->dx > 0) || !(cfg->dt >= 0)) return fail(nullptr, MPMHIP_EINVAL, "dx must be > 0 and dt >= 0");
  if (cfg->max_particles <= 0 || cfg->max_particles >= (1ll << 31)) return fail(nullptr, MPMHIP_EINVAL, "max_particles out of range");
  if (cfg->n_planes < 0 || cfg->n_planes > 8) return fail(nullptr, MPMHIP_EINVAL, "n_planes out of range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, MPMHIP_EHIP, "no HIP device available (libmpmhip has no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, MPMHIP_EINVAL, "device %d of %d", cfg->device, ndev);
  mpmhip_ctx *c = new (std::nothrow) mpmhip_ctx();
  if (!c) return fail(nullptr, MPMHIP_ENOMEM, "host allocation failed");
  c->cfg = *cfg;
  c->device = cfg->device;
  c->knobs = lp::Knobs::from_env();
  c->reorder_interval = cfg->reorder_interval;
  if (const char *e = getenv("MPMHIP_REORDER_INTERVAL")) c->reorder_interval = atoi(e);
  c->deterministic = cfg->deterministic != 0;
  if (const char *e = getenv("MPMHIP_DETERMINISTIC")) c->deterministic = atoi(e) != 0;
  auto bail = [&](int code) { g_create_error = c->err; mpmhip_destroy(c); return code; };
  if (hipSetDevice(c->device) != hipSuccess) { fail(c, MPMHIP_EHIP, "hipSetDevice failed"); return bail(MPMHIP_EHIP); }
  Params &P = c->P;
  memset(&P, 0, sizeof P);
  memset(&c->T, 0, sizeof c->T);
  int maxnb = 0;
  for (int k = 0; k < 3; k++) {
    P.res[k] = cfg->res[k];
    P.g[k] = cfg->gravity[k];
    int nb = (cfg->res[k] + 1 + BS - 1) / BS + 1;
    if (nb > maxnb) maxnb = nb;
  }
  P.dx = cfg->dx; P.idx = 1.0f / cfg->dx; P.dt = cfg->dt;
  P.particle_gravity = cfg->particle_gravity; P.apic_damping = cfg->apic_damping; P.rpic_damping = cfg->rpic_damping;
  P.clean_boundary = cfg->clean_boundary;
  P.store_b = cfg->discard_apic_b ? 0 : 1;
  P.clamp_pos = cfg->generic_path ? 1 : 0;
  P.test_small_rank = getenv("MPMHIP_TEST_SMALL_RANK") ? atoi(getenv("MPMHIP_TEST_SMALL_RANK")) : 0;
  memset(&c->LS, 0, sizeof c->LS);
  c->LS.particle_collision = cfg->particle_collision;
  P.particle_collision = cfg->particle_collision;
  c->particle_collision_cfg = cfg->particle_collision;
  if (mpmhip_set_levelset(c, cfg->n_planes, &cfg->planes[0][0], cfg->friction) != MPMHIP_OK) return bail(MPMHIP_EINVAL);
  int kbits = 1;
  while ((1 << kbits) < maxnb) kbits++;
  if (kbits > 8) { fail(c, MPMHIP_EINVAL, "grid too large for 32-bit keys"); return bail(MPMHIP_EINVAL); }
  P.kbits = kbits;
  c->NB = 1u << (3 * kbits);
  P.nbw = c->NB / 32u;
  if (P.nbw == 0) P.nbw = 1;
  c->cap = cfg->max_particles;
  int64_t mb = cfg->max_blocks;
  if (mb <= 0) mb = c->cap / 48 + 4096;  // a block of 64 cells at >= ~1 particle/cell on average, plus slack
  if (mb > (int64_t)c->NB) mb = c->NB;
  P.max_blocks = (uint32_t)mb;

  hipError_t e = hipSuccess;
  auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  A(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
  c->stream = c->own_stream;
  A(c->rg.alloc((size_t)c->cap));
  A(c->rp.alloc((size_t)c->cap));
  A(c->rb.alloc((size_t)c->cap * BW));
  A(c->rg2.alloc((size_t)c->cap));  // k_g2p writes the updated records here, at their sorted positions; the two sets swap
  A(c->rp2.alloc((size_t)c->cap));
  A(c->rb2.alloc((size_t)c->cap * BW));
  A(c->key.alloc((size_t)c->cap));
  A(c->pidc.alloc((size_t)c->cap));
  A(c->rank.alloc((size_t)c->cap));
  A(c->perm.alloc((size_t)c->cap));
  A(c->chunk_blk.alloc((size_t)c->cap / 256 + 2));
  A(c->bits.alloc((size_t)P.nbw));
  A(c->blk_flag.alloc((size_t)P.nbw * 32));
  A(c->wprefix.alloc((size_t)P.nbw));
  A(c->fat_slot.alloc((size_t)c->NB));
  A(c->act_blk.alloc((size_t)mb + 1));
  A(c->act_start.alloc((size_t)mb + 2));
  A(c->cell_cnt.alloc((size_t)mb * BC));
  A(c->cell_start.alloc((size_t)mb * BC + 1));
  // key-indexed cell counters (256 B per block of the WHOLE block space: 67 MB at 128^3, 537 MB at 256^3..508^3): with them the ranks
  // need no block table and share a launch with it (k_sort_front); grids of 2^24 blocks (res > 508) keep the four-launch sort
  // (MPMHIP_SORT_V1, A/B and tests: the four launches)
  const bool want_keyed = c->NB <= lp::KEYED_MAX_BLOCK_SPACE && !c->knobs.sort_v1;  // (the table itself is allocated behind every other buffer, below)
  A(c->nbr.alloc((size_t)mb * 32));
  A(c->own_list.alloc((size_t)mb * 8));
  c->bt_slots = (P.nbw + 255) / 256;
  c->ct_slots = (uint32_t)(((size_t)mb + 15) / 16 + 1);  // k_cell_table chunks are >= 16 blocks
  const size_t n_slots64 = c->bt_slots + 2 * (size_t)c->ct_slots;
  A(c->scan_slots.alloc(n_slots64));
  A(c->tiles.alloc((size_t)mb * TN));
  A(c->gridv.alloc((size_t)mb * 8 * BC));
  A(c->cnt.alloc(1));
  A(c->d_LS.alloc(1));
  A(c->h_pinned.alloc(65536 / sizeof(uint32_t)));
  if (e == hipSuccess && c->h_pinned) memset(c->h_pinned, 0, 65536);
  if (e == hipSuccess) {
    void *dp = nullptr;
    A(hipHostGetDevicePointer(&dp, c->h_pinned, 0));
    c->d_stats = reinterpret_cast<FillStats *>(reinterpret_cast<uint32_t *>(dp) + mpmhip_ctx::FILL_STATS_WORD);
  }
  A(c->d_groups.alloc((size_t)c->groups_cap));
  if (e == hipSuccess && want_keyed) {
    // (an optimisation's table, 256 B per block of the whole block space: 67 MB at 128^3, 537 MB from 256^3 to 508^3.  A device that
    // cannot spare it keeps the four-launch sort instead of failing the create — or a later mpmhip_reserve, a tiled arena, the next
    // rank sharing the device: the table is only taken while it is at most an eighth of what is free NOW, behind every other buffer)
    size_t free_b = 0, total_b = 0;
    const size_t table_b = (size_t)c->NB * BC * sizeof(uint32_t);
    const bool room = hipMemGetInfo(&free_b, &total_b) == hipSuccess && table_b <= free_b / 8;
    if (!room || c->cellcnt_key.alloc((size_t)c->NB * BC) != hipSuccess) (void)hipGetLastError();
  }
  if (e != hipSuccess) {
    fail(c, MPMHIP_ENOMEM, "device allocation failed: %s (max_particles=%lld, max_blocks=%lld)", hipGetErrorString(e),
         (long long)c->cap, (long long)mb);
    return bail(MPMHIP_ENOMEM);
  }
  sync_pidc(c);
  A(hipMemset(c->bits, 0, sizeof(uint32_t) * P.nbw));
  A(hipMemset(c->blk_flag, 0, (size_t)P.nbw * 32));
  A(hipMemset(c->cell_cnt, 0, sizeof(uint32_t) * (size_t)mb * BC));
  if (c->cellcnt_key) A(hipMemset(c->cellcnt_key, 0, sizeof(uint32_t) * (size_t)c->NB * BC));
  A(hipMemset(c->cell_start, 0, sizeof(uint32_t) * ((size_t)mb * BC + 1)));
  A(hipMemset(c->act_start, 0, sizeof(uint32_t) * ((size_t)mb + 2)));
  A(hipMemset(c->cnt, 0, sizeof(Counters)));
  A(hipMemcpy(c->d_LS, &c->LS, sizeof c->LS, hipMemcpyHostToDevice));
  A(hipMemset(c->scan_slots, 0, sizeof(unsigned long long) * n_slots64));  // epoch 0 is never used
  A(hipMemset(c->fat_slot, 0, sizeof(uint32_t) * (size_t)c->NB));
  A(hipMemset(c->rb, 0, sizeof(float) * (size_t)c->cap * BW));
  {  // the single-pass scans spin on their predecessors: their grids must fit on the device all at once (k_sort.h)
    int cus = 0;
    A(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    if (cus > 0) c->n_cus = cus;
  }
  A(hipDeviceSynchronize());
  if (e != hipSuccess) { fail(c, MPMHIP_EHIP, "device init failed: %s", hipGetErrorString(e)); return bail(MPMHIP_EHIP); }
  // every chained scan this ctx can launch (k_sort.h; the block-table role of k_sort_front included: its workgroups are the first of
  // their launch): the grid the host will use must lie inside the set the device certainly keeps resident — asked of the occupancy
  // API once, here, instead of being assumed at the first sort.  (The waits are bounded on top of it: k_sort.h.)
  {
#define MPM_CT_ALL(K) (const void *)K<16, false>, (const void *)K<32, false>, (const void *)K<64, false>, (const void *)K<16, true>, (const void *)K<32, true>, (const void *)K<64, true>
    const void *scans[] = {(const void *)k_sort_front, (const void *)k_block_table, MPM_CT_ALL(k_cell_table), MPM_CT_ALL(k_cell_table_plain),
                           (const void *)k_async_compact<Store3>, (const void *)k_async_gather_ordered<Work3>,
                           (const void *)k_async_file_ordered<Work3>, (const void *)k_async_load_ordered<Work3>,
                           (const void *)k_async_export_ordered<Store3>};
#undef MPM_CT_ALL
    for (const void *k : scans) {
      int per_cu = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, 256, 0) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        fail(c, MPMHIP_EHIP, "the occupancy query of a chained-scan kernel failed: its launch cannot be sized safely");
        return bail(MPMHIP_EHIP);
      }
      if (scan_limit(c, k) > lp::scan_resident_set(c->n_cus, per_cu)) {
        fail(c, MPMHIP_EINVAL, "a chained scan would be launched with %u workgroups, the device keeps %u resident (MPMHIP_SCAN_GRID=%d?)",
             scan_limit(c, k), lp::scan_resident_set(c->n_cus, per_cu), c->knobs.scan_grid);
        return bail(MPMHIP_EINVAL);
      }
    }
  }
  *out = c;
  return MPMHIP_OK;
}

void mpmhip_destroy(mpmhip_ctx *c) {
  if (!c) return;
  hipSetDevice(c->device);
  if (c->own_stream) hipStreamSynchronize(c->own_stream);
  for (auto &ev : c->ev_pool)
    for (int k = 0; k <= PH_COUNT; k++) hipEventDestroy(ev.e[k]);
  { auto &R = c->rigid; if (R.side) { hipStreamSynchronize(R.side); hipStreamDestroy(R.side); } if (R.ev_fork) hipEventDestroy(R.ev_fork); if (R.ev_join) hipEventDestroy(R.ev_join); }
  tn_free(c);
  if (c->own_stream) hipStreamDestroy(c->own_stream);
  delete c;  // (the members free their arrays on the device set above)
}

int mpmhip_set_stream(mpmhip_ctx *c, void *s) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return MPMHIP_OK;
}

int mpmhip_set_deterministic(mpmhip_ctx *c, int32_t enabled) {
  if (!c) return MPMHIP_EINVAL;
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "set_deterministic inside a substep");
  c->deterministic = enabled != 0;
  sync_pidc(c);  // (the key writers keep the ids beside the keys from now on; until a G2P has, k_cell_order reads the records)
  c->rec.id_cache_dropped();
  return MPMHIP_OK;
}

int mpmhip_set_dirichlet(mpmhip_ctx *c, int32_t enabled) {
  if (!c) return MPMHIP_EINVAL;
  c->dirichlet = enabled != 0;
  return MPMHIP_OK;
}

static void sdf_release(mpmhip_ctx *c) {
  c->sdf.release();
  memset(&c->LS.sdf, 0, sizeof c->LS.sdf);
  c->P.particle_collision = c->particle_collision_cfg;
}

static int check_shapes(mpmhip_ctx *c, int32_t n, const mpmhip_shape *shapes) {
  if (n < 0 || n > MPMHIP_MAX_SHAPES || (n > 0 && !shapes)) return fail(c, MPMHIP_EINVAL, "between 0 and %d level-set shapes", MPMHIP_MAX_SHAPES);
  for (int i = 0; i < n; i++) {
    if (shapes[i].type < 0 || shapes[i].type > 2) return fail(c, MPMHIP_EINVAL, "shape %d: unknown type %d", i, shapes[i].type);
    if (shapes[i].type == 1 && !(shapes[i].p[3] > 0)) return fail(c, MPMHIP_EINVAL, "shape %d: sphere radius must be > 0", i);
    if (shapes[i].type == 2)
      for (int k = 0; k < 3; k++)
        if (!(shapes[i].p[k] < shapes[i].p[3 + k])) return fail(c, MPMHIP_EINVAL, "shape %d: cuboid needs lo < hi", i);
  }
  return MPMHIP_OK;
}

int mpmhip_set_levelset_shapes(mpmhip_ctx *c, int32_t n, const mpmhip_shape *shapes, float friction) {
  // (a bad count or a missing array is refused without a message here; check_shapes words it for the other entries)
  if (!c || n < 0 || n > MPMHIP_MAX_SHAPES || (n > 0 && !shapes)) return MPMHIP_EINVAL;
  if (int rc = check_shapes(c, n, shapes)) return rc;
  if (c->LS.sdf.phi0) {  // shapes replace a sampled set: nothing of it survives
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    sdf_release(c);
  }
  c->LS.n = n;
  c->LS.friction = friction;
  c->LS.dynamic = 0; c->LS.n1 = 0;
  for (int i = 0; i < n; i++) {
    c->LS.s[i].type = shapes[i].type;
    c->LS.s[i].inside_out = shapes[i].inside_out;
    for (int k = 0; k < 6; k++) c->LS.s[i].p[k] = shapes[i].p[k];
  }
  if (c->d_LS) {  // (not yet allocated while mpmhip_create installs the config's planes: create uploads it)
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->d_LS, &c->LS, sizeof c->LS, hipMemcpyHostToDevice));
  }
  return MPMHIP_OK;
}

int mpmhip_set_levelset_keyframes(mpmhip_ctx *c, float t0, float t1, int32_t n0, const mpmhip_shape *shapes0, int32_t n1,
                                  const mpmhip_shape *shapes1, float friction) {
  if (!c) return MPMHIP_EINVAL;
  if (!(t1 > t0)) return fail(c, MPMHIP_EINVAL, "key frame times must satisfy t0 < t1");
  if (int rc = check_shapes(c, n0, shapes0)) return rc;
  if (int rc = check_shapes(c, n1, shapes1)) return rc;
  if (int rc = mpmhip_set_levelset_shapes(c, n0, shapes0, friction)) return rc;
  c->LS.dynamic = 1; c->LS.n1 = n1; c->LS.t0 = t0; c->LS.t1 = t1;
  for (int i = 0; i < n1; i++) {
    c->LS.s1[i].type = shapes1[i].type;
    c->LS.s1[i].inside_out = shapes1[i].inside_out;
    for (int k = 0; k < 6; k++) c->LS.s1[i].p[k] = shapes1[i].p[k];
  }
  HIPCHK(c, hipMemcpy(c->d_LS, &c->LS, sizeof c->LS, hipMemcpyHostToDevice));
  return MPMHIP_OK;
}

// device arrays for a sampled set of d's lattice (a static set keeps a second frame it already has: the next dynamic one reuses it)
static int sdf_reserve(mpmhip_ctx *c, const mpmhip_sdf_desc *d, bool two) {
  HIPCHK(c, c->sdf.reserve(c->LS.sdf, (size_t)d->res[0] * d->res[1] * d->res[2], two));
  return MPMHIP_OK;
}

// c->sdf.frame[0 / 1] hold the key frames: make them the ctx's level set
static int sdf_install(mpmhip_ctx *c, const mpmhip_sdf_desc *d, bool two, float t0, float t1, float friction) {
  SdfDev &S = c->LS.sdf;
  sdf_fill<3>(S, *d, c->sdf.frame[0], two ? c->sdf.frame[1].get() : nullptr, t0, t1);
  // the one-load path of the grid pass: same spacing as the grid and the origin on a node (to 1e-4 of a cell)
  S.aligned = d->spacing == c->P.dx;
  for (int k = 0; k < 3; k++) {
    const float o = d->origin[k] * c->P.idx, r = nearbyintf(o);
    if (!(fabsf(o - r) <= 1e-4f) || fabsf(r) > 65536.0f) S.aligned = 0;
    S.off[k] = S.aligned ? -(int)r : 0;
  }
  c->LS.n = 0; c->LS.dynamic = 0; c->LS.n1 = 0;  // the sampled set replaces the shapes
  c->LS.friction = friction;
  c->P.particle_collision = 0;
  HIPCHK(c, hipMemcpy(c->d_LS, &c->LS, sizeof c->LS, hipMemcpyHostToDevice));
  return MPMHIP_OK;
}

// Sampled level set: see include/mpmhip.h.  The arrays are copied into device memory the ctx owns; a call with the lattice of the
// installed set (the per-frame update of a dynamic level set) reuses that memory.
int mpmhip_set_levelset_sdf(mpmhip_ctx *c, const mpmhip_sdf_desc *d, const float *phi0, const float *phi1, float t0, float t1,
                            float friction) {
  if (!c) return MPMHIP_EINVAL;
  if (!d || !phi0) return fail(c, MPMHIP_EINVAL, "set_levelset_sdf: the lattice description and the first key frame are required");
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "set_levelset_sdf inside a substep");
  std::string why;
  const size_t count = sdf_lattice::check<3>(d->res, d->origin, d->spacing, why);
  if (!count) return fail(c, MPMHIP_EINVAL, "set_levelset_sdf: %s", why.c_str());
  if (phi1 && !(t1 > t0)) return fail(c, MPMHIP_EINVAL, "key frame times must satisfy t0 < t1");
  if (c->rigid.ls_collision)
    return fail(c, MPMHIP_EINVAL, "rigid_body_levelset_collision is not supported with a sampled level set");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // (kernels in flight read the arrays)
  if (int rc = sdf_reserve(c, d, phi1 != nullptr)) return rc;
  HIPCHK(c, hipMemcpy(c->sdf.frame[0], phi0, sizeof(float) * count, hipMemcpyHostToDevice));
  if (phi1) HIPCHK(c, hipMemcpy(c->sdf.frame[1], phi1, sizeof(float) * count, hipMemcpyHostToDevice));
  return sdf_install(c, d, phi1 != nullptr, t0, t1, friction);
}

// the device's level-set evaluation at host-given points (tests): phi in grid units, the unit gradient, d phi / dt, hit = 0 where
// there is no level set
int mpmhip_debug_levelset_sample(mpmhip_ctx *c, int64_t n, const float *pos, float t, float *phi, float *grad, float *dphidt,
                                 int32_t *hit) {
  if (!c || n <= 0 || !pos || !phi || !grad || !dphidt || !hit) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<float> dP, dO;
  HIPCHK(c, dP.alloc(3 * n));
  if (hipError_t e = dO.alloc(6 * n); e != hipSuccess) return fail(c, MPMHIP_EHIP, "hipMalloc failed: %s", hipGetErrorString(e));
  int rc = MPMHIP_OK;
  if (hipMemcpy(dP, pos, sizeof(float) * 3 * n, hipMemcpyHostToDevice) != hipSuccess) rc = fail(c, MPMHIP_EHIP, "hipMemcpy failed");
  if (!rc) rc = run_debug(c, k_debug_levelset_sample, c->LS, t, c->P.idx, n, (const float *)dP, dO.get(), dO + n, dO + 4 * n, reinterpret_cast<int32_t *>(dO + 5 * n));
  if (!rc) {
    hipError_t e = hipMemcpy(phi, dO, sizeof(float) * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(grad, dO + n, sizeof(float) * 3 * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(dphidt, dO + 4 * n, sizeof(float) * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(hit, dO + 5 * n, sizeof(int32_t) * n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(c, MPMHIP_EHIP, "hipMemcpy failed: %s", hipGetErrorString(e));
  }
  return rc;
}

int mpmhip_set_levelset(mpmhip_ctx *c, int32_t n_planes, const float *planes, float friction) {
  if (!c || n_planes < 0 || n_planes > 8 || (n_planes > 0 && !planes)) return MPMHIP_EINVAL;
  mpmhip_shape sh[8];
  memset(sh, 0, sizeof sh);
  for (int i = 0; i < n_planes; i++)
    for (int k = 0; k < 4; k++) sh[i].p[k] = planes[4 * i + k];
  return mpmhip_set_levelset_shapes(c, n_planes, sh, friction);
}

int mpmhip_add_group(mpmhip_ctx *c, int32_t material, const float params[MPMHIP_NPARAM]) {
  if (!c || !params) return MPMHIP_EINVAL;
  if (material < MPMHIP_VISCO || material > MPMHIP_ELASTIC) return fail(c, MPMHIP_EINVAL, "unknown material id %d", material);
  if ((int)c->groups.size() >= c->groups_cap) return fail(c, MPMHIP_ECAPACITY, "too many particle groups (max %d)", c->groups_cap);
  if (!(params[0] > 0) || !(params[1] > 0)) return fail(c, MPMHIP_EINVAL, "group mass and vol must be > 0");
  GroupParams g;
  memset(&g, 0, sizeof g);
  memcpy(g.p, params, sizeof g.p);
  g.type = material;
  c->groups.push_back(g);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(c->d_groups, c->groups.data(), sizeof(GroupParams) * c->groups.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return (int)c->groups.size() - 1;
}

// The particle positions changed behind k_g2p's back (uploads, new particles, deletions): key[] and the block flags
// G2P wrote for the OLD positions must not leak into the next sort — k_build_keys only ORs new flags on top, so stale
// ones would turn into phantom active blocks (empty tiles, inflated n_active, spurious capacity errors).
static int clear_block_flags(mpmhip_ctx *c, bool needed) {  // `needed`: what a RecordState transition returned
  if (needed) HIPCHK(c, hipMemsetAsync(c->blk_flag, 0, (size_t)c->P.nbw * 32, c->stream));
  return MPMHIP_OK;
}
static int invalidate_keys(mpmhip_ctx *c) { return clear_block_flags(c, c->rec.positions_changed()); }

// Every record of the ctx is dropped (the caller may put others in their place: set_slots): no slots, no deleted ones, no array
// that describes them.  n_dead is zeroed by a blocking copy, or on the ctx stream between the async stepper's launches.
enum DeadCount { DEAD_ZERO_SYNC, DEAD_ZERO_ON_STREAM, DEAD_KEEP };
static int drop_records(mpmhip_ctx *c, DeadCount dead) {
  set_slots(c, 0);
  const uint32_t zero = 0;
  if (dead == DEAD_ZERO_SYNC) HIPCHK(c, hipMemcpy(&c->cnt->n_dead, &zero, sizeof zero, hipMemcpyHostToDevice));
  if (dead == DEAD_ZERO_ON_STREAM) HIPCHK(c, hipMemsetAsync(&c->cnt->n_dead, 0, sizeof(uint32_t), c->stream));
  return clear_block_flags(c, c->rec.records_dropped());
}

// synchronise and read the device counters; reports the sticky capacity error
static int read_counters(mpmhip_ctx *c, Counters &h) {
  // through the ctx's pinned page: an "async" copy into pageable memory is staged and costs ~50 us more
  Counters *pin = reinterpret_cast<Counters *>(c->h_pinned.get());
  HIPCHK(c, hipMemcpyAsync(pin, c->cnt, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  h = *pin;
  if (c->rec.compact() && !c->rec.sorted() && !c->in_substep && (int64_t)h.n_sorted < c->n_slots) {
    // k_g2p left the live records in [0, n_sorted): the slots behind are all dead (particles deleted in earlier substeps)
    const uint32_t tail = (uint32_t)(c->n_slots - (int64_t)h.n_sorted);
    h.n_dead = h.n_dead >= tail ? h.n_dead - tail : 0u;
    set_slots(c, h.n_sorted);
    HIPCHK(c, hipMemcpy(&c->cnt->n_dead, &h.n_dead, sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  if (h.error & 1u)
    return fail(c, MPMHIP_ECAPACITY, "active blocks (%u) exceed max_blocks (%u): recreate the ctx with a larger max_blocks",
                h.n_active, c->P.max_blocks);
  if (h.error & 2u)
    return fail(c, MPMHIP_ECAPACITY, "a particle moved more than margin=%d cells outside this rank's brick between "
                "two migrations: migrate more often or raise the margin", c->T.margin);
  if (h.error & 16u)
    return fail(c, MPMHIP_EHIP, "tiled run: a peer rank's halo / migration epoch did not arrive within the wait limit "
                "(MPMHIP_TILE_WAIT_S): a rank is missing, stalled or out of step");
  if (h.error & SCAN_ERROR_BIT)
    return fail(c, MPMHIP_EHIP, "sort: a chained scan waited %.0f s for a chunk that never published its sum (k_sort.h): the launch did not "
                "fit the device's resident set (another runtime, a partitioned device, a debugger?) — lower MPMHIP_SCAN_GRID",
                (double)SCAN_WAIT_TICKS / 1e8);
  if (h.error & RIGID_MPR_ERROR_BIT)
    return fail(c, MPMHIP_EHIP, "rigid-rigid collisions: the portal refinement of a pair of bodies did not end within its loop bound "
                "(MPR_MAX_* of k_rigid_collide.h); the pair was treated as not colliding");
  if (h.error & 4u)
    return fail(c, MPMHIP_ECAPACITY, "the colored distance field of the rigid bodies needs more than %u pages of 4^3 nodes: "
                "recreate the ctx with a larger max_blocks", c->rigid.max_pages);
  return MPMHIP_OK;
}

// discard_apic_b: bring the apic_b side array up to date from RecP.A before anybody reads it or invalidates A
static int ensure_b_current(mpmhip_ctx *c) {
  if (!c->rec.b_stale()) return MPMHIP_OK;
  if (!c->rec.affine_valid()) return fail(c, MPMHIP_EINVAL, "internal: apic_b is stale and the affine matrices are invalid");
  hipLaunchKernelGGL(k_recover_b, dim3(particle_grid(c->n_slots)), dim3(256), 0, c->stream, c->P, (const RecG *)c->rg,
                     (const RecP *)c->rp, c->rb, (const GroupParams *)c->d_groups);
  int rc = launch_check(c, "recover_b");
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->rec.b_recovered();
  return MPMHIP_OK;
}

static int async_drop_view(mpmhip_ctx *c);
int mpmhip_add_particles(mpmhip_ctx *c, int32_t group, int64_t n, const float *x, const float *v, const float *F,
                         const float *B, const float *aux) {
  if (!c || n < 0 || (n > 0 && !x)) return MPMHIP_EINVAL;
  if (group < 0 || group >= (int)c->groups.size()) return fail(c, MPMHIP_EINVAL, "unknown group %d", group);
  if (n == 0) return MPMHIP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = async_drop_view(c)) return rc;  // (resident async stepper: records that only mirror the pools go first)
  if (c->n_slots + n > c->cap)
    return fail(c, MPMHIP_ECAPACITY, "particle capacity exceeded: %lld + %lld > %lld", (long long)c->n_slots, (long long)n, (long long)c->cap);
  if (int rc = ensure_b_current(c)) return rc;  // A of every particle is recomputed from apic_b below
  const int mat = c->groups[group].type;
  // Jp = 1 (:204), j = 1 (:460), logJp = 0 (:595), visco_tau = 1000 (:65)
  const float aux0 = (mat == MPMHIP_SNOW || mat == MPMHIP_WATER) ? 1.0f : (mat == MPMHIP_VISCO ? 1000.0f : 0.0f);
  std::vector<RecG> hg((size_t)n);
  std::vector<RecP> hp((size_t)n);
  std::vector<float> hb((size_t)n * BW, 0.0f);
  for (int64_t i = 0; i < n; i++) {
    RecG &g = hg[i];
    RecP &p = hp[i];
    for (int k = 0; k < 3; k++) {
      g.x[k] = p.x[k] = x[3 * i + k];
      p.v[k] = v ? v[3 * i + k] : 0.0f;
    }
    for (int k = 0; k < 9; k++) {
      g.F[k] = F ? F[9 * i + k] : ((k % 4 == 0) ? 1.0f : 0.0f);
      p.A[k] = 0.0f;
      hb[(size_t)i * BW + k] = B ? B[9 * i + k] : 0.0f;
    }
    g.aux = aux ? aux[i] : aux0;
    g.gid = (uint32_t)group;
    p.mass = c->groups[group].p[0];
    g.pid = c->next_pid + (int32_t)i;
    g.pad = 0;
  }
  c->next_pid += (int32_t)n;
  c->host_particle_bytes += (int64_t)n * (sizeof(RecG) + sizeof(RecP) + sizeof(float) * BW);
  HIPCHK(c, hipMemcpy(c->rg + c->n_slots, hg.data(), sizeof(RecG) * n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->rp + c->n_slots, hp.data(), sizeof(RecP) * n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->rb + (size_t)c->n_slots * BW, hb.data(), sizeof(float) * n * BW, hipMemcpyHostToDevice));
  set_slots(c, c->n_slots + n);
  return clear_block_flags(c, c->rec.particles_appended());
}

// drop every particle (groups, level set and configuration stay): the asynchronous stepper reloads the working set of
// every advance (AsyncMPM<dim>::advance gathers block pools into `particles`, src/async/async_mpm.cpp:255-318)
int mpmhip_clear_particles(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "clear_particles inside a substep");
  c->next_pid = 0;
  return drop_records(c, DEAD_ZERO_SYNC);
}
// base_delta_t / current_t of the next substeps (AsyncMPM<dim>::step sets both per advance, src/async/async_mpm.cpp:405-408)
int mpmhip_set_dt(mpmhip_ctx *c, float dt) {
  if (!c || !(dt >= 0)) return MPMHIP_EINVAL;
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "set_dt inside a substep");
  if (int rc = ensure_b_current(c)) return rc;  // the stored P2G matrices carry the old dt: they are rebuilt from apic_b
  c->P.dt = dt;
  c->rec.affine_inputs_changed();
  return MPMHIP_OK;
}
int mpmhip_set_time(mpmhip_ctx *c, double t) {
  if (!c) return MPMHIP_EINVAL;
  c->t = (float)t; c->request_t = (float)t;
  return MPMHIP_OK;
}
// the three clocks of a ctx (current_t, the request_t accumulator of step(), the substep counter that phases the physical
// reorder): read / restored when a host layer re-creates a ctx (e.g. to grow it) so that the run continues unchanged
int mpmhip_get_clock(const mpmhip_ctx *c, double *t, double *request_t, int64_t *substeps) {
  if (!c) return MPMHIP_EINVAL;
  if (t) *t = c->t;
  if (request_t) *request_t = c->request_t;
  if (substeps) *substeps = c->substeps;
  return MPMHIP_OK;
}
int mpmhip_set_clock(mpmhip_ctx *c, double t, double request_t, int64_t substeps) {
  if (!c || substeps < 0) return MPMHIP_EINVAL;
  c->t = (float)t; c->request_t = (float)request_t; c->substeps = substeps;
  return MPMHIP_OK;
}

int64_t mpmhip_num_particles(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  if (hipSetDevice(c->device) != hipSuccess) return MPMHIP_EHIP;
  Counters h;
  int rc = read_counters(c, h);
  return rc ? rc : c->n_slots - (int64_t)h.n_dead;
}

// host mirrors of the record arrays (download / upload are not on the hot path)
static int fetch_records(mpmhip_ctx *c, std::vector<RecG> &hg, std::vector<RecP> *hp, std::vector<float> *hb) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t n = (size_t)c->n_slots;
  c->host_particle_bytes += (int64_t)n * (sizeof(RecG) + (hp ? sizeof(RecP) : 0) + (hb ? sizeof(float) * BW : 0));
  hg.resize(n);
  if (n) HIPCHK(c, hipMemcpy(hg.data(), c->rg, sizeof(RecG) * n, hipMemcpyDeviceToHost));
  if (hp) { hp->resize(n); if (n) HIPCHK(c, hipMemcpy(hp->data(), c->rp, sizeof(RecP) * n, hipMemcpyDeviceToHost)); }
  if (hb) { hb->resize(n * BW); if (n) HIPCHK(c, hipMemcpy(hb->data(), c->rb, sizeof(float) * n * BW, hipMemcpyDeviceToHost)); }
  return MPMHIP_OK;
}

int mpmhip_download(mpmhip_ctx *c, int32_t field, void *dst, int64_t n_capacity) {
  if (!c || !dst) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (field < MPMHIP_F_X || field > MPMHIP_F_STATES) return fail(c, MPMHIP_EINVAL, "unknown field %d", field);
  if (field == MPMHIP_F_B)
    if (int rc = ensure_b_current(c)) return rc;
  std::vector<RecG> hg;
  std::vector<RecP> hp;
  std::vector<float> hb;
  int rc = fetch_records(c, hg, field == MPMHIP_F_V ? &hp : nullptr, field == MPMHIP_F_B ? &hb : nullptr);
  if (rc) return rc;
  int64_t m = 0;
  for (size_t i = 0; i < hg.size(); i++) {  // live slots, in slot order
    if (hg[i].pid < 0) continue;
    if (m >= n_capacity) return fail(c, MPMHIP_ECAPACITY, "download buffer holds %lld particles, more are alive", (long long)n_capacity);
    float *f = (float *)dst;
    int32_t *q = (int32_t *)dst;
    switch (field) {
      case MPMHIP_F_X: for (int k = 0; k < 3; k++) f[3 * m + k] = hg[i].x[k]; break;
      case MPMHIP_F_V: for (int k = 0; k < 3; k++) f[3 * m + k] = hp[i].v[k]; break;
      case MPMHIP_F_B: for (int k = 0; k < 9; k++) f[9 * m + k] = hb[i * BW + k]; break;
      case MPMHIP_F_F: for (int k = 0; k < 9; k++) f[9 * m + k] = hg[i].F[k]; break;
      case MPMHIP_F_AUX: f[m] = hg[i].aux; break;
      case MPMHIP_F_GID: q[m] = (int32_t)hg[i].gid; break;
      case MPMHIP_F_ID: q[m] = hg[i].pid; break;
      case MPMHIP_F_STATES: q[m] = (int32_t)hg[i].pad; break;
    }
    m++;
  }
  return (int)m;
}

int mpmhip_upload(mpmhip_ctx *c, int32_t field, const void *src, int64_t n) {
  if (!c || !src) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (field < MPMHIP_F_X || field > MPMHIP_F_STATES || field == MPMHIP_F_GID)
    return fail(c, MPMHIP_EINVAL, "field %d cannot be uploaded", field);
  std::vector<RecG> hg;
  std::vector<RecP> hp;
  std::vector<float> hb;
  int rc = ensure_b_current(c);
  if (rc) return rc;
  if ((rc = fetch_records(c, hg, &hp, &hb))) return rc;
  int64_t live = 0;
  for (auto &g : hg) live += g.pid >= 0;
  if (n != live) return fail(c, MPMHIP_EINVAL, "upload of %lld records but the ctx holds %lld particles", (long long)n, (long long)live);
  const float *f = (const float *)src;
  const int32_t *q = (const int32_t *)src;
  int64_t m = 0;
  for (size_t i = 0; i < hg.size(); i++) {
    if (hg[i].pid < 0) continue;
    switch (field) {
      case MPMHIP_F_X: for (int k = 0; k < 3; k++) hg[i].x[k] = hp[i].x[k] = f[3 * m + k]; break;
      case MPMHIP_F_V: for (int k = 0; k < 3; k++) hp[i].v[k] = f[3 * m + k]; break;
      case MPMHIP_F_B: for (int k = 0; k < 9; k++) hb[i * BW + k] = f[9 * m + k]; break;
      case MPMHIP_F_F: for (int k = 0; k < 9; k++) hg[i].F[k] = f[9 * m + k]; break;
      case MPMHIP_F_AUX: hg[i].aux = f[m]; break;
      case MPMHIP_F_STATES: hg[i].pad = (uint32_t)q[m]; break;
      case MPMHIP_F_ID:
        hg[i].pid = q[m] < 0 ? 0 : q[m];
        if (hg[i].pid + 1 > c->next_pid) c->next_pid = hg[i].pid + 1;
        break;
    }
    m++;
  }
  const size_t ns = hg.size();
  c->host_particle_bytes += (int64_t)ns * (sizeof(RecG) + sizeof(RecP) + sizeof(float) * BW);
  HIPCHK(c, hipMemcpy(c->rg, hg.data(), sizeof(RecG) * ns, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->rp, hp.data(), sizeof(RecP) * ns, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->rb, hb.data(), sizeof(float) * ns * BW, hipMemcpyHostToDevice));
  if (field == MPMHIP_F_X || field == MPMHIP_F_V)
    if (int rc = invalidate_keys(c)) return rc;
  if (field == MPMHIP_F_B || field == MPMHIP_F_F || field == MPMHIP_F_AUX) c->rec.affine_inputs_changed();
  if (field == MPMHIP_F_ID) c->rec.ids_changed(c->deterministic);
  return MPMHIP_OK;
}

// ------------------------------------------------------------------------------------------------ phases
static int do_reorder(mpmhip_ctx *c);

static inline bool rigid_active(const mpmhip_ctx *c);
// bit t set = some particle group of the ctx is of material type t
static uint32_t material_mask(const mpmhip_ctx *c) {
  uint32_t mask = 0;
  for (const GroupParams &g : c->groups) mask |= 1u << (g.type & 31);
  return mask;
}
static_assert(lp::RANK_BATCH == RANK_BATCH && lp::BC == BC && lp::MAT_ALL == MAT_ALL, "launch_plan.h: copies of the device-side constants");
// what the launch plans depend on (launch_plan.h).  The fill statistics are {live particles, active blocks, owner entries} of a
// recent sort: k_cell_table's last chunk stores them straight into the pinned page, never waited for, so they may be a few
// substeps old ({0, 0, 0} before the first sort has reported)
static lp::Facts facts(const mpmhip_ctx *c) {
  const volatile FillStats *fs = reinterpret_cast<const volatile FillStats *>(c->h_pinned + mpmhip_ctx::FILL_STATS_WORD);
  lp::Facts f;
  f.n_slots = c->n_slots; f.max_blocks = c->P.max_blocks; f.nbw = c->P.nbw; f.n_cus = c->n_cus;
  f.mask = material_mask(c);
  f.n_live = fs->n_live; f.n_act = fs->n_active; f.n_own = fs->n_own;
  f.keyed_table = c->cellcnt_key != nullptr; f.tiled = c->T.enabled != 0; f.has_boxes = c->T.n_boxes > 0;
  f.rigid = rigid_active(c); f.deterministic = c->deterministic; f.store_b = c->P.store_b != 0;
  f.sampled_levelset = c->LS.sdf.phi0 != nullptr; f.has_chunk_blk = c->chunk_blk != nullptr;
  return f;
}
// workgroups a chained-scan kernel may be launched with (launch_plan.h: scan_grid_for), per kernel: asked of the occupancy API once
static uint32_t scan_limit(mpmhip_ctx *c, const void *kernel) {
  const void *key = kernel;
  auto it = c->scan_limits.find(key);
  if (it != c->scan_limits.end()) return it->second;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu < 1) per_cu = 1;
  const uint32_t lim = lp::scan_grid_for(c->n_cus, per_cu, c->knobs.scan_grid);
  c->scan_limits[key] = lim;
  return lim;
}
static int do_sort(mpmhip_ctx *c) {
  const lp::SortPlan plan = lp::plan_sort(c->knobs, facts(c));
  Params &P = c->P;
  hipStream_t st = c->stream;
  const int pg = particle_grid(c->n_slots);
  const bool build_keys = !c->rec.keys_valid();
  if (build_keys) hipLaunchKernelGGL(k_build_keys, dim3(pg), dim3(256), 0, st, P, c->rg, c->rp, c->cnt, c->key, c->blk_flag);
  // pidc[] holds the ids of the current key[]: k_build_keys wrote both just now, or the last G2P did
  const bool ids_cached = P.pidc && (build_keys || c->rec.pidc_valid());
  c->list_valid = plan.build_list;
  c->last_sort.keyed = plan.keyed; c->last_sort.build_list = plan.build_list; c->last_sort.ct = plan.ct;
  c->last_sort.cell_order_form = plan.cell_order_form; c->last_sort.ids_cached = ids_cached; c->last_sort.deterministic = c->deterministic;
  uint32_t *const nbr = plan.build_list ? c->nbr : nullptr;
  uint32_t epoch = ++c->sort_epoch;
  if ((epoch & 0x7FFFFFu) == 0u) epoch = ++c->sort_epoch;  // (k_cell_table's scan words keep 23 bits of it; 0 = never published)
  // (single-pass scans: never more workgroups than are resident at once, see k_sort.h)
  uint32_t *counters = c->cell_cnt;
  if (plan.keyed) {
    // block table and in-cell ranks in ONE launch (k_sort_front): the ranks count into key-indexed counters and need no table
    const uint32_t bt_wgs = std::min(plan.bt_chunks, scan_limit(c, (const void *)k_sort_front));
    hipLaunchKernelGGL(k_sort_front, dim3(bt_wgs + plan.rank_wgs), dim3(256), 0, st, P, c->blk_flag, c->bits, c->wprefix, c->act_blk, c->cnt,
                       c->scan_slots, epoch, bt_wgs, c->key, c->rank, c->cellcnt_key);
    counters = c->cellcnt_key;
  } else {
    const uint32_t bt_wgs = std::min(plan.bt_chunks, scan_limit(c, (const void *)k_block_table));
    hipLaunchKernelGGL(k_block_table, dim3(bt_wgs), dim3(256), 0, st, P, c->blk_flag, c->bits, c->wprefix, c->act_blk, c->cnt, c->scan_slots, epoch);
    hipLaunchKernelGGL(k_rank, dim3(plan.rank_wgs), dim3(256), 0, st, P, c->key, c->rank, c->cell_cnt, c->bits, c->wprefix,
                       c->cnt, (const uint32_t *)c->act_blk, nbr);
  }
  if (plan.build_list) {  // (the two forms publish different scan words: each has its own slots)
    const auto kern = cell_table_kernel(plan);
    const uint32_t ct_wgs = std::min(plan.ct_chunks, scan_limit(c, (const void *)kern));
    if (epoch - c->list_clear_epoch >= (1u << 22)) {
      // the list form's scan words keep 23 bits of the epoch, and a word is only rewritten when that form runs with the chunk in use: one
      // left from epoch e would match again at e + 2^23 (8.4 M sorts: reachable in a long run).  Zeroing them every 2^22 sorts keeps every
      // surviving word younger than that; the epoch field 0 is never published.
      HIPCHK(c, hipMemsetAsync(c->scan_slots + c->bt_slots + c->ct_slots, 0, sizeof(unsigned long long) * c->ct_slots, st));
      c->list_clear_epoch = epoch;
    }
    hipLaunchKernelGGL(kern, dim3(ct_wgs), dim3(256), 0, st, P,
                       c->cnt, counters, c->act_start, c->cell_start, c->scan_slots + c->bt_slots + c->ct_slots, epoch, c->knobs.rank_runs_mul,
                       c->chunk_blk, nbr, c->own_list, c->d_stats, (const uint32_t *)c->act_blk, (const uint32_t *)c->bits, (const uint32_t *)c->wprefix);
  } else {
    const auto kern = cell_table_plain_kernel(plan);
    const uint32_t ct_wgs = std::min(plan.ct_chunks, scan_limit(c, (const void *)kern));
    hipLaunchKernelGGL(kern, dim3(ct_wgs), dim3(256), 0, st, P,
                       c->cnt, counters, c->act_start, c->cell_start, c->scan_slots + c->bt_slots, epoch, c->knobs.rank_runs_mul, c->chunk_blk,
                       c->d_stats, (const uint32_t *)c->act_blk);
  }
  if (plan.keyed)
    hipLaunchKernelGGL(k_perm_keyed, dim3(pg), dim3(256), 0, st, P, (const Counters *)c->cnt, c->key, c->rank, c->cell_start, c->perm,
                       (const uint32_t *)c->bits, (const uint32_t *)c->wprefix);
  else
    hipLaunchKernelGGL(k_perm, dim3(pg), dim3(256), 0, st, P, (const Counters *)c->cnt, c->key, c->rank, c->cell_start, c->perm);
  if (c->deterministic) {
    // every cell's entries in ascending creation id (k_sort.h: k_cell_order); rank[] is idle until the next sort: the ordered index goes
    // there and then IS the index
    if (plan.cell_order_form == 0)
      hipLaunchKernelGGL((ids_cached ? k_cell_order<true> : k_cell_order<false>), dim3(plan.cell_order_wgs), dim3(256), 0, st, P, (const Counters *)c->cnt,
                         (const uint32_t *)c->cell_start, (const uint32_t *)c->perm, (const float4 *)c->rg.get(), c->rank);
    else
      hipLaunchKernelGGL((ids_cached ? k_cell_order_blocks<true> : k_cell_order_blocks<false>), dim3(plan.cell_order_wgs), dim3(256), 0, st, P,
                         (const Counters *)c->cnt, (const uint32_t *)c->cell_start, (const uint32_t *)c->perm, (const float4 *)c->rg.get(), c->rank);
    std::swap(c->perm, c->rank);
  }
  // (k_cell_table's last chunk stores (live particles, active blocks, owner entries) of this sort straight into the pinned page,
  // never waited for: the host picks the G2P walk by how full the blocks are and sizes the grid pass's launch from numbers
  // that may be a few substeps old: facts)
  c->rec.sort_done();  // (key[] now holds k_rank's packed (rank, cell index) words)
  int rc = launch_check(c, "sort");
  if (rc) return rc;
  // sort_allocator (src/mpm.cpp:752-768, every reorder_interval substeps :811-813): needed here only for records that
  // did not come out of k_g2p (fresh uploads, arrivals of a migration) — k_g2p itself leaves the records in sorted order
  // every substep, so a running simulation never pays for a separate reorder (nor for its host synchronisation)
  // (not for the working sets of the resident asynchronous stepper: they live for ONE substep)
  if ((c->reorder_interval > 0 && !c->rec.ordered() && !c->async.resident) || c->compact_requested) {
    c->compact_requested = false;
    return do_reorder(c);
  }
  return MPMHIP_OK;
}

// physical reorder into sorted order + compaction of deleted slots (sort_allocator, src/mpm.cpp:752-768).
// Needs the live count on the host, hence one synchronisation: keep reorder_interval large.
static int do_reorder(mpmhip_ctx *c) {
  const int pg = particle_grid(c->n_slots * 4);
  hipLaunchKernelGGL(k_gather_records, dim3(pg), dim3(256), 0, c->stream, c->cnt, c->perm, (const float4 *)c->rg.get(),
                     (const float4 *)c->rp.get(), (const float4 *)c->rb.get(), (float4 *)c->rg2.get(), (float4 *)c->rp2.get(), (float4 *)c->rb2.get());
  hipLaunchKernelGGL(k_identity_perm, dim3(particle_grid(c->n_slots)), dim3(256), 0, c->stream, c->cnt, c->perm);
  int rc = launch_check(c, "reorder");
  if (rc) return rc;
  Counters h;
  if ((rc = read_counters(c, h))) return rc;
  std::swap(c->rg, c->rg2); std::swap(c->rp, c->rp2); std::swap(c->rb, c->rb2);
  c->rec.reordered();
  set_slots(c, h.n_sorted);
  const uint32_t zero = 0;
  HIPCHK(c, hipMemcpy(&c->cnt->n_dead, &zero, sizeof zero, hipMemcpyHostToDevice));
  return MPMHIP_OK;
}

static RigidXfer rigid_xfer(mpmhip_ctx *c);
// The plain transfer kernel (every block away from the bodies) and the colour-aware one (the flagged blocks) touch disjoint
// blocks and particles, and each is latency-bound at two waves per SIMD: they run side by side, the colour-aware kernel on a
// second stream that waits for what the ctx stream has enqueued so far (fork) and is waited for before anything else (join).
static int rigid_fork(mpmhip_ctx *c, hipStream_t *s, int which) {
  auto &R = c->rigid;
  *s = c->stream;
  if (!(c->knobs.rigid_concurrent & which)) return MPMHIP_OK;
  if (!R.side) {
    // the highest priority: the colour-aware kernels are the longer ones of a pair and get their wave slots first
    // (8 M scene: 1.163 -> 1.150 ms per substep against the default priority)
    int lo = 0, hi = 0;  // (numerically lower = higher priority)
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    HIPCHK(c, hipStreamCreateWithPriority(&R.side, hipStreamNonBlocking, hi));
    HIPCHK(c, hipEventCreateWithFlags(&R.ev_fork, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&R.ev_join, hipEventDisableTiming));
  }
  HIPCHK(c, hipEventRecord(R.ev_fork, c->stream));
  HIPCHK(c, hipStreamWaitEvent(R.side, R.ev_fork, 0));
  *s = R.side;
  return MPMHIP_OK;
}
static int rigid_join(mpmhip_ctx *c, hipStream_t s) {
  if (s == c->stream) return MPMHIP_OK;
  HIPCHK(c, hipEventRecord(c->rigid.ev_join, s));
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->rigid.ev_join, 0));
  return MPMHIP_OK;
}
static int do_rigid_apply_tmp(mpmhip_ctx *c);
static int rigid_imp_rows(mpmhip_ctx *c);

static int do_p2g(mpmhip_ctx *c, int phase = 0) {
  const lp::P2GPlan plan = lp::plan_p2g(c->knobs, facts(c));
  if (!c->rec.affine_valid()) {
    hipLaunchKernelGGL(k_affine, dim3(particle_grid(c->n_slots)), dim3(256), 0, c->stream, c->P, c->rg, c->rp, c->rb,
                       c->d_groups);
    c->rec.affine_rebuilt();
  }
  // one wavefront per block (all 27 nodes, all particles) measured fastest at 256^3 / 8 M: 0.187 ms against
  // 0.237 (two waves splitting the nodes) and 0.225 (two waves splitting the particles).  Splitting the particles does
  // not help small problems either (128^3 / 1 M, where only 2 448 waves exist: 34 us with one wave per block, 37 with
  // two, 48 with four)
  hipStream_t rs = c->stream;
  if (plan.rigid) { if (int rc = rigid_fork(c, &rs, 1)) return rc; }
  hipLaunchKernelGGL(plan.rigid ? k_p2g<true> : k_p2g<false>, dim3(plan.wgs), dim3(64), 0, c->stream, c->P,
                     (const float4 *)c->rp.get(), c->cnt, c->act_blk, c->cell_start, c->perm, c->d_groups, c->tiles, c->T, phase,
                     plan.rigid ? (const uint8_t *)c->rigid.d_blk_rigid : (const uint8_t *)nullptr);
  if (plan.rigid) {  // blocks near a body (block_op_rigid), then RigidBody::apply_tmp_velocity (src/transfer.cpp:578-580)
    if (plan.rigid_mats.kind == lp::MatSet::ALL_DET) { if (int rc = rigid_imp_rows(c)) return rc; }
    hipLaunchKernelGGL(rigid_p2g_kernel(plan.rigid_mats), dim3(plan.rigid_wgs), dim3(64), 0, rs, c->P, (const float4 *)c->rp.get(),
                       (const float4 *)c->rg.get(), c->cnt, c->act_blk, c->cell_start, c->perm, c->d_groups, c->tiles, rigid_xfer(c));
    if (int rc = rigid_join(c, rs)) return rc;
    // (a job with bodies: this rank's sums go out as its row, the sum over the ranks is applied behind the wait — tn_rows_apply)
    if (int rc = c->rows_substep ? tn_row_out(c, 0) : do_rigid_apply_tmp(c)) return rc;
  }
  return launch_check(c, "p2g");
}
// dense: what the kernels' `dense` argument points at; nullptr: the ctx's staging array of the dense views (modes 1-3; unused in mode 0)
static int do_grid(mpmhip_ctx *c, int mode, int phase = 0, float4 *dense = nullptr) {
  const lp::GridPlan plan = lp::plan_grid(c->knobs, facts(c), mode, c->list_valid);
  if (!dense) dense = c->dense;
  c->P.t = c->t;  // this->current_t of the substep in flight (src/mpm.cpp:532-533)
  c->LS.dirichlet = c->dirichlet ? 1 : 0;
  if (plan.refuse_energy_on_tiled)
    // (only the owner-list walk knows which rank counts a halo node's kinetic energy — the lowest that holds mass on it; the per-block
    // walk would add every halo node on every rank that holds it)
    return fail(c, MPMHIP_EINVAL, "calculate_energy of a tiled ctx needs the owner-list walk of the grid pass: do not set MPMHIP_GRID_WALK=0");
  if (plan.walk == lp::GridWalk::LIST)
    hipLaunchKernelGGL(grid_list_kernel(plan, mode), dim3(plan.wgs), dim3(256), 0, c->stream, c->P, c->cnt, (const uint32_t *)c->nbr,
                       (const uint32_t *)c->own_list, c->tiles, c->gridv, c->fat_slot, reinterpret_cast<double *>(dense), c->T,
                       c->d_boxes_cur, c->LS, phase);
  else
    hipLaunchKernelGGL(grid_blocks_kernel(plan, mode), dim3(plan.wgs), dim3(256), 0, c->stream, c->P, c->cnt, c->act_blk, c->bits, c->wprefix,
                       c->tiles, c->gridv, c->fat_slot, dense, c->T, c->d_boxes_cur, c->LS, phase);
  return launch_check(c, "grid");
}
static int do_g2p(mpmhip_ctx *c, int phase = 0) {
  const lp::G2PPlan plan = lp::plan_g2p(c->knobs, facts(c), phase);
  c->P.t = c->t;
  // what every G2P kernel takes; tail: the chunk table (packed), the phase (per block), the bodies (colour-aware)
  auto launch = [&](auto kern, int wgs, hipStream_t s, auto... tail) {
    hipLaunchKernelGGL(kern, dim3(wgs), dim3(256), 0, s, c->P, (const float4 *)c->rg.get(), (float4 *)c->rg2.get(), (float4 *)c->rp2.get(),
                       (float4 *)c->rb2.get(), c->cnt, c->act_blk, c->act_start, c->perm, c->d_groups, c->gridv, c->fat_slot, c->cnt, c->key,
                       c->blk_flag, (const LevelSetDev *)c->d_LS, tail...);
  };
  if (plan.packed) {
    launch(g2p_packed_kernel(plan), plan.wgs, c->stream, (const uint32_t *)c->chunk_blk);
    c->rec.g2p_done(plan.store_b, c->P.pidc != nullptr);
    return launch_check(c, "g2p_packed");
  }
  hipStream_t rs = c->stream;
  if (plan.rigid) { if (int rc = rigid_fork(c, &rs, 2)) return rc; }
  launch(g2p_kernel(plan), plan.wgs, c->stream, phase_box(c->T), phase);
  if (plan.rigid) {
    if (plan.rigid_mats.kind == lp::MatSet::ALL_DET) { if (int rc = rigid_imp_rows(c)) return rc; }
    launch(rigid_g2p_kernel(plan.rigid_mats), plan.rigid_wgs, rs, rigid_xfer(c));
    if (int rc = rigid_join(c, rs)) return rc;
    if (int rc = c->rows_substep ? tn_row_out(c, 1) : do_rigid_apply_tmp(c)) return rc;
  }
  c->rec.g2p_done(plan.store_b, c->P.pidc != nullptr);
  return launch_check(c, "g2p");
}

// particle_collision against a sampled level set (k_sdf.h): behind the LAST k_g2p launch of a substep, on the buffers it wrote
static int do_sdf_collide(mpmhip_ctx *c) {
  if (!c->LS.sdf.phi0 || !c->particle_collision_cfg || c->n_slots == 0) return MPMHIP_OK;
  hipLaunchKernelGGL(k_sdf_collide, dim3(particle_grid(c->n_slots)), dim3(256), 0, c->stream, c->P, (const Counters *)c->cnt,
                     (float4 *)c->rg2.get(), (float4 *)c->rp2.get(), c->key, c->blk_flag, c->cnt, c->LS.sdf);
  return launch_check(c, "sdf_collide");
}

// behind the LAST k_g2p launch of a substep: the buffers it wrote become the current records
static void swap_records(mpmhip_ctx *c) {
  std::swap(c->rg, c->rg2); std::swap(c->rp, c->rp2); std::swap(c->rb, c->rb2);
  c->rec.records_swapped();
}

static int need_sorted(mpmhip_ctx *c, const char *who) {
  if (!c->rec.sorted()) return fail(c, MPMHIP_EINVAL, "%s needs sorted particles: call mpmhip_sort first", who);
  return MPMHIP_OK;
}

#include "rigid_api.h"
#include "rigid_collide_api.h"
#include "mesh_sdf_api.h"

int mpmhip_sort(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  return do_sort(c);
}
int mpmhip_p2g(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = need_sorted(c, "p2g");
  return rc ? rc : do_p2g(c);
}
int mpmhip_grid_update(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = need_sorted(c, "grid_update");
  return rc ? rc : do_grid(c, 0);
}
int mpmhip_g2p(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = need_sorted(c, "g2p");
  if (rc || (rc = do_g2p(c)) || (rc = do_sdf_collide(c))) return rc;
  swap_records(c);
  return MPMHIP_OK;
}

static int get_events(mpmhip_ctx *c, mpmhip_ctx::Ev **out) {
  if (c->ev_used == c->ev_pool.size()) {
    mpmhip_ctx::Ev ev;
    for (int k = 0; k <= PH_COUNT; k++) HIPCHK(c, hipEventCreate(&ev.e[k]));
    c->ev_pool.push_back(ev);
  }
  *out = &c->ev_pool[c->ev_used++];
  return MPMHIP_OK;
}

static int collect_events(mpmhip_ctx *c) {
  if (c->ev_used == 0) return MPMHIP_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < c->ev_used; i++) {
    if (c->ev_level == 4) {  // begin part -> "p2g", interior part (split substeps) -> "grid", end part -> "g2p"
      float ms = 0;
      HIPCHK(c, hipEventElapsedTime(&ms, c->ev_pool[i].e[0], c->ev_pool[i].e[1]));
      c->phase_ms[PH_P2G] += ms;
      if (c->ev_pool[i].ov) {
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev_pool[i].e[2], c->ev_pool[i].e[3]));
        c->phase_ms[PH_GRID] += ms;
      }
      HIPCHK(c, hipEventElapsedTime(&ms, c->ev_pool[i].e[4], c->ev_pool[i].e[5]));
      c->phase_ms[PH_G2P] += ms;
      c->prof_substeps++;
      continue;
    }
    if (c->ev_pool[i].ov && c->ev_level >= 2) {  // split substep: the interior launch was bracketed separately
      float ms = 0;
      const int a = c->ev_level == 2 ? 0 : 3;
      HIPCHK(c, hipEventElapsedTime(&ms, c->ev_pool[i].e[a], c->ev_pool[i].e[a + 1]));
      c->phase_ms[c->ev_level == 2 ? PH_G2P : PH_P2G] += ms;
    }
    for (int k = 0; k < PH_COUNT; k++) {
      if ((c->ev_level == 2 && k != PH_G2P) || (c->ev_level == 3 && k != PH_P2G)) continue;
      float ms = 0;
      HIPCHK(c, hipEventElapsedTime(&ms, c->ev_pool[i].e[k], c->ev_pool[i].e[k + 1]));
      c->phase_ms[k] += ms;
    }
    c->prof_substeps++;
  }
  c->ev_used = 0;
  return MPMHIP_OK;
}

static int do_halo_pack(mpmhip_ctx *c) {
  if (c->T.n_boxes == 0) return MPMHIP_OK;
  int nb = (int)((c->T.box_blocks + 3) / 4);  // one wave per grid block of a box
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(k_halo_pack, dim3(nb), dim3(256), 0, c->stream, c->P, c->T, c->d_boxes_cur, c->bits, c->wprefix,
                     (const float4 *)c->tiles);
  return launch_check(c, "halo_pack");
}

// A tiled substep is begin [exchange] end, or — with mpmhip_set_overlap — begin [exchange starts] interior
// [exchange done] end: begin runs the sort, the P2G of the blocks that touch a halo box and the halo pack; interior
// runs everything that cannot touch a halo node (P2G, grid, G2P) while the boxes are on the wire; end finishes the
// boundary part with the peers' sums.  With level-1 profiling the split is off so the phase table stays clean.
int mpmhip_substep_begin(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "substep_begin called twice without substep_end");
  int rc;
  mpmhip_ctx::Ev *ev = nullptr;
  int lvl = c->profiling;
  const bool bodies = rigid_active(c);
  // (the colour-aware kernels have no phase argument: a ctx with bodies runs its substeps unsplit, whatever mpmhip_set_overlap said)
  c->ov_active = c->overlap && c->T.n_boxes > 0 && lvl != 1 && !bodies;
  c->interior_done = false;
  c->rows_substep = c->tn.on && c->tn.rows;
  if ((lvl == 2 || lvl == 3) && c->prof_every > 1 && (c->substeps % c->prof_every) != 0) lvl = 0;  // not a sampled substep
  if (lvl) {
    if (c->ev_used >= 4096 && (rc = collect_events(c))) return rc;
    if ((rc = get_events(c, &ev))) return rc;
    ev->ov = c->ov_active;
    if (lvl == 1 || lvl == 4) HIPCHK(c, hipEventRecord(ev->e[0], c->stream));
  }
  // articulate + rasterize_rigid_boundary (src/mpm.cpp:466-472) next to the sort, gather_cdf (:506-508) behind both
  hipStream_t rs = c->stream;
  if (bodies && (rc = do_rigid_rigidify(c, c->P.dt))) return rc;  // rigidify opens the block (:468), on the ctx stream, before the fork
  if (bodies && ((rc = rigid_fork(c, &rs, 4)) || (rc = do_rigid_pre_a(c, rs)))) return rc;
  if ((rc = do_sort(c))) return rc;
  if (bodies && ((rc = rigid_join(c, rs)) || (rc = do_rigid_pre_b(c)))) return rc;
  if (ev && (lvl == 1 || lvl == 3)) HIPCHK(c, hipEventRecord(ev->e[1], c->stream));
  if ((rc = do_p2g(c, c->ov_active ? 1 : 0))) return rc;
  if (ev && lvl == 3) HIPCHK(c, hipEventRecord(ev->e[2], c->stream));
  if (c->tn.on) tn_begin_substep(c);  // (native data plane: this substep's epoch and box table)
  if ((rc = do_halo_pack(c))) return rc;
  if (ev && lvl == 1) HIPCHK(c, hipEventRecord(ev->e[2], c->stream));
  if (ev && lvl == 4) HIPCHK(c, hipEventRecord(ev->e[1], c->stream));
  c->cur_ev = ev;
  c->in_substep = true;
  return MPMHIP_OK;
}

int mpmhip_substep_interior(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->in_substep) return fail(c, MPMHIP_EINVAL, "substep_interior without substep_begin");
  if (!c->ov_active || c->interior_done) return MPMHIP_OK;
  int rc;
  mpmhip_ctx::Ev *ev = c->cur_ev;
  const int lvl = c->profiling;
  if (ev && lvl == 3) HIPCHK(c, hipEventRecord(ev->e[3], c->stream));
  if (ev && lvl == 4) HIPCHK(c, hipEventRecord(ev->e[2], c->stream));
  if ((rc = do_p2g(c, 2))) return rc;
  if (ev && lvl == 3) HIPCHK(c, hipEventRecord(ev->e[4], c->stream));
  if ((rc = do_grid(c, 0, 2))) return rc;
  if (ev && lvl == 2) HIPCHK(c, hipEventRecord(ev->e[0], c->stream));
  if ((rc = do_g2p(c, 2))) return rc;
  if (ev && lvl == 2) HIPCHK(c, hipEventRecord(ev->e[1], c->stream));
  if (ev && lvl == 4) HIPCHK(c, hipEventRecord(ev->e[3], c->stream));
  c->interior_done = true;
  return MPMHIP_OK;
}

// behind the G2P of a substep whose impulse rows went to the job (tn.rows): the rows of the rigid G2P summed and applied, then what
// substep_end does behind the records' swap.  mpmhip_tiled_advance_group calls it for every rank once every rank's G2P is enqueued.
static int substep_finish_rows(mpmhip_ctx *c) {
  int rc;
  if (!c->rows_substep) return MPMHIP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  c->rows_substep = false;
  if ((rc = tn_rows_apply(c, 1))) return rc;
  if ((rc = do_rigid_advect(c, c->P.dt))) return rc;  // src/mpm.cpp:570-572
  c->t += c->P.dt;  // src/mpm.cpp:573
  c->substeps++;
  return MPMHIP_OK;
}

int mpmhip_substep_end(mpmhip_ctx *c) {  // grid (+ halo sum), G2P
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->in_substep) return fail(c, MPMHIP_EINVAL, "substep_end without substep_begin");
  int rc;
  if (c->ov_active && !c->interior_done && (rc = mpmhip_substep_interior(c))) return rc;  // caller skipped it
  mpmhip_ctx::Ev *ev = c->cur_ev;
  c->cur_ev = nullptr;
  c->in_substep = false;
  const int lvl = c->profiling, ph = c->ov_active ? 1 : 0;
  if (c->rows_substep && (rc = tn_rows_apply(c, 0))) return rc;  // (the rigid P2G's impulses of ALL ranks: RigidBody::apply_tmp_velocity)
  if (rigid_active(c) && c->rigid.ls_collision && (rc = do_rigid_ls_collision(c))) return rc;  // src/mpm.cpp:535-538
  if (ev && lvl == 1) HIPCHK(c, hipEventRecord(ev->e[3], c->stream));
  if (ev && lvl == 4) HIPCHK(c, hipEventRecord(ev->e[4], c->stream));
  if ((rc = do_grid(c, 0, ph))) return rc;
  if (ev && (lvl == 1 || lvl == 2)) HIPCHK(c, hipEventRecord(ev->e[4], c->stream));
  if ((rc = do_g2p(c, ph))) return rc;
  if ((rc = do_sdf_collide(c))) return rc;
  if (ev && (lvl == 1 || lvl == 2 || lvl == 4)) HIPCHK(c, hipEventRecord(ev->e[5], c->stream));
  swap_records(c);
  if (c->rows_substep) return c->tn.defer_finish ? MPMHIP_OK : substep_finish_rows(c);
  if (rigid_active(c) && (rc = do_rigid_advect(c, c->P.dt))) return rc;  // src/mpm.cpp:570-572
  c->t += c->P.dt;  // src/mpm.cpp:573
  c->substeps++;
  return MPMHIP_OK;
}

int mpmhip_set_overlap(mpmhip_ctx *c, int32_t enabled) {
  if (!c) return MPMHIP_EINVAL;
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "set_overlap inside a substep");
  c->overlap = enabled != 0;
  return MPMHIP_OK;
}

int64_t mpmhip_tiled_run(mpmhip_ctx *c, int64_t n, int64_t until_migration, mpmhip_exchange_fn exchange, void *user) {
  if (!c || n < 0) return MPMHIP_EINVAL;
  if (c->tn.on) return fail(c, MPMHIP_EINVAL, "this ctx has a native plan (mpmhip_tiled_setup): advance it with mpmhip_tiled_advance");
  if (c->T.n_boxes > 0 && !exchange) return fail(c, MPMHIP_EINVAL, "this ctx has halo boxes: tiled_run needs an exchange callback");
  if (c->T.enabled && c->rigid.enabled)
    return fail(c, MPMHIP_EINVAL, "tiled_run: a tiled ctx with rigid bodies advances through the native plan only (mpmhip_tiled_setup, mpmhip_tiled_advance): the callback path does not carry the bodies' impulses");
  if (until_migration > 0 && until_migration < n) n = until_migration;
  for (int64_t i = 0; i < n; i++) {
    int rc = mpmhip_substep_begin(c);
    if (rc) return rc;
    if (c->T.n_boxes > 0) {
      int32_t e = exchange(user, MPMHIP_EXCHANGE_START);
      if (!e && (rc = mpmhip_substep_interior(c))) e = rc;
      if (!e) e = exchange(user, MPMHIP_EXCHANGE_WAIT);
      if (e) {
        c->in_substep = false; c->cur_ev = nullptr;  // (the substep is abandoned: the ctx can be stepped or destroyed again)
        return e < 0 ? e : fail(c, MPMHIP_EINVAL, "tiled_run: the exchange callback returned %d", (int)e);
      }
    }
    if ((rc = mpmhip_substep_end(c))) return rc;
  }
  return n;
}

int mpmhip_substep(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  if (c->T.n_boxes > 0)
    return fail(c, MPMHIP_EINVAL, "this ctx has halo boxes: drive it with substep_begin / exchange / substep_end");
  int rc = mpmhip_substep_begin(c);
  return rc ? rc : mpmhip_substep_end(c);
}

int mpmhip_run_substeps(mpmhip_ctx *c, int32_t n) {
  for (int32_t i = 0; i < n; i++) {
    int rc = mpmhip_substep(c);
    if (rc) return rc;
  }
  return MPMHIP_OK;
}

int mpmhip_step(mpmhip_ctx *c, float dt) {  // MPM<dim>::step, src/mpm.cpp:428-439
  if (!c) return MPMHIP_EINVAL;
  if (dt < 0) {
    int rc = mpmhip_substep(c);
    c->request_t = c->t;
    return rc;
  }
  c->request_t += dt;
  while (c->t + c->P.dt < c->request_t) {
    int rc = mpmhip_substep(c);
    if (rc) return rc;
  }
  return MPMHIP_OK;
}

double mpmhip_current_time(const mpmhip_ctx *c) { return c ? (double)c->t : 0.0; }

int mpmhip_synchronize(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  Counters h;
  return read_counters(c, h);
}

static int ensure_dense(mpmhip_ctx *c, size_t &nodes) {
  nodes = (size_t)(c->P.res[0] + 1) * (c->P.res[1] + 1) * (c->P.res[2] + 1);
  if (!c->dense) {
    if (c->dense.alloc(nodes) != hipSuccess) return fail(c, MPMHIP_ENOMEM, "dense grid staging allocation failed");
  }
  return MPMHIP_OK;
}

int mpmhip_download_grid(mpmhip_ctx *c, int32_t which, float *dst) {
  if (!c || !dst || (which != 0 && which != 1)) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  size_t nodes;
  int rc = ensure_dense(c, nodes);
  if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(c->dense, 0, nodes * sizeof(float4), c->stream));
  if ((rc = do_grid(c, which == 0 ? 1 : 3))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(dst, c->dense, nodes * sizeof(float4), hipMemcpyDeviceToHost));
  return MPMHIP_OK;
}

int mpmhip_upload_grid(mpmhip_ctx *c, const float *src) {
  if (!c || !src) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = need_sorted(c, "upload_grid");
  if (rc) return rc;
  size_t nodes;
  if ((rc = ensure_dense(c, nodes))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->dense, src, nodes * sizeof(float4), hipMemcpyHostToDevice));
  return do_grid(c, 2);
}

int mpmhip_delete_particles_inside_level_set(mpmhip_ctx *c, int64_t *deleted) {
  if (!c || !deleted) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  *deleted = 0;
  if ((c->LS.n <= 0 && !c->LS.sdf.phi0) || c->n_slots == 0) return MPMHIP_OK;
  if (int rc = ensure_b_current(c)) return rc;  // the recovery reads every live record: do it before some die
  Counters before, after;
  if (int rc = read_counters(c, before)) return rc;
  c->P.t = c->t;
  hipLaunchKernelGGL(k_delete_inside_levelset, dim3(particle_grid(c->n_slots)), dim3(256), 0, c->stream, c->P, (RecG *)c->rg,
                     c->LS, c->cnt);
  if (int rc = launch_check(c, "delete_inside_levelset")) return rc;
  if (int rc = read_counters(c, after)) return rc;
  *deleted = (int64_t)after.n_dead - (int64_t)before.n_dead;
  if (*deleted) return invalidate_keys(c);  // key[] still lists the deleted ones: rebuild
  return MPMHIP_OK;
}

// ---------------------------------------------------------------------------------------------- .bgeo frames
int mpmhip_bgeo_size(mpmhip_ctx *c, int32_t verbose, size_t *bytes) {
  if (!c || !bytes) return MPMHIP_EINVAL;
  int64_t n = mpmhip_num_particles(c);
  if (n < 0) return (int)n;
  if (c->rigid.enabled) n += (int64_t)c->rigid.store.h_smp.size();  // the boundary particles of rigid bodies are rows too (type = 1)
  *bytes = bgeo_bytes((uint32_t)n, verbose != 0);
  return MPMHIP_OK;
}

int mpmhip_bgeo_encode(mpmhip_ctx *c, int32_t verbose, void *dst, size_t capacity, size_t *written) {
  if (!c || !dst || !written) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (verbose)
    if (int rc = ensure_b_current(c)) return rc;
  std::vector<uint32_t> order;
  std::vector<int32_t> ids;
  const bool with_rigid = c->rigid.enabled && !c->rigid.store.h_smp.empty();
  if (int rc = bgeo_order(c, order, with_rigid ? &ids : nullptr)) return rc;
  const uint32_t nm = (uint32_t)order.size();  // material particles
  const uint32_t n = nm + (with_rigid ? (uint32_t)c->rigid.store.h_smp.size() : 0u);
  const size_t total = bgeo_bytes(n, verbose != 0);
  int32_t *limits = nullptr;  // async stepping: per-slot (dt_limit, stiffness_limit, cfl_limit) of the particle's block
  if (c->async.enabled && c->async.limits_valid) limits = c->async.d_particle_limits;
  if (total > capacity)
    return fail(c, MPMHIP_ECAPACITY, "bgeo image needs %zu bytes, the buffer holds %zu", total, capacity);
  uint8_t *out = static_cast<uint8_t *>(dst);
  const std::vector<uint8_t> head = bgeo_header(n, verbose != 0);
  std::memcpy(out, head.data(), head.size());
  out += head.size();
  const size_t W = verbose ? BGEO_W_VERBOSE : BGEO_W_PLAIN;
  const size_t row_bytes = (size_t)n * W * 4, mat_bytes = (size_t)nm * W * 4;
  std::vector<uint8_t> mat_rows;  // with rigid bodies the material rows are merged with the boundary particles' by creation id
  uint8_t *mat_dst = out;
  if (with_rigid) { mat_rows.resize(mat_bytes); mat_dst = mat_rows.data(); }
  if (nm) {
    DevBuf<uint32_t> d_order, d_rows;
    HIPCHK(c, d_order.alloc((size_t)nm));
    HIPCHK(c, d_rows.alloc((size_t)nm * W));
    HIPCHK(c, hipMemcpyAsync(d_order, order.data(), (size_t)nm * 4, hipMemcpyHostToDevice, c->stream));
    const dim3 grid(particle_grid(nm)), wg(256);
    if (verbose)
      hipLaunchKernelGGL(k_bgeo_rows<true>, grid, wg, 0, c->stream, nm, (const uint32_t *)d_order, (const RecG *)c->rg,
                         (const RecP *)c->rp, (const float *)c->rb, (const GroupParams *)c->d_groups, (const int32_t *)limits, d_rows);
    else
      hipLaunchKernelGGL(k_bgeo_rows<false>, grid, wg, 0, c->stream, nm, (const uint32_t *)d_order, (const RecG *)c->rg,
                         (const RecP *)c->rp, (const float *)c->rb, (const GroupParams *)c->d_groups, (const int32_t *)limits, d_rows);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(mat_dst, d_rows, mat_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (with_rigid) {
    auto &R = c->rigid;  // (the boundary particles' rows: rigid_setup.h)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<RigidBodyDev> hb(MAX_RIGID);
    HIPCHK(c, hipMemcpy(hb.data(), R.d_rb, sizeof(RigidBodyDev) * MAX_RIGID, hipMemcpyDeviceToHost));
    rigid_setup::merge_rows_by_id(out, W * 4, nm, [&](size_t im) { return ids[im]; }, R.store.h_smp_id,
                                  [&](size_t im, uint8_t *row) { std::memcpy(row, mat_rows.data() + im * W * 4, W * 4); },
                                  [&](size_t ir, uint8_t *row) { rigid_setup::bgeo_boundary_row<3>(R.store, hb.data(), ir, row, W * 4); });
  }
  out = bgeo_put_tail(out + row_bytes, n);
  *written = (size_t)(out - static_cast<uint8_t *>(dst));
  if (*written != total) return fail(c, MPMHIP_EINVAL, "internal: bgeo image is %zu bytes, expected %zu", *written, total);
  return MPMHIP_OK;
}

int mpmhip_write_bgeo(mpmhip_ctx *c, const char *path, int32_t verbose) {
  if (!c || !path) return MPMHIP_EINVAL;
  const size_t len = std::strlen(path);
  if (len >= 3 && std::strcmp(path + len - 3, ".gz") == 0)
    return fail(c, MPMHIP_ENOTIMPL, "gzip-compressed .bgeo (the reference writes plain %%04d.bgeo, src/mpm.h:336)");
  size_t bytes = 0, written = 0;
  if (int rc = mpmhip_bgeo_size(c, verbose, &bytes)) return rc;
  std::vector<uint8_t> img;
  try { img.resize(bytes); } catch (const std::bad_alloc &) { return fail(c, MPMHIP_ENOMEM, "host allocation of %zu bytes failed", bytes); }
  if (int rc = mpmhip_bgeo_encode(c, verbose, img.data(), img.size(), &written)) return rc;
  FILE *f = std::fopen(path, "wb");
  if (!f) return fail(c, MPMHIP_EINVAL, "cannot open '%s' for writing: %s", path, std::strerror(errno));
  const size_t ok = std::fwrite(img.data(), 1, written, f);
  const int cl = std::fclose(f);
  if (ok != written || cl != 0) return fail(c, MPMHIP_EINVAL, "short write to '%s': %s", path, std::strerror(errno));
  return MPMHIP_OK;
}

// MPM<dim>::calculate_energy (src/mpm.cpp:1078-1110): sort + P2G, kinetic energy of the grid, potential energy
// of the particles.  Leaves the ctx sorted with fresh P2G tiles (like the reference, which leaves its grid rasterized).
// calculate_energy (src/mpm.cpp:1078-1110) in two halves, so that a tiled job can put its halo exchange between them:
//   begin  sort, rasterize (P2G) [+ halo pack and the start of the exchange]
//   end    [the peers' sums have arrived] grid kinetic energy, particles' potential energy -> out = {kinetic, potential, particles of
//          a type without potential_energy()}: this ctx's SHARE — on a tiled ctx a node's kinetic energy is counted by the lowest
//          rank that holds mass on it (k_grid mode 4), so the shares add up to the one-ctx energy.
static int energy_begin(mpmhip_ctx *c) {
  int rc;
  c->ov_active = false;
  if ((rc = do_sort(c))) return rc;
  if ((rc = do_p2g(c))) return rc;
  if (c->tn.on && c->T.n_boxes > 0) {
    tn_begin_substep(c);
    if ((rc = do_halo_pack(c))) return rc;
  }
  return MPMHIP_OK;
}
// The deterministic mode stores every partial sum at a canonical place and adds them in a fixed order (k_grid.h: MODE 5,
// k_particles.h: k_potential_energy_sorted, k_sum_fixed): the kinetic energy per node block at its slot 8 a + o, the potential energy
// per wave of a fixed launch over the particles in sorted order.
static int energy_end_det(mpmhip_ctx *c) {
  const size_t mb = c->P.max_blocks;
  if (c->energy_parts_cap < mb) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->energy_parts_cap = 0;
    HIPCHK(c, c->d_energy_parts.alloc(mb * 8 + POT_WAVES));
    c->energy_parts_cap = mb;
  }
  double *kin = c->d_energy_parts, *pot = c->d_energy_parts + 8 * mb, *acc = c->d_energy;
  HIPCHK(c, hipMemsetAsync(kin, 0, 8 * mb * sizeof(double), c->stream));  // (node blocks no walk visits: not owned, not in phase)
  int rc = do_grid(c, 5, 0, reinterpret_cast<float4 *>(kin));  // k_grid<5> stores into its `dense` argument
  if (rc) return rc;
  const uint32_t *n_active = &c->cnt->n_active;
  hipLaunchKernelGGL(k_sum_fixed, dim3(1), dim3(1024), 0, c->stream, (const double *)kin, n_active, (uint32_t)mb, 8u, acc);
  hipLaunchKernelGGL(k_potential_energy_sorted, dim3(POT_WAVES / 4), dim3(256), 0, c->stream, (const Counters *)c->cnt,
                     (const uint32_t *)c->perm, (const RecG *)c->rg, (const GroupParams *)c->d_groups, pot, acc + 2);
  hipLaunchKernelGGL(k_sum_fixed, dim3(1), dim3(1024), 0, c->stream, (const double *)pot, (const uint32_t *)nullptr, POT_WAVES, 1u, acc + 1);
  return launch_check(c, "energy (deterministic)");
}
static int energy_end(mpmhip_ctx *c, double out[3]) {
  int rc;
  if (!c->d_energy) HIPCHK(c, c->d_energy.alloc(4));
  HIPCHK(c, hipMemsetAsync(c->d_energy, 0, 4 * sizeof(double), c->stream));
  if (c->deterministic) {
    if ((rc = energy_end_det(c))) return rc;
  } else {
    if ((rc = do_grid(c, 4, 0, reinterpret_cast<float4 *>(c->d_energy.get())))) return rc;  // k_grid<4> accumulates into its `dense` argument
    hipLaunchKernelGGL(k_potential_energy, dim3(particle_grid(c->n_slots)), dim3(256), 0, c->stream, c->P, (const RecG *)c->rg,
                       (const GroupParams *)c->d_groups, c->d_energy + 1);
    if ((rc = launch_check(c, "potential_energy"))) return rc;
  }
  double *acc = c->d_energy;
  double *h = reinterpret_cast<double *>(c->h_pinned + 12288);  // (pinned: behind the reductions' staging)
  HIPCHK(c, hipMemcpyAsync(h, acc, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < 3; i++) out[i] = h[i];
  return MPMHIP_OK;
}
namespace { int tn_energy(mpmhip_ctx *c, double out[3]); }  // (tiled_api.h: exchange + reduction over the ranks)

int mpmhip_calculate_energy(mpmhip_ctx *c, double *kinetic, double *potential) {
  if (!c || !kinetic || !potential) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "calculate_energy inside a substep");
  double e[3];
  int rc;
  if (c->tn.on && c->tn.world > 1) {  // the whole job's energy: collective over the ranks
    if ((rc = tn_energy(c, e))) return rc;
  } else {
    if (c->T.n_boxes > 0) return fail(c, MPMHIP_ENOTIMPL, "calculate_energy on a ctx tiled through the callback path (mpmhip_set_halo): "
                                      "use the native data plane (mpmhip_tiled_setup), whose calculate_energy covers the whole job");
    if ((rc = energy_begin(c)) || (rc = energy_end(c, e))) return rc;
  }
  *kinetic = e[0];
  *potential = e[1];
  if (e[2] != 0.0)
    return fail(c, MPMHIP_ENOTIMPL, "%.0f particles are of a type without potential_energy() (reference: TC_NOT_IMPLEMENTED); "
                "kinetic energy is valid", e[2]);
  return MPMHIP_OK;
}

int mpmhip_set_profiling(mpmhip_ctx *c, int32_t level) {
  if (!c || level < 0 || level > 4) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "set_profiling inside a substep");
  int rc = collect_events(c);  // pending events belong to the old level
  c->profiling = level;
  c->ev_level = level;
  return rc;
}
int mpmhip_set_profile_sampling(mpmhip_ctx *c, int32_t every) {
  if (!c || every < 1) return MPMHIP_EINVAL;
  c->prof_every = every;
  return MPMHIP_OK;
}
int mpmhip_profile_reset(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = collect_events(c);
  for (int k = 0; k < PH_COUNT; k++) c->phase_ms[k] = 0;
  c->prof_substeps = 0;
  return rc;
}
int mpmhip_profile(mpmhip_ctx *c, char *json, size_t cap) {
  if (!c || !json || cap == 0) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = collect_events(c);
  if (rc) return rc;
  Counters h;
  if ((rc = read_counters(c, h))) return rc;
  int w = snprintf(json, cap,
                   "{\"substeps\":%lld,\"particles\":%lld,\"active_blocks\":%u,\"rank_mode\":%u,\"phases\":{\"sort\":%.6f,\"p2g\":%.6f,"
                   "\"exchange\":%.6f,\"grid\":%.6f,\"g2p\":%.6f}}",
                   (long long)c->prof_substeps, (long long)(c->n_slots - h.n_dead), h.n_active, h.rank_mode, c->phase_ms[PH_SORT],
                   c->phase_ms[PH_P2G], c->phase_ms[PH_EXCH], c->phase_ms[PH_GRID], c->phase_ms[PH_G2P]);
  return (w < 0 || (size_t)w >= cap) ? fail(c, MPMHIP_EINVAL, "profile buffer too small") : MPMHIP_OK;
}

// ------------------------------------------------------------------------------------------------ tiling (host)
int mpmhip_set_partition(mpmhip_ctx *c, int32_t rank, const int32_t dims[3], const int32_t *cuts_x,
                         const int32_t *cuts_y, const int32_t *cuts_z, int32_t margin) {
  if (!c || !dims || !cuts_x || !cuts_y || !cuts_z) return MPMHIP_EINVAL;
  if (c->rigid.col.on) return fail(c, MPMHIP_EINVAL, "rigid_body_collision is not supported on a tiled (multi-GPU) ctx: the bodies of a job meet no other body");
  const int32_t *const cuts[3] = {cuts_x, cuts_y, cuts_z};
  tplan::Partition part;
  const std::string refused = part.init(c->P.res, dims, cuts, margin, rank);
  if (!refused.empty()) return fail(c, MPMHIP_EINVAL, "%s", refused.c_str());
  Tiling T;
  memset(&T, 0, sizeof T);
  memcpy(T.dims, part.dims, sizeof T.dims);
  memcpy(T.cuts, part.cuts, sizeof T.cuts);
  part.brick(rank, T.lo, T.hi);
  T.enabled = 1; T.rank = rank; T.margin = margin;
  c->T = T;  // halo boxes (if any) must be set again
  return MPMHIP_OK;
}

int mpmhip_set_halo(mpmhip_ctx *c, int32_t n, const mpmhip_halo_box *boxes) {
  if (!c || n < 0 || n > MPMHIP_MAX_HALO_BOXES || (n > 0 && !boxes)) return MPMHIP_EINVAL;
  if (n > 0 && !c->T.enabled) return fail(c, MPMHIP_EINVAL, "set_halo needs set_partition first");
  if (c->tn.on) return fail(c, MPMHIP_EINVAL, "this ctx has a native plan (mpmhip_tiled_setup): its halo boxes are the library's");
  if (n > 0 && c->rigid.enabled)
    return fail(c, MPMHIP_EINVAL, "set_halo: a ctx with rigid bodies exchanges its halo through the native plan only (mpmhip_tiled_setup): the callback path does not carry the bodies' impulses");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  Tiling &T = c->T;
  T.n_boxes = 0; T.box_nodes = 0; T.box_blocks = 0;
  if (n == 0) return MPMHIP_OK;
  std::vector<DevBox> hb((size_t)n);
  uint64_t off = 0;
  for (int i = 0; i < n; i++) {
    const mpmhip_halo_box &b = boxes[i];
    if (i > 0 && b.peer < boxes[i - 1].peer) return fail(c, MPMHIP_EINVAL, "halo boxes must be sorted by peer rank");
    if (b.peer == T.rank || !b.send || !b.recv) return fail(c, MPMHIP_EINVAL, "halo box %d: bad peer or null buffer", i);
    for (int a = 0; a < 3; a++) {
      if (b.lo[a] < 0 || b.hi[a] <= b.lo[a] || b.hi[a] > c->P.res[a] + 1) return fail(c, MPMHIP_EINVAL, "halo box %d: bad extent on axis %d", i, a);
      hb[i].lo[a] = b.lo[a]; hb[i].dim[a] = b.hi[a] - b.lo[a];
    }
    hb[i].peer = b.peer; hb[i].off = (uint32_t)off;
    hb[i].send = (float4 *)b.send; hb[i].recv = (const float4 *)b.recv; hb[i].flag = nullptr;
    off += (uint64_t)hb[i].dim[0] * hb[i].dim[1] * hb[i].dim[2];
    if (off >= (1ull << 31)) return fail(c, MPMHIP_EINVAL, "halo boxes too large");
  }
  // node box this rank's particles can touch: base cells in [lo-margin, hi+margin), stencil base..base+2.  KNOWN DIFFERENCE to the
  // native plan (tiled_api.h: tn_apply_plan cuts the interior from the node box the boxes were cut from, clip box and occupancy
  // included): against this uncut box a box of a caller who clips its boxes ends inside an axis and the interior collapses
  // (tests/cpp/tiled_plan_host.cpp: tp_occupancy_cut_interior) — correct, but nothing is left to overlap the exchange with.
  int nlo[3], nhi[3];
  for (int a = 0; a < 3; a++) {
    nlo[a] = std::max(0, T.lo[a] - T.margin);
    nhi[a] = std::min(c->P.res[a] + 1, T.hi[a] + T.margin + 2);
  }
  const tplan::Interior I = tplan::interior(nlo, nhi, boxes, (size_t)n);
  for (int i = 0; i < n; i++) hb[i].boff = I.boff[i];
  for (int a = 0; a < 3; a++) { T.int_lo[a] = I.lo[a]; T.int_hi[a] = I.hi[a]; }
  if (!c->d_boxes) HIPCHK(c, c->d_boxes.alloc((size_t)MPMHIP_MAX_HALO_BOXES));
  HIPCHK(c, hipMemcpy(c->d_boxes, hb.data(), sizeof(DevBox) * n, hipMemcpyHostToDevice));
  c->d_boxes_cur = c->d_boxes;
  T.n_boxes = n; T.box_nodes = (uint32_t)off; T.box_blocks = I.box_blocks;
  return MPMHIP_OK;
}

int mpmhip_halo_pack(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = need_sorted(c, "halo_pack");
  return rc ? rc : do_halo_pack(c);
}

static int ensure_counts(mpmhip_ctx *c, int world) {
  if (!c->T.enabled) return fail(c, MPMHIP_EINVAL, "no partition set");
  if (world != c->T.dims[0] * c->T.dims[1] * c->T.dims[2]) return fail(c, MPMHIP_EINVAL, "world=%d does not match the partition", world);
  if (c->counts_cap < world) {
    HIPCHK(c, c->d_counts.alloc((size_t)world + 8));  // + the 6 bounds and the speed of mpmhip_migration_scan + one word of the native data plane
    c->counts_cap = world;
  }
  return MPMHIP_OK;
}

// one pass over the particles, one synchronisation: leaver counts per destination + bounding box of the base cells
// + the fastest particle (cells per substep)
int mpmhip_migration_scan(mpmhip_ctx *c, int32_t world, int64_t *counts, int32_t lo[3], int32_t hi[3],
                          float *max_cells_per_substep) {
  if (!c || !counts) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = ensure_counts(c, world);
  if (rc) return rc;
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "migration inside a substep");
  if ((size_t)world + 7 + sizeof(Counters) / 4 > 65536 / 4) return fail(c, MPMHIP_EINVAL, "world too large");
  hipLaunchKernelGGL(k_scan_init, dim3((world + 8 + 255) / 256), dim3(256), 0, c->stream, c->d_counts, world, 0u);
  int grid = particle_grid(c->n_slots);
  if (grid > 128) grid = 128;  // few workgroups: 6 same-address atomics each for the bounds
  hipLaunchKernelGGL(k_leaver_count, dim3(grid), dim3(256), 0, c->stream, c->P, c->T, (const float4 *)c->rg.get(),
                     (const float4 *)c->rp.get(), c->d_counts, reinterpret_cast<int *>(c->d_counts + world), c->cnt);
  if ((rc = launch_check(c, "leaver_count"))) return rc;
  uint32_t *h = c->h_pinned + sizeof(Counters) / 4;  // behind the counters read_counters() fetches
  HIPCHK(c, hipMemcpyAsync(h, c->d_counts, sizeof(uint32_t) * ((size_t)world + 7), hipMemcpyDeviceToHost, c->stream));
  Counters hc;
  if ((rc = read_counters(c, hc))) return rc;  // the ONE synchronisation; reports the margin violation
  for (int i = 0; i < world; i++) counts[i] = h[i];
  for (int k = 0; k < 3; k++) {
    if (lo) lo[k] = (int32_t)h[world + k];
    if (hi) hi[k] = (int32_t)h[world + 3 + k];
  }
  if (max_cells_per_substep) std::memcpy(max_cells_per_substep, &h[world + 6], sizeof(float));
  return MPMHIP_OK;
}

int mpmhip_leaver_counts(mpmhip_ctx *c, int32_t world, int64_t *counts) {
  return mpmhip_migration_scan(c, world, counts, nullptr, nullptr, nullptr);
}

int mpmhip_export_leavers(mpmhip_ctx *c, int32_t world, const int64_t *counts, void *dev_records) {
  if (!c || !counts) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = ensure_counts(c, world);
  if (rc) return rc;
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "migration inside a substep");
  std::vector<uint32_t> cur((size_t)world);
  uint64_t off = 0;
  for (int i = 0; i < world; i++) { cur[i] = (uint32_t)off; off += (uint64_t)counts[i]; }
  if (off == 0) return MPMHIP_OK;
  if (!dev_records) return MPMHIP_EINVAL;
  uint32_t *pin = c->h_pinned + 1024;  // stays untouched until the next migration: no synchronisation needed
  memcpy(pin, cur.data(), sizeof(uint32_t) * world);
  HIPCHK(c, hipMemcpyAsync(c->d_counts, pin, sizeof(uint32_t) * world, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_leaver_pack, dim3(particle_grid(c->n_slots)), dim3(256), 0, c->stream, c->P, c->T, (float4 *)c->rg.get(),
                     (const float4 *)c->rp.get(), (const float4 *)c->rb.get(), c->key, c->d_counts, (float4 *)dev_records, c->cnt);
  return launch_check(c, "leaver_pack");
}

int mpmhip_import_particles(mpmhip_ctx *c, int64_t n, const void *dev_records) {
  if (!c || n < 0 || (n > 0 && !dev_records)) return MPMHIP_EINVAL;
  if (n == 0) return MPMHIP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->in_substep || c->rec.sorted()) return fail(c, MPMHIP_EINVAL, "import_particles between sort and G2P");
  if (c->n_slots + n > c->cap)
    return fail(c, MPMHIP_ECAPACITY, "particle capacity exceeded on import: %lld + %lld > %lld (request_compaction or a larger max_particles)",
                (long long)c->n_slots, (long long)n, (long long)c->cap);
  hipLaunchKernelGGL(k_import, dim3(particle_grid(n)), dim3(256), 0, c->stream, c->P, (uint32_t)n, (uint32_t)c->n_slots,
                     (const float4 *)dev_records, (float4 *)c->rg.get(), (float4 *)c->rp.get(), (float4 *)c->rb.get(), c->key, c->blk_flag,
                     c->cnt);
  // discard_apic_b, rows behind RecP.A: what arrived in a record's apic_b row is the sender's stale row, and the pack hands out the
  // places in the buffer by atomics, so WHICH stale row lands at which slot differs from run to run.  Nobody reads a stale row before
  // k_recover_b has rewritten it — except a job's snapshot, which copies the rows as they lie and must be the same bytes in two runs
  // of the deterministic mode: the arrivals' rows are zero.  (Current rows, b_stale off, are kept: they are the particles' apic_b.)
  if (c->rec.b_stale()) HIPCHK(c, hipMemsetAsync(c->rb.get() + (size_t)c->n_slots * BW, 0, (size_t)n * BW * sizeof(float), c->stream));
  set_slots(c, c->n_slots + n);
  c->rec.records_imported();
  return launch_check(c, "import");
}

int mpmhip_active_bounds(mpmhip_ctx *c, int32_t lo[3], int32_t hi[3]) {
  if (!c || !lo || !hi) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->d_bounds) HIPCHK(c, c->d_bounds.alloc(6));
  const int init[6] = {1 << 30, 1 << 30, 1 << 30, -1, -1, -1};
  int h[6];
  HIPCHK(c, hipMemcpyAsync(c->d_bounds, init, sizeof init, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // `init` lives on this stack frame
  hipLaunchKernelGGL(k_active_bounds, dim3(64), dim3(256), 0, c->stream, c->P, (const Counters *)c->cnt,
                     (const uint32_t *)c->act_blk, c->d_bounds);
  int rc = launch_check(c, "active_bounds");
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(h, c->d_bounds, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 3; k++) { lo[k] = h[k]; hi[k] = h[3 + k]; }
  return MPMHIP_OK;
}

int64_t mpmhip_num_slots(mpmhip_ctx *c) { return c ? c->n_slots : MPMHIP_EINVAL; }

int mpmhip_request_compaction(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  c->compact_requested = true;
  return MPMHIP_OK;
}

int64_t mpmhip_capacity(mpmhip_ctx *c) { return c ? c->cap : MPMHIP_EINVAL; }

int mpmhip_reserve(mpmhip_ctx *c, int64_t max_particles) {
  if (!c) return MPMHIP_EINVAL;
  if (max_particles <= c->cap) return MPMHIP_OK;
  if (max_particles >= (1ll << 31)) return fail(c, MPMHIP_EINVAL, "max_particles out of range");
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "reserve inside a substep");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t n = (size_t)c->n_slots, cap = (size_t)max_particles;
  hipError_t e = hipSuccess;
  auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  A(c->rg.regrow(n, cap, false)); A(c->rp.regrow(n, cap, false)); A(c->rb.regrow(n * BW, cap * BW, true));
  A(c->rg2.regrow(0, cap, false)); A(c->rp2.regrow(0, cap, false)); A(c->rb2.regrow(0, cap * BW, false));
  A(c->key.regrow(0, cap, false)); A(c->pidc.regrow(0, cap, false)); A(c->rank.regrow(0, cap, false)); A(c->perm.regrow(0, cap, false)); A(c->chunk_blk.regrow(0, cap / 256 + 2, false));
  if (c->rigid.d_bnd) A(c->rigid.d_bnd.regrow(n, cap, true));
  if (c->async.d_blk_of) {  // (re-allocated at the size of the ctx by the next update_dt_limits)
    c->async.d_blk_of.reset(); c->async.d_particle_limits.reset();
    c->async.blk_of_cap = 0; c->async.limits_valid = false;
  }
  if (e != hipSuccess) return fail(c, MPMHIP_ENOMEM, "growing the particle arrays to %lld failed: %s", (long long)max_particles, hipGetErrorString(e));
  c->cap = max_particles;
  c->cfg.max_particles = max_particles;
  sync_pidc(c);
  if (int rc = clear_block_flags(c, c->rec.index_dropped())) return rc;  // (the next sort rebuilds keys from the records)
  if (c->cfg.max_blocks <= 0) {  // auto-sized block table: same rule as mpmhip_create
    int64_t mb = c->cap / 48 + 4096;
    if (mb > (int64_t)c->NB) mb = c->NB;
    if ((uint32_t)mb > c->P.max_blocks) {
      const size_t m = (size_t)mb;
      A(c->act_blk.regrow(0, m + 1, false)); A(c->act_start.regrow(0, m + 2, true));
      A(c->cell_cnt.regrow(0, m * BC, true)); A(c->cell_start.regrow(0, m * BC + 1, true));
      A(c->nbr.regrow(0, m * 32, false)); A(c->own_list.regrow(0, m * 8, false));
      c->ct_slots = (uint32_t)((m + 15) / 16 + 1);
      A(c->scan_slots.regrow(0, c->bt_slots + 2 * (size_t)c->ct_slots, true));  // (epoch 0 is never used)
      c->list_clear_epoch = c->sort_epoch;
      A(c->tiles.regrow(0, m * TN, false)); A(c->gridv.regrow(0, m * 8 * BC, false));
      if (c->rigid.d_blk_rigid) { A(c->rigid.d_blk_rigid.regrow(0, m + 1, true)); A(c->rigid.d_rigid_list.regrow(0, m + 1, false)); }
      if (c->rigid.d_imp_rows) { A(c->rigid.d_imp_rows.regrow(0, m * IMP_ROW, false)); c->rigid.imp_rows_cap = m; }
      if (e != hipSuccess) return fail(c, MPMHIP_ENOMEM, "growing the block table to %lld failed: %s", (long long)mb, hipGetErrorString(e));
      c->P.max_blocks = (uint32_t)mb;
      HIPCHK(c, hipMemset(c->fat_slot, 0, sizeof(uint32_t) * (size_t)c->NB));  // slots of the old grid array
    }
  }
  return MPMHIP_OK;
}

// the launch bound of the chained scans as a function of what the occupancy API answered (no device needed: scan_grid_for)
int mpmhip_debug_scan_grid(int32_t n_cus, int32_t per_cu, int32_t env_request, uint32_t *limit, uint32_t *resident) {
  if (!limit || !resident || n_cus < 1 || per_cu < 0) return MPMHIP_EINVAL;
  *limit = lp::scan_grid_for(n_cus, per_cu, env_request);
  *resident = lp::scan_resident_set(n_cus, per_cu);
  return MPMHIP_OK;
}
int64_t mpmhip_debug_live_buffers(void) { return hostmem::g_live_buffers.load(std::memory_order_relaxed); }
int mpmhip_debug_g2p_is_packed(const mpmhip_ctx *c) { return c ? (lp::plan_g2p(c->knobs, facts(c), 0).packed ? 1 : 0) : MPMHIP_EINVAL; }
int mpmhip_debug_transfer_plan(const mpmhip_ctx *c, int32_t out[8]) {
  if (!c || !out) return MPMHIP_EINVAL;
  lp::transfer_plan_words(c->knobs, facts(c), out);
  return MPMHIP_OK;
}
// read-only view of what the last do_sort left (include/mpmhip.h): the facts, then one array per call
static int sort_view_counters(mpmhip_ctx *c, Counters &h) {
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->rec.sorted()) return fail(c, MPMHIP_EINVAL, "debug_sort: the particles are not sorted: call mpmhip_sort first");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(&h, c->cnt, sizeof h, hipMemcpyDeviceToHost));  // (not read_counters: the error word is reported, not raised)
  return MPMHIP_OK;
}
int mpmhip_debug_sort_info(mpmhip_ctx *c, int64_t out[MPMHIP_SORT_INFO_WORDS]) {
  if (!c || !out) return MPMHIP_EINVAL;
  Counters h;
  if (int rc = sort_view_counters(c, h)) return rc;
  const auto &s = c->last_sort;
  const int64_t words[MPMHIP_SORT_INFO_WORDS] = {
      c->n_slots, h.n_sorted, h.n_active, h.n_dead, h.error, h.rank_mode, h.n_own, s.keyed ? 1 : 0, s.build_list ? 1 : 0, s.ct,
      s.deterministic ? s.cell_order_form : -1, s.ids_cached ? 1 : 0, c->list_valid ? 1 : 0, c->P.nbw, c->P.max_blocks, c->P.kbits};
  memcpy(out, words, sizeof words);
  return MPMHIP_OK;
}
int64_t mpmhip_debug_sort_array(mpmhip_ctx *c, int32_t which, void *dst, int64_t capacity_bytes) {
  if (!c || (!dst && capacity_bytes > 0) || capacity_bytes < 0) return MPMHIP_EINVAL;
  Counters h;
  if (int rc = sort_view_counters(c, h)) return rc;
  const size_t na = std::min(h.n_active, c->P.max_blocks), ns = std::min<size_t>(h.n_sorted, (size_t)c->n_slots);
  const void *src = nullptr;
  size_t words = 0;
  switch (which) {
    case MPMHIP_SORT_SLOT_ID: words = (size_t)c->n_slots; break;  // (gathered from the records below)
    case MPMHIP_SORT_BITS: src = c->bits.get(); words = c->P.nbw; break;
    case MPMHIP_SORT_WPREFIX: src = c->wprefix.get(); words = c->P.nbw; break;
    case MPMHIP_SORT_ACT_BLK: src = c->act_blk.get(); words = na; break;
    case MPMHIP_SORT_ACT_START: src = c->act_start.get(); words = na + 1; break;
    case MPMHIP_SORT_CELL_START: src = c->cell_start.get(); words = na * BC + 1; break;
    case MPMHIP_SORT_PERM: src = c->perm.get(); words = ns; break;
    case MPMHIP_SORT_NBR: src = c->nbr.get(); words = c->list_valid ? na * 32 : 0; break;
    case MPMHIP_SORT_OWN_LIST: src = c->own_list.get(); words = c->list_valid ? std::min<size_t>(h.n_own, (size_t)c->P.max_blocks * 8) : 0; break;
    case MPMHIP_SORT_CHUNK_BLK: src = c->chunk_blk.get(); words = c->chunk_blk ? (ns + 255) / 256 : 0; break;
    default: return fail(c, MPMHIP_EINVAL, "debug_sort_array: unknown array %d", which);
  }
  const int64_t bytes = (int64_t)(words * sizeof(uint32_t));
  if (bytes > capacity_bytes) return -bytes;
  if (bytes == 0) return 0;
  if (which == MPMHIP_SORT_SLOT_ID) {
    std::vector<RecG> hg(words);
    HIPCHK(c, hipMemcpy(hg.data(), c->rg, sizeof(RecG) * words, hipMemcpyDeviceToHost));
    int32_t *q = (int32_t *)dst;
    for (size_t i = 0; i < words; i++) q[i] = hg[i].pid < 0 ? -1 : hg[i].pid;
  } else {
    HIPCHK(c, hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost));
  }
  return bytes;
}
int mpmhip_debug_copy_bandwidth(mpmhip_ctx *c, size_t bytes, int32_t iters, double *gb_per_s) {
  if (!c || !gb_per_s || iters <= 0 || bytes < 16) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = bytes / 16;
  DevBuf<float4> a, b;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t e = a.alloc(n);
  if (e == hipSuccess) e = b.alloc(n);
  if (e == hipSuccess) e = hipMemsetAsync(a, 0, n * 16, c->stream);
  if (e == hipSuccess) e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  double best = 0.0;
  // best over a few shapes of the same copy (loads in flight per lane, workgroups per CU, store hint): the
  // yardstick should be the best a plain kernel does, not one arbitrary launch shape
  using Kern = void (*)(float4 *, const float4 *, size_t);
  const Kern kerns[] = {k_stream_copy<1, false>, k_stream_copy<4, false>, k_stream_copy<4, true>, k_stream_copy<8, true>};
  const int grids[] = {256 * 4, 256 * 16, 256 * 64};
  for (const Kern &k : kerns)
    for (int g : grids)
      for (int it = 0; e == hipSuccess && it < iters + 1; it++) {  // the first pass of a shape is a warm-up
        hipEventRecord(e0, c->stream);
        hipLaunchKernelGGL(k, dim3(g), dim3(256), 0, c->stream, b, (const float4 *)a, n);
        hipEventRecord(e1, c->stream);
        e = hipEventSynchronize(e1);
        float ms = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess && it > 0 && ms > 0.0f) best = std::max(best, 2.0 * (double)n * 16.0 / (ms * 1e-3) / 1e9);
        if (it == iters && getenv("MPMHIP_BW_VERBOSE"))
          std::fprintf(stderr, "copy variant %d grid %d: %.0f GB/s\n", (int)(&k - kerns), g, 2.0 * (double)n * 16.0 / (ms * 1e-3) / 1e9);
      }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  HIPCHK(c, e);
  *gb_per_s = best;
  return MPMHIP_OK;
}

// 64-byte record gather of known size (calibration of the FETCH_SIZE counter, profiles/calibrate_fetch.py): n (a power
// of two) records read through an index of the given pattern, `iters` launches; *gb_per_s = (64 + 4) n / best time
int mpmhip_debug_gather_bandwidth(mpmhip_ctx *c, int64_t n, int32_t mode, int32_t iters, double *gb_per_s) {
  if (!c || !gb_per_s || iters <= 0 || n < 1024 || (n & (n - 1)) || n > (1ll << 30) || mode < 0 || mode > 2) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<float4> rec, out;
  DevBuf<uint32_t> idx;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  const int grid = 256 * 16;
  hipError_t e = rec.alloc((size_t)n * 4);
  if (e == hipSuccess) e = idx.alloc((size_t)n);
  if (e == hipSuccess) e = out.alloc((size_t)grid * 4);
  if (e == hipSuccess) e = hipMemsetAsync(rec, 0, (size_t)n * 64, c->stream);
  if (e == hipSuccess) e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  double best = 0.0;
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_probe_indices, dim3(4096), dim3(256), 0, c->stream, idx, (uint32_t)n, (int)mode);
    for (int it = 0; e == hipSuccess && it < iters + 1; it++) {
      hipEventRecord(e0, c->stream);
      hipLaunchKernelGGL(k_gather_records_probe, dim3(grid), dim3(256), 0, c->stream, (const float4 *)rec, (const uint32_t *)idx,
                         (uint32_t)n, out);
      hipEventRecord(e1, c->stream);
      e = hipEventSynchronize(e1);
      float ms = 0.0f;
      if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
      if (e == hipSuccess && it > 0 && ms > 0.0f) best = std::max(best, 68.0 * (double)n / (ms * 1e-3) / 1e9);
    }
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  HIPCHK(c, e);
  *gb_per_s = best;
  return MPMHIP_OK;
}

// ------------------------------------------------------------------------------------------------ 2D demo (configs[0])
struct mpmhip_mpm88 {
  mpm88::Params P{};
  int device = 0;
  int64_t n = 0, cap = 0;
  DevBuf<float> x, v, F, C, Jp, grid;
  hipStream_t stream = nullptr;
  std::string err;
};
static thread_local std::string g_mpm88_create_error;
static int fail88(mpmhip_mpm88 *m, int code, const std::string &msg) {
  (m ? m->err : g_mpm88_create_error) = msg;
  return code;
}
#define HIPCHK88(m, call)                                                                                      \
  do {                                                                                                         \
    hipError_t e_ = (call);                                                                                    \
    if (e_ != hipSuccess) return fail88((m), MPMHIP_EHIP, std::string(#call " failed: ") + hipGetErrorString(e_)); \
  } while (0)

const char *mpmhip_mpm88_last_error(const mpmhip_mpm88 *m) { return m ? m->err.c_str() : g_mpm88_create_error.c_str(); }

int mpmhip_mpm88_create(int32_t n_grid, float dt, int32_t plastic, int32_t device, mpmhip_mpm88 **out) {
  if (!out || n_grid < 4 || n_grid > 8192 || !(dt > 0.0f)) return fail88(nullptr, MPMHIP_EINVAL, "mpm88: bad n_grid / dt");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail88(nullptr, MPMHIP_EHIP, "no HIP device available: libmpmhip has no CPU fallback");
  if (device < 0 || device >= ndev) return fail88(nullptr, MPMHIP_EINVAL, "mpm88: no such device");
  mpmhip_mpm88 *m = new (std::nothrow) mpmhip_mpm88;
  if (!m) return fail88(nullptr, MPMHIP_ENOMEM, "host allocation failed");
  m->device = device;
  const float E = 1e4f, nu = 0.2f;  // mls-mpm88.cpp:8-9
  m->P.n = n_grid; m->P.dt = dt; m->P.dx = 1.0f / n_grid; m->P.inv_dx = 1.0f / m->P.dx;
  m->P.mu_0 = E / (2 * (1 + nu)); m->P.lambda_0 = E * nu / ((1 + nu) * (1 - 2 * nu)); m->P.hardening = 10.0f;
  m->P.mass = 1.0f; m->P.vol = 1.0f; m->P.plastic = plastic ? 1 : 0;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = m->grid.alloc((size_t)3 * (n_grid + 1) * (n_grid + 1));
  if (e != hipSuccess) {
    const int rc = fail88(nullptr, MPMHIP_EHIP, std::string("mpm88 create: ") + hipGetErrorString(e));
    mpmhip_mpm88_destroy(m);
    return rc;
  }
  *out = m;
  return MPMHIP_OK;
}

void mpmhip_mpm88_destroy(mpmhip_mpm88 *m) {
  if (!m) return;
  hipSetDevice(m->device);
  if (m->stream) { hipStreamSynchronize(m->stream); hipStreamDestroy(m->stream); }
  delete m;
}

int64_t mpmhip_mpm88_num_particles(const mpmhip_mpm88 *m) { return m ? m->n : MPMHIP_EINVAL; }

int mpmhip_mpm88_add(mpmhip_mpm88 *m, int64_t n, const float *x, const float *v, const float *F, const float *C, const float *Jp) {
  if (!m || n < 0 || (n > 0 && !x)) return MPMHIP_EINVAL;
  if (n == 0) return MPMHIP_OK;
  HIPCHK88(m, hipSetDevice(m->device));
  HIPCHK88(m, hipStreamSynchronize(m->stream));
  const int64_t total = m->n + n;
  if (total > m->cap) {  // grow: new arrays, old contents copied over
    const int64_t cap = std::max<int64_t>(total, 2 * m->cap);
    DevBuf<float> *arrs[5] = {&m->x, &m->v, &m->F, &m->C, &m->Jp};
    const int width[5] = {2, 2, 4, 4, 1};
    for (int a = 0; a < 5; a++) HIPCHK88(m, arrs[a]->regrow((size_t)m->n * width[a], (size_t)cap * width[a], false));
    m->cap = cap;
  }
  std::vector<float> h;
  auto put = [&](float *dst, const float *src, int width, const float *dflt) -> hipError_t {
    if (!src) {
      h.resize((size_t)n * width);
      for (int64_t i = 0; i < n; i++)
        for (int k = 0; k < width; k++) h[(size_t)i * width + k] = dflt[k];
      src = h.data();
    }
    return hipMemcpy(dst + m->n * width, src, sizeof(float) * n * width, hipMemcpyHostToDevice);
  };
  const float zero4[4] = {0, 0, 0, 0}, eye[4] = {1, 0, 0, 1}, one[1] = {1};
  HIPCHK88(m, put(m->x, x, 2, zero4));
  HIPCHK88(m, put(m->v, v, 2, zero4));   // Particle(x, c, v = Vec(0)): F(1), C(0), Jp(1)  (mls-mpm88.cpp:12-13)
  HIPCHK88(m, put(m->F, F, 4, eye));
  HIPCHK88(m, put(m->C, C, 4, zero4));
  HIPCHK88(m, put(m->Jp, Jp, 1, one));
  m->n = total;
  return MPMHIP_OK;
}

int mpmhip_mpm88_advance(mpmhip_mpm88 *m, int32_t steps) {
  if (!m || steps < 0) return MPMHIP_EINVAL;
  HIPCHK88(m, hipSetDevice(m->device));
  const int nn = m->P.n + 1;
  const dim3 pg((unsigned)std::max<int64_t>((m->n + 255) / 256, 1)), gg((unsigned)((nn * nn + 255) / 256)), wg(256);
  for (int s = 0; s < steps; s++) {
    HIPCHK88(m, hipMemsetAsync(m->grid, 0, sizeof(float) * 3 * nn * nn, m->stream));  // :17
    if (m->n)
      hipLaunchKernelGGL(mpm88::k_p2g, pg, wg, 0, m->stream, m->P, m->n, (const float *)m->x, (const float *)m->v,
                         (const float *)m->F, (const float *)m->C, (const float *)m->Jp, m->grid);
    hipLaunchKernelGGL(mpm88::k_grid, gg, wg, 0, m->stream, m->P, m->grid);
    if (m->n)
      hipLaunchKernelGGL(mpm88::k_g2p, pg, wg, 0, m->stream, m->P, m->n, m->x, m->v, m->F, m->C, m->Jp, (const float *)m->grid);
    HIPCHK88(m, hipGetLastError());
  }
  return MPMHIP_OK;
}

int mpmhip_mpm88_download(mpmhip_mpm88 *m, float *x, float *v, float *F, float *C, float *Jp) {
  if (!m) return MPMHIP_EINVAL;
  HIPCHK88(m, hipSetDevice(m->device));
  HIPCHK88(m, hipStreamSynchronize(m->stream));
  float *dst[5] = {x, v, F, C, Jp};
  const float *src[5] = {m->x, m->v, m->F, m->C, m->Jp};
  const int width[5] = {2, 2, 4, 4, 1};
  for (int a = 0; a < 5; a++)
    if (dst[a] && m->n) HIPCHK88(m, hipMemcpy(dst[a], src[a], sizeof(float) * m->n * width[a], hipMemcpyDeviceToHost));
  return MPMHIP_OK;
}

int mpmhip_mpm88_download_grid(mpmhip_mpm88 *m, float *grid) {
  if (!m || !grid) return MPMHIP_EINVAL;
  HIPCHK88(m, hipSetDevice(m->device));
  HIPCHK88(m, hipStreamSynchronize(m->stream));
  const int nn = m->P.n + 1;
  HIPCHK88(m, hipMemcpy(grid, m->grid, sizeof(float) * 3 * nn * nn, hipMemcpyDeviceToHost));
  return MPMHIP_OK;
}

// ------------------------------------------------------------------------------------------------ AsyncMPM (first half)
// Block-local time-step limits of the reference's asynchronous stepper (src/async/async_mpm.{h,cpp}): the per-block
// reduction over the particles runs on the device, the block state machine (power-of-two limits, :112-164) on the host.
int mpmhip_async_enable(mpmhip_ctx *c, const mpmhip_async_config *cfg) {
  if (!c || !cfg) return MPMHIP_EINVAL;
  if (!(cfg->unit_delta_t > 0) || cfg->max_units < 1) return fail(c, MPMHIP_EINVAL, "unit_delta_t > 0 and max_units >= 1 required");
  if (rigid_active(c) || c->rigid.enabled) return fail(c, MPMHIP_EINVAL, "asynchronous stepping cannot be combined with rigid bodies");
  if (c->rigid.col.on) return fail(c, MPMHIP_EINVAL, "rigid_body_collision: asynchronous stepping has no rigid bodies");
  if (c->T.enabled) return fail(c, MPMHIP_EINVAL, "asynchronous stepping cannot be combined with the multi-GPU tiling");
  HIPCHK(c, hipSetDevice(c->device));
  auto &A = c->async;
  A.sched_enable(3, c->P.res, *cfg);
  const size_t nblk = A.nblk();
  HIPCHK(c, A.d_tab.alloc(3 * nblk));
  HIPCHK(c, A.d_blk_limits.alloc(3 * nblk));
  A.enabled = true; A.limits_valid = false;
  return MPMHIP_OK;
}

static int async_ensure_particle_arrays(mpmhip_ctx *c) {
  auto &A = c->async;
  if (A.blk_of_cap < c->cap) {
    HIPCHK(c, A.d_blk_of.alloc((size_t)c->cap));
    HIPCHK(c, A.d_particle_limits.alloc(3 * (size_t)c->cap));
    A.blk_of_cap = c->cap;
  }
  return MPMHIP_OK;
}
static int async_reset_table(mpmhip_ctx *c) {
  // (min allowed dt, max |v|^2, count) per block: min starts at the bits of 0.1f (":104 min_allowed_dt = 0.1"), max at 1e-16f
  auto &A = c->async;
  const size_t nblk = A.strength.size();
  std::vector<uint32_t> init(3 * nblk);
  const float f01 = 0.1f, fv = 1e-16f;
  uint32_t b01, bv;
  memcpy(&b01, &f01, 4); memcpy(&bv, &fv, 4);
  for (size_t b = 0; b < nblk; b++) { init[3 * b] = b01; init[3 * b + 1] = bv; init[3 * b + 2] = 0; }
  HIPCHK(c, hipMemcpyAsync(A.d_tab, init.data(), sizeof(uint32_t) * 3 * nblk, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // (`init` lives on this stack frame)
  return MPMHIP_OK;
}
// the reduced table -> the block state machine of AsyncMPM<dim>::update_dt_limits (AsyncSched::limits_from_table): async_api.h
extern "C++" {
namespace {
template <class Ctx> int async_limits_from_table(Ctx *c);
}
}

int mpmhip_async_update_dt_limits(mpmhip_ctx *c) {  // AsyncMPM<dim>::update_dt_limits, src/async/async_mpm.cpp:90-164
  if (!c) return MPMHIP_EINVAL;
  auto &A = c->async;
  if (!A.enabled) return fail(c, MPMHIP_EINVAL, "mpmhip_async_enable first");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nblk = A.strength.size();
  if (int rc = async_ensure_particle_arrays(c)) return rc;
  if (int rc = async_reset_table(c)) return rc;
  hipLaunchKernelGGL(k_async_block_reduce, dim3(particle_grid(c->n_slots)), dim3(256), 0, c->stream, c->P, (const RecG *)c->rg,
                     (const RecP *)c->rp, (const GroupParams *)c->d_groups, A.nb[0], A.nb[1], A.nb[2], A.d_tab, A.d_blk_of);
  if (int rc = launch_check(c, "async_block_reduce")) return rc;
  if (int rc = async_limits_from_table(c)) return rc;
  // what the frame output shows per particle (src/async/async_visualize.cpp:17-26)
  std::vector<int32_t> lim(3 * nblk);
  for (size_t b = 0; b < nblk; b++) { lim[3 * b] = (int32_t)A.continuous[b]; lim[3 * b + 1] = (int32_t)A.strength[b]; lim[3 * b + 2] = (int32_t)A.cfl[b]; }
  HIPCHK(c, hipMemcpy(A.d_blk_limits, lim.data(), sizeof(int32_t) * 3 * nblk, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_async_particle_limits, dim3(particle_grid(c->n_slots)), dim3(256), 0, c->stream, c->P,
                     (const uint32_t *)A.d_blk_of, (const int32_t *)A.d_blk_limits, A.d_particle_limits);
  if (int rc = launch_check(c, "async_particle_limits")) return rc;
  A.limits_valid = true;
  return MPMHIP_OK;
}

// non-empty scheduler blocks: corner node (3 ints), strength / cfl / continuous limits, particle count.  Returns the number.
int64_t mpmhip_async_blocks(mpmhip_ctx *c, int64_t capacity, int32_t *coord, int64_t *strength, int64_t *cfl, int64_t *continuous,
                            int64_t *count, int64_t min_max[2]) {
  if (!c || !c->async.enabled) return MPMHIP_EINVAL;
  auto &A = c->async;
  int64_t n = 0;
  for (int bx = 0; bx < A.nb[0]; bx++)
    for (int by = 0; by < A.nb[1]; by++)
      for (int bz = 0; bz < A.nb[2]; bz++) {
        const size_t b = ((size_t)bx * A.nb[1] + by) * A.nb[2] + bz;
        if (!A.count[b]) continue;
        if (n >= capacity) return fail(c, MPMHIP_ECAPACITY, "block buffer too small");
        if (coord) { coord[3 * n] = bx * 4; coord[3 * n + 1] = by * 4; coord[3 * n + 2] = bz * 8; }
        if (strength) strength[n] = A.strength[b];
        if (cfl) cfl[n] = A.cfl[b];
        if (continuous) continuous[n] = A.continuous[b];
        if (count) count[n] = A.count[b];
        n++;
      }
  if (min_max) { min_max[0] = A.min_delta_t_int; min_max[1] = A.max_delta_t_int; }
  return n;
}

// dense view of the block table: nb[3] blocks per axis (block b = (bx nb[1] + by) nb[2] + bz), limits of EVERY block
int64_t mpmhip_async_table(mpmhip_ctx *c, int32_t nb[3], int64_t capacity, int64_t *strength, int64_t *cfl, int64_t *continuous,
                           int64_t *count) {
  if (!c || !c->async.enabled || !nb) return MPMHIP_EINVAL;
  auto &A = c->async;
  for (int k = 0; k < 3; k++) nb[k] = A.nb[k];
  const int64_t n = (int64_t)A.continuous.size();
  if (capacity < n) return n;  // (query of the size)
  for (int64_t b = 0; b < n; b++) {
    if (strength) strength[b] = A.strength[b];
    if (cfl) cfl[b] = A.cfl[b];
    if (continuous) continuous[b] = A.continuous[b];
    if (count) count[b] = A.count[b];
  }
  return n;
}

int mpmhip_async_set_time_int(mpmhip_ctx *c, int64_t t_int) {
  if (!c || !c->async.enabled || t_int < 0) return MPMHIP_EINVAL;
  c->async.current_t_int = t_int;
  return MPMHIP_OK;
}

int mpmhip_debug_allowed_dt(mpmhip_ctx *c, int32_t material, const float params[MPMHIP_NPARAM], int64_t n, const float *F,
                            const float *aux, const float *v, float dx, float *out) {
  if (!c || n <= 0) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  GroupParams g;
  if (material < MPMHIP_VISCO || material > MPMHIP_ELASTIC) return fail(c, MPMHIP_EINVAL, "unknown material id %d", material);
  memset(&g, 0, sizeof g);
  memcpy(g.p, params, sizeof g.p);
  g.type = material;
  DevBuf<float> dF, dA, dV, dO;
  HIPCHK(c, dF.alloc(9 * n)); HIPCHK(c, dA.alloc(n)); HIPCHK(c, dV.alloc(3 * n)); HIPCHK(c, dO.alloc(n));
  HIPCHK(c, hipMemcpy(dF, F, sizeof(float) * 9 * n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dA, aux, sizeof(float) * n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dV, v, sizeof(float) * 3 * n, hipMemcpyHostToDevice));
  int rc = run_debug(c, k_debug_allowed_dt, g, n, (const float *)dF, (const float *)dA, (const float *)dV, dx, dO.get());
  if (!rc) HIPCHK(c, hipMemcpy(out, dO, sizeof(float) * n, hipMemcpyDeviceToHost));
  return rc;
}

// ------------------------------------------------------------------------------------------------ MPM<2>
// The reference's 2D simulation (create_simulation2('mpm') -> MPM<2>, which runs the generic transfer path): its own small
// object — SoA particle arrays, dense (res+1)^2 grid — see k_mpm2d.h.
struct mpmhip2d_ctx {
  mpm2d::Params P{};
  LevelSetDev LS{};
  SdfFrames sdf;  // mpmhip2d_set_levelset_sdf: the installed sampled level set's key frames (LS.n == 0 while it is installed)
  int device = 0;
  int64_t n = 0, cap = 0;
  DevBuf<float> x, v, F, B, aux, grid;
  DevBuf<int32_t> gid, pid;
  DevBuf<unsigned int> n_dead;
  DevBuf<GroupParams> d_groups;
  std::vector<GroupParams> groups;
  int32_t next_pid = 0;
  float t = 0.0f, request_t = 0.0f;
  hipStream_t stream = nullptr;
  std::string err;
  // CPIC rigid bodies (k_rigid2d.h): segments, boundary particles, dense colored distance field
  bool rigid_enabled = false;
  rigid_setup::Store<2> rigid;  // the bodies' host records, boundary particles (+ creation ids) and elements
  DevBuf<mpm2d::Rigid2> d_rb;
  DevBuf<mpm2d::Sample2> d_smp;
  DevBuf<float> d_elems;
  DevBuf<unsigned long long> d_mind;
  DevBuf<uint32_t> d_tags, d_states;
  DevBuf<mpm2d::Bnd2> d_bnd;
  float penalty = 0.0f, pushing_force = 20000.0f;
  // rigid_body_levelset_collision: the boundary particles' order (see k2_ls_keys)
  bool ls_collision = false;
  DevBuf<uint32_t> d_smp_rank, d_ls_vals[2];
  uint32_t n_ranked = 0, ls_cap = 0;
  DevBuf<unsigned long long> d_ls_keys[2];
  DevBuf<uint8_t> d_ls_tmp;
  size_t ls_tmp_bytes = 0;
  mpm2d::Joints2 joints{};     // MPM<2>::articulations ('rotation' joints)
  int joint_iterations = 100;  // 'articulation_iterations'
  float base_dt = 0.0f;        // the configured "base_delta_t" (P.dt is what the next substep uses: the async stepper sets it per advance)
  // deterministic mode (mpmhip2d_config.deterministic, k_mpm2d_det.h): the cell sort's counters and index, the staged P2G
  // records, the impulse rows; allocated when the mode is first used (det2_reserve), freed with the ctx
  struct Det2 {
    bool on = false;
    int64_t cap = 0;                 // particles the per-particle arrays hold
    DevBuf<uint32_t> count, start;   // [nodes + 1]; start[nodes] = live particles
    DevBuf<uint32_t> off, unordered, idx;
    DevBuf<int32_t> key;
    DevBuf<float4> rec;              // [3 cap]
    DevBuf<float> rows;              // [ceil(cap / 256)][DET_ROW]; entries behind 3 * bodies are never written nor read
    DevBuf<uint8_t> scan_tmp;
    size_t scan_bytes = 0;
  } det;
  AsyncResident async;  // AsyncMPM<2> (async_api.h): the block scheduler + the device store of pool / backup containers
  SeedWork seed;  // mpmhip2d_seed_particles (seed_api.h): the tile and the work buffers of the candidate passes
};
static int async_drop_view(mpmhip2d_ctx *m);
int mpmhip2d_async_step(mpmhip2d_ctx *m, float dt);
static void det2_free(mpmhip2d_ctx *m) {  // a failed det2_reserve leaves nothing half-allocated
  const bool on = m->det.on;
  m->det = mpmhip2d_ctx::Det2();
  m->det.on = on;
}
static thread_local std::string g_2d_create_error;
static int fail2d(mpmhip2d_ctx *m, int code, const std::string &msg) {
  (m ? m->err : g_2d_create_error) = msg;
  return code;
}
#define HIPCHK2D(m, call)                                                                                      \
  do {                                                                                                         \
    hipError_t e_ = (call);                                                                                    \
    if (e_ != hipSuccess) return fail2d((m), MPMHIP_EHIP, std::string(#call " failed: ") + hipGetErrorString(e_)); \
  } while (0)

// the particle arrays of the 2D object hold at least `need` particles (its first m->n stay)
static int a2_grow_particles(mpmhip2d_ctx *m, int64_t need) {
  if (need <= m->cap) return MPMHIP_OK;
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  const size_t cap = (size_t)need + (size_t)need / 2 + 1024, keep = (size_t)m->n;
  hipError_t e = hipSuccess;
  auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  A(m->x.regrow(2 * keep, 2 * cap, false)); A(m->v.regrow(2 * keep, 2 * cap, false)); A(m->F.regrow(4 * keep, 4 * cap, false));
  A(m->B.regrow(4 * keep, 4 * cap, false)); A(m->aux.regrow(keep, cap, false)); A(m->gid.regrow(keep, cap, false));
  A(m->pid.regrow(keep, cap, false));
  if (e != hipSuccess) return fail2d(m, MPMHIP_ENOMEM, std::string("growing the particle arrays failed: ") + hipGetErrorString(e));
  m->cap = (int64_t)cap;
  return MPMHIP_OK;
}
// the same for any 2D object (a snapshot larger than max_particles): the per-particle arrays of the CPIC coupling grow with them
static int a2_grow_particles_any(mpmhip2d_ctx *m, int64_t need) {
  if (need <= m->cap) return MPMHIP_OK;
  const size_t keep = (size_t)m->n;
  if (int rc = a2_grow_particles(m, need)) return rc;
  if (m->rigid_enabled) {
    hipError_t e = m->d_states.regrow(keep, (size_t)m->cap, true);
    if (e == hipSuccess) e = m->d_bnd.regrow(keep, (size_t)m->cap, true);
    if (e != hipSuccess) return fail2d(m, MPMHIP_ENOMEM, std::string("growing the particle arrays failed: ") + hipGetErrorString(e));
  }
  return MPMHIP_OK;
}

const char *mpmhip2d_last_error(const mpmhip2d_ctx *m) { return m ? m->err.c_str() : g_2d_create_error.c_str(); }

int mpmhip2d_create(const mpmhip2d_config *cfg, mpmhip2d_ctx **out) {
  if (!cfg || !out) return fail2d(nullptr, MPMHIP_EINVAL, "null argument");
  *out = nullptr;
  for (int k = 0; k < 2; k++)
    if (cfg->res[k] < 8 || cfg->res[k] > 16384) return fail2d(nullptr, MPMHIP_EINVAL, "res outside [8,16384]");
  if (!(cfg->dx > 0) || !(cfg->dt >= 0) || cfg->max_particles <= 0) return fail2d(nullptr, MPMHIP_EINVAL, "dx > 0, dt >= 0, max_particles > 0 required");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail2d(nullptr, MPMHIP_EHIP, "no HIP device available (libmpmhip has no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail2d(nullptr, MPMHIP_EINVAL, "no such device");
  mpmhip2d_ctx *m = new (std::nothrow) mpmhip2d_ctx;
  if (!m) return fail2d(nullptr, MPMHIP_ENOMEM, "host allocation failed");
  m->device = cfg->device;
  mpm2d::Params &P = m->P;
  P.res[0] = cfg->res[0]; P.res[1] = cfg->res[1];
  P.dx = cfg->dx; P.idx = 1.0f / cfg->dx; P.dt = cfg->dt; P.t = 0.0f;
  m->base_dt = cfg->dt;
  P.g[0] = cfg->gravity[0]; P.g[1] = cfg->gravity[1];
  P.particle_gravity = cfg->particle_gravity; P.apic_damping = cfg->apic_damping; P.rpic_damping = cfg->rpic_damping;
  P.clean_boundary = cfg->clean_boundary; P.particle_collision = cfg->particle_collision; P.clamp_pos = 1;
  m->det.on = cfg->deterministic != 0;
  if (const char *e = getenv("MPMHIP_DETERMINISTIC")) m->det.on = atoi(e) != 0;
  memset(&m->LS, 0, sizeof m->LS);
  m->cap = cfg->max_particles;
  const size_t c = (size_t)m->cap, nodes = (size_t)(P.res[0] + 1) * (P.res[1] + 1);
  hipError_t e = hipSetDevice(m->device);
  auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  A(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
  A(m->x.alloc(2 * c)); A(m->v.alloc(2 * c)); A(m->F.alloc(4 * c)); A(m->B.alloc(4 * c)); A(m->aux.alloc(c));
  A(m->gid.alloc(c)); A(m->pid.alloc(c)); A(m->grid.alloc(3 * nodes)); A(m->n_dead.alloc(1));
  A(m->d_groups.alloc((size_t)MPMHIP_MAX_GROUPS));
  if (e == hipSuccess) e = hipMemset(m->n_dead, 0, sizeof(unsigned int));
  if (e != hipSuccess) {
    const int rc = fail2d(nullptr, MPMHIP_ENOMEM, std::string("mpmhip2d_create: ") + hipGetErrorString(e));
    mpmhip2d_destroy(m);
    return rc;
  }
  *out = m;
  return MPMHIP_OK;
}

void mpmhip2d_destroy(mpmhip2d_ctx *m) {
  if (!m) return;
  hipSetDevice(m->device);
  if (m->stream) { hipStreamSynchronize(m->stream); hipStreamDestroy(m->stream); }
  delete m;  // (the members free their arrays on the device set above)
}

// level set in the plane: the shapes of mpmhip_shape with z ignored (plane = line n.x + d, sphere = disc, cuboid = box with
// p[2], p[5] spanning z = 0); two key frames like mpmhip_set_levelset_keyframes when n1 >= 0
int mpmhip2d_set_levelset(mpmhip2d_ctx *m, int32_t n0, const mpmhip_shape *shapes0, int32_t n1, const mpmhip_shape *shapes1,
                          float t0, float t1, float friction) {
  if (!m || n0 < 0 || n0 > MPMHIP_MAX_SHAPES || n1 > MPMHIP_MAX_SHAPES || (n0 > 0 && !shapes0) || (n1 > 0 && !shapes1)) return MPMHIP_EINVAL;
  if (n1 >= 0 && !(t1 > t0)) return fail2d(m, MPMHIP_EINVAL, "key frame times must satisfy t0 < t1");
  HIPCHK2D(m, hipSetDevice(m->device));
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  LevelSetDev &L = m->LS;
  m->sdf.release();  // shapes replace a sampled set: nothing of it survives
  memset(&L, 0, sizeof L);
  L.n = n0; L.friction = friction; L.dynamic = n1 >= 0; L.n1 = n1 >= 0 ? n1 : 0; L.t0 = t0; L.t1 = t1;
  auto put = [](ShapeDev &d, const mpmhip_shape &s) {
    d.type = s.type; d.inside_out = s.inside_out;
    for (int k = 0; k < 6; k++) d.p[k] = s.p[k];
    if (s.type == 2) { d.p[2] = -1e30f; d.p[5] = 1e30f; }  // a box in the plane: unbounded along z
    if (s.type == 1) d.p[2] = 0.0f;
    if (s.type == 0) d.p[2] = 0.0f;
  };
  for (int i = 0; i < n0; i++) put(L.s[i], shapes0[i]);
  for (int i = 0; i < L.n1; i++) put(L.s1[i], shapes1[i]);
  return MPMHIP_OK;
}

// Sampled level set in the plane: see include/mpmhip.h.  The arrays are copied into device memory the ctx owns; a call with the
// lattice size of the installed set (the per-frame update of a dynamic level set) reuses that memory.
int mpmhip2d_set_levelset_sdf(mpmhip2d_ctx *m, const mpmhip2d_sdf_desc *d, const float *phi0, const float *phi1, float t0, float t1,
                              float friction) {
  if (!m) return MPMHIP_EINVAL;
  if (!d || !phi0) return fail2d(m, MPMHIP_EINVAL, "set_levelset_sdf: the lattice description and the first key frame are required");
  std::string why;
  const size_t count = sdf_lattice::check<2>(d->res, d->origin, d->spacing, why);
  if (!count) return fail2d(m, MPMHIP_EINVAL, "set_levelset_sdf: " + why);
  if (phi1 && !(t1 > t0)) return fail2d(m, MPMHIP_EINVAL, "key frame times must satisfy t0 < t1");
  if (m->ls_collision) return fail2d(m, MPMHIP_EINVAL, "rigid_body_levelset_collision is not supported with a sampled level set");
  HIPCHK2D(m, hipSetDevice(m->device));
  HIPCHK2D(m, hipStreamSynchronize(m->stream));  // (kernels in flight read the arrays)
  LevelSetDev &L = m->LS;
  HIPCHK2D(m, m->sdf.reserve(L.sdf, count, phi1 != nullptr));
  if (!phi1) m->sdf.frame[1].reset();  // a static set keeps no second frame (a dynamic set's per-frame update always brings two)
  HIPCHK2D(m, hipMemcpy(m->sdf.frame[0], phi0, sizeof(float) * count, hipMemcpyHostToDevice));
  if (phi1) HIPCHK2D(m, hipMemcpy(m->sdf.frame[1], phi1, sizeof(float) * count, hipMemcpyHostToDevice));
  const int dirichlet = L.dirichlet, pc = L.particle_collision;
  memset(&L, 0, sizeof L);  // the sampled set replaces the shapes
  L.dirichlet = dirichlet; L.particle_collision = pc;
  L.friction = friction;
  sdf_fill<2>(L.sdf, *d, m->sdf.frame[0], phi1 ? m->sdf.frame[1].get() : nullptr, t0, t1);
  return MPMHIP_OK;
}

// the device's level-set evaluation at host-given points (tests)
int mpmhip2d_debug_levelset_sample(mpmhip2d_ctx *m, int64_t n, const float *pos, float t, float *phi, float *grad, float *dphidt,
                                   int32_t *hit) {
  if (!m || n <= 0 || !pos || !phi || !grad || !dphidt || !hit) return MPMHIP_EINVAL;
  HIPCHK2D(m, hipSetDevice(m->device));
  DevBuf<float> dP, dO;
  HIPCHK2D(m, dP.alloc(2 * (size_t)n));
  HIPCHK2D(m, dO.alloc(5 * (size_t)n));
  HIPCHK2D(m, hipMemcpyAsync(dP, pos, sizeof(float) * 2 * n, hipMemcpyHostToDevice, m->stream));
  hipLaunchKernelGGL(mpm2d::k2_debug_levelset_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->stream, m->LS, t, m->P.idx, n,
                     (const float *)dP, dO.get(), dO + n, dO + 3 * n, reinterpret_cast<int32_t *>(dO + 4 * n));
  HIPCHK2D(m, hipGetLastError());
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  HIPCHK2D(m, hipMemcpy(phi, dO, sizeof(float) * n, hipMemcpyDeviceToHost));
  HIPCHK2D(m, hipMemcpy(grad, dO + n, sizeof(float) * 2 * n, hipMemcpyDeviceToHost));
  HIPCHK2D(m, hipMemcpy(dphidt, dO + 3 * n, sizeof(float) * n, hipMemcpyDeviceToHost));
  HIPCHK2D(m, hipMemcpy(hit, dO + 4 * n, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  return MPMHIP_OK;
}

// the device's 2D constitutive math at host-given rows (tests; k_debug2d.h)
static int debug2d_group(mpmhip2d_ctx *m, int32_t material, const float *params, GroupParams &g) {
  if (material < MPMHIP_VISCO || material > MPMHIP_ELASTIC) return fail2d(m, MPMHIP_EINVAL, "unknown material id " + std::to_string(material));
  memset(&g, 0, sizeof g);
  memcpy(g.p, params, sizeof g.p);
  g.type = material;
  return MPMHIP_OK;
}
static unsigned debug2d_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 1024); }  // grid-stride beyond

int mpmhip2d_debug_force(mpmhip2d_ctx *m, int32_t material, const float params[MPMHIP_NPARAM], int64_t n, const float *F,
                         const float *aux, float *out) {
  if (!m || n < 0 || !params || !F || !aux || !out) return MPMHIP_EINVAL;
  GroupParams g;
  int rc = debug2d_group(m, material, params, g);
  if (rc || n == 0) return rc;
  HIPCHK2D(m, hipSetDevice(m->device));
  DevBuf<float> dF, dA, dO;
  HIPCHK2D(m, dF.alloc(4 * (size_t)n)); HIPCHK2D(m, dA.alloc((size_t)n)); HIPCHK2D(m, dO.alloc(4 * (size_t)n));
  HIPCHK2D(m, hipMemcpyAsync(dF, F, sizeof(float) * 4 * n, hipMemcpyHostToDevice, m->stream));
  HIPCHK2D(m, hipMemcpyAsync(dA, aux, sizeof(float) * n, hipMemcpyHostToDevice, m->stream));
  hipLaunchKernelGGL(mpm2d::k2_debug_force, dim3(debug2d_blocks(n)), dim3(256), 0, m->stream, g, n, (const float *)dF, (const float *)dA,
                     dO.get());
  HIPCHK2D(m, hipGetLastError());
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  HIPCHK2D(m, hipMemcpy(out, dO, sizeof(float) * 4 * n, hipMemcpyDeviceToHost));
  return MPMHIP_OK;
}

int mpmhip2d_debug_plasticity(mpmhip2d_ctx *m, int32_t material, const float params[MPMHIP_NPARAM], int64_t n, const float *cdg,
                              float *F, float *aux, float *force_out) {
  if (!m || n < 0 || !params || !cdg || !F || !aux) return MPMHIP_EINVAL;
  GroupParams g;
  int rc = debug2d_group(m, material, params, g);
  if (rc || n == 0) return rc;
  HIPCHK2D(m, hipSetDevice(m->device));
  DevBuf<float> dC, dF, dA, dO;
  HIPCHK2D(m, dC.alloc(4 * (size_t)n)); HIPCHK2D(m, dF.alloc(4 * (size_t)n)); HIPCHK2D(m, dA.alloc((size_t)n));
  if (force_out) HIPCHK2D(m, dO.alloc(4 * (size_t)n));
  HIPCHK2D(m, hipMemcpyAsync(dC, cdg, sizeof(float) * 4 * n, hipMemcpyHostToDevice, m->stream));
  HIPCHK2D(m, hipMemcpyAsync(dF, F, sizeof(float) * 4 * n, hipMemcpyHostToDevice, m->stream));
  HIPCHK2D(m, hipMemcpyAsync(dA, aux, sizeof(float) * n, hipMemcpyHostToDevice, m->stream));
  hipLaunchKernelGGL(mpm2d::k2_debug_plasticity, dim3(debug2d_blocks(n)), dim3(256), 0, m->stream, g, n, (const float *)dC, dF.get(),
                     dA.get(), force_out ? dO.get() : (float *)nullptr);
  HIPCHK2D(m, hipGetLastError());
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  HIPCHK2D(m, hipMemcpy(F, dF, sizeof(float) * 4 * n, hipMemcpyDeviceToHost));
  HIPCHK2D(m, hipMemcpy(aux, dA, sizeof(float) * n, hipMemcpyDeviceToHost));
  if (force_out) HIPCHK2D(m, hipMemcpy(force_out, dO, sizeof(float) * 4 * n, hipMemcpyDeviceToHost));
  return MPMHIP_OK;
}

int mpmhip2d_debug_svd2(mpmhip2d_ctx *m, int64_t n, const float *F, float *cu, float *su, float *S) {
  if (!m || n < 0 || !F || !cu || !su || !S) return MPMHIP_EINVAL;
  if (n == 0) return MPMHIP_OK;
  HIPCHK2D(m, hipSetDevice(m->device));
  DevBuf<float> dF, dO;
  HIPCHK2D(m, dF.alloc(4 * (size_t)n)); HIPCHK2D(m, dO.alloc(4 * (size_t)n));
  HIPCHK2D(m, hipMemcpyAsync(dF, F, sizeof(float) * 4 * n, hipMemcpyHostToDevice, m->stream));
  hipLaunchKernelGGL(mpm2d::k2_debug_svd, dim3(debug2d_blocks(n)), dim3(256), 0, m->stream, n, (const float *)dF, dO.get(), dO + n, dO + 2 * n);
  HIPCHK2D(m, hipGetLastError());
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  HIPCHK2D(m, hipMemcpy(cu, dO, sizeof(float) * n, hipMemcpyDeviceToHost));
  HIPCHK2D(m, hipMemcpy(su, dO + n, sizeof(float) * n, hipMemcpyDeviceToHost));
  HIPCHK2D(m, hipMemcpy(S, dO + 2 * n, sizeof(float) * 2 * n, hipMemcpyDeviceToHost));
  return MPMHIP_OK;
}

int mpmhip2d_delete_particles_inside_level_set(mpmhip2d_ctx *m, int64_t *deleted) {
  if (!m || !deleted) return MPMHIP_EINVAL;
  *deleted = 0;
  if (m->async.resident) return fail2d(m, MPMHIP_EINVAL, "delete_particles_inside_level_set: not on a resident asynchronous stepper");
  if ((m->LS.n <= 0 && !m->LS.sdf.phi0) || m->n == 0) return MPMHIP_OK;
  HIPCHK2D(m, hipSetDevice(m->device));
  unsigned int before = 0, after = 0;
  HIPCHK2D(m, hipMemcpyAsync(&before, m->n_dead, sizeof before, hipMemcpyDeviceToHost, m->stream));
  m->P.t = m->t;
  hipLaunchKernelGGL(mpm2d::k2_delete_inside, dim3((unsigned)((m->n + 255) / 256)), dim3(256), 0, m->stream, m->P, m->LS, m->n,
                     (const float *)m->x, m->pid.get(), m->n_dead.get());
  HIPCHK2D(m, hipGetLastError());
  HIPCHK2D(m, hipMemcpyAsync(&after, m->n_dead, sizeof after, hipMemcpyDeviceToHost, m->stream));
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  *deleted = (int64_t)after - (int64_t)before;
  return MPMHIP_OK;
}

int mpmhip2d_set_dirichlet(mpmhip2d_ctx *m, int32_t enabled, float distance_left, float distance_right, float velocity_left,
                           float velocity_right) {
  if (!m) return MPMHIP_EINVAL;
  m->P.dirichlet = enabled != 0;
  m->P.dl = distance_left; m->P.dr = distance_right; m->P.vl = velocity_left; m->P.vr = velocity_right;
  return MPMHIP_OK;
}

int mpmhip2d_add_group(mpmhip2d_ctx *m, int32_t material, const float params[MPMHIP_NPARAM]) {
  if (!m || !params) return MPMHIP_EINVAL;
  if (material < MPMHIP_VISCO || material > MPMHIP_ELASTIC) return fail2d(m, MPMHIP_EINVAL, "unknown material id");
  if ((int)m->groups.size() >= MPMHIP_MAX_GROUPS) return fail2d(m, MPMHIP_ECAPACITY, "too many particle groups");
  if (!(params[0] > 0) || !(params[1] > 0)) return fail2d(m, MPMHIP_EINVAL, "group mass and vol must be > 0");
  GroupParams g;
  memset(&g, 0, sizeof g);
  memcpy(g.p, params, sizeof g.p);
  g.type = material;
  m->groups.push_back(g);
  HIPCHK2D(m, hipSetDevice(m->device));
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  HIPCHK2D(m, hipMemcpy(m->d_groups, m->groups.data(), sizeof(GroupParams) * m->groups.size(), hipMemcpyHostToDevice));
  return (int)m->groups.size() - 1;
}

int mpmhip2d_add_particles(mpmhip2d_ctx *m, int32_t group, int64_t n, const float *x, const float *v, const float *F, const float *B,
                           const float *aux) {
  if (!m || n < 0 || (n > 0 && !x)) return MPMHIP_EINVAL;
  if (group < 0 || group >= (int)m->groups.size()) return fail2d(m, MPMHIP_EINVAL, "unknown group");
  if (n == 0) return MPMHIP_OK;
  HIPCHK2D(m, hipSetDevice(m->device));
  if (int rc = async_drop_view(m)) return rc;  // (resident async stepper: arrays that only mirror the pools go first)
  if (m->n + n > m->cap) {
    if (!m->async.resident) return fail2d(m, MPMHIP_ECAPACITY, "particle capacity exceeded");
    if (int rc = a2_grow_particles(m, m->n + n)) return rc;  // (a resident stepper's arrays hold one batch or one working set)
  }
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  const int mat = m->groups[group].type;
  const float aux0 = (mat == MPMHIP_SNOW || mat == MPMHIP_WATER) ? 1.0f : (mat == MPMHIP_VISCO ? 1000.0f : 0.0f);
  std::vector<float> h;
  auto put = [&](float *dst, const float *src, int width, const float *dflt) -> hipError_t {
    if (!src) {
      h.resize((size_t)n * width);
      for (int64_t i = 0; i < n; i++)
        for (int k = 0; k < width; k++) h[(size_t)i * width + k] = dflt[k];
      src = h.data();
    }
    return hipMemcpy(dst + m->n * width, src, sizeof(float) * n * width, hipMemcpyHostToDevice);
  };
  const float zero4[4] = {0, 0, 0, 0}, eye[4] = {1, 0, 0, 1}, a0[1] = {aux0};
  HIPCHK2D(m, put(m->x, x, 2, zero4));
  HIPCHK2D(m, put(m->v, v, 2, zero4));
  HIPCHK2D(m, put(m->F, F, 4, eye));
  HIPCHK2D(m, put(m->B, B, 4, zero4));
  HIPCHK2D(m, put(m->aux, aux, 1, a0));
  std::vector<int32_t> ids((size_t)n), gs((size_t)n, group);
  for (int64_t i = 0; i < n; i++) ids[i] = m->next_pid + (int32_t)i;
  m->next_pid += (int32_t)n;
  HIPCHK2D(m, hipMemcpy(m->pid + m->n, ids.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
  HIPCHK2D(m, hipMemcpy(m->gid + m->n, gs.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
  m->n += n;
  return MPMHIP_OK;
}

static mpm2d::RigidArgs2 rigid_args2(mpmhip2d_ctx *m) {
  mpm2d::RigidArgs2 R;
  memset(&R, 0, sizeof R);
  R.enabled = m->rigid_enabled && m->rigid.bodies.size() > 1;  // has_rigid_body()
  R.mind = m->d_mind; R.tags = m->d_tags; R.rb = m->d_rb; R.states = m->d_states; R.bnd = m->d_bnd;
  R.penalty = m->penalty; R.pushing_force = m->pushing_force;
  return R;
}
// rasterize_rigid_boundary + gather_cdf (src/mpm.cpp:466-472, 506-508)
static int rigid2_pre(mpmhip2d_ctx *m) {
  const size_t nodes = (size_t)(m->P.res[0] + 1) * (m->P.res[1] + 1);
  HIPCHK2D(m, hipMemsetAsync(m->d_mind, 0xFF, sizeof(unsigned long long) * nodes, m->stream));
  HIPCHK2D(m, hipMemsetAsync(m->d_tags, 0, sizeof(uint32_t) * nodes, m->stream));
  const mpm2d::RigidArgs2 R = rigid_args2(m);
  const uint32_t ns = (uint32_t)m->rigid.h_smp.size();
  if (ns)
    hipLaunchKernelGGL(mpm2d::k2_cdf_rasterize, dim3((ns + 255) / 256), dim3(256), 0, m->stream, m->P.res[0], m->P.res[1], m->P.dx, m->P.idx, R,
                       (const mpm2d::Sample2 *)m->d_smp, (const float *)m->d_elems, ns);
  if (m->n)
    hipLaunchKernelGGL(mpm2d::k2_gather_cdf, dim3((unsigned)((m->n + 255) / 256)), dim3(256), 0, m->stream, m->P.res[0], m->P.res[1], m->P.dx,
                       m->P.idx, R, m->n, (const float *)m->x, (const int32_t *)m->pid);
  HIPCHK2D(m, hipGetLastError());
  return MPMHIP_OK;
}
// rigid_body_levelset_collision(current_t, dt) (src/mpm_rigid_body.cpp:347-387), between normalize_grid and the grid boundary
// condition (src/mpm.cpp:535-538); see do_rigid_ls_collision of rigid_api.h
static int rigid2_ls_collision(mpmhip2d_ctx *m) {
  const uint32_t n = (uint32_t)m->rigid.h_smp.size();
  if (n == 0 || m->LS.n == 0) return MPMHIP_OK;
  if (m->ls_cap < n) {
    m->ls_tmp_bytes = 0;
    const size_t cap = (size_t)n + n / 4 + 1024;
    for (int k = 0; k < 2; k++) { HIPCHK2D(m, m->d_ls_keys[k].alloc(cap)); HIPCHK2D(m, m->d_ls_vals[k].alloc(cap)); }
    size_t bytes = 0;
    HIPCHK2D(m, hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, m->d_ls_keys[0].get(), m->d_ls_keys[1].get(), m->d_ls_vals[0].get(), m->d_ls_vals[1].get(), (int)cap, 0, 64, m->stream));
    HIPCHK2D(m, m->d_ls_tmp.alloc(bytes));
    m->ls_tmp_bytes = bytes;
    m->ls_cap = (uint32_t)cap;
  }
  if (m->n_ranked < n) {  // boundary particles added since: behind everybody else, in creation order (appended to `particles`)
    std::vector<uint32_t> rk(n);
    HIPCHK2D(m, hipStreamSynchronize(m->stream));
    if (m->n_ranked) HIPCHK2D(m, hipMemcpy(rk.data(), m->d_smp_rank, sizeof(uint32_t) * m->n_ranked, hipMemcpyDeviceToHost));
    for (uint32_t s = m->n_ranked; s < n; s++) rk[s] = s;
    HIPCHK2D(m, m->d_smp_rank.alloc((size_t)n + n / 4 + 1024));
    HIPCHK2D(m, hipMemcpy(m->d_smp_rank, rk.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    m->n_ranked = n;
  }
  hipLaunchKernelGGL(mpm2d::k2_ls_keys, dim3((n + 255) / 256), dim3(256), 0, m->stream, m->P.idx, (const mpm2d::Rigid2 *)m->d_rb,
                     (const mpm2d::Sample2 *)m->d_smp, n, (const uint32_t *)m->d_smp_rank, m->d_ls_keys[0], m->d_ls_vals[0]);
  size_t bytes = m->ls_tmp_bytes;
  HIPCHK2D(m, hipcub::DeviceRadixSort::SortPairs(m->d_ls_tmp, bytes, m->d_ls_keys[0].get(), m->d_ls_keys[1].get(), m->d_ls_vals[0].get(), m->d_ls_vals[1].get(), (int)n, 0, 64, m->stream));
  mpm2d::Restitution2 rest;
  memset(&rest, 0, sizeof rest);
  for (size_t b = 1; b < m->rigid.bodies.size(); b++) rest.e[b] = m->rigid.bodies[b].cfg.restitution;
  hipLaunchKernelGGL(mpm2d::k2_ls_collide, dim3(1), dim3(1024), 0, m->stream, m->P, m->LS, m->d_rb, (int)m->rigid.bodies.size(),
                     (const mpm2d::Sample2 *)m->d_smp, (const uint32_t *)m->d_ls_vals[1], n, m->d_smp_rank, rest);
  HIPCHK2D(m, hipGetLastError());
  return MPMHIP_OK;
}
static int rigid2_advect(mpmhip2d_ctx *m) {
  const float dt = m->P.dt;
  const mpm2d::Steps2 st = rigid_setup::scripted_steps<2>(m->rigid, m->t, dt);
  hipLaunchKernelGGL(mpm2d::k2_rigid_advect, dim3(1), dim3(64), 0, m->stream, m->d_rb, (int)m->rigid.bodies.size(), st, dt, m->P.g[0], m->P.g[1]);
  HIPCHK2D(m, hipGetLastError());
  return MPMHIP_OK;
}

int mpmhip2d_set_deterministic(mpmhip2d_ctx *m, int32_t on) {
  if (!m) return MPMHIP_EINVAL;
  m->det.on = on != 0;
  return MPMHIP_OK;
}
int mpmhip2d_upload_ids(mpmhip2d_ctx *m, int64_t n, const int32_t *ids) {
  if (!m || !ids) return MPMHIP_EINVAL;
  if (m->async.resident) return fail2d(m, MPMHIP_EINVAL, "upload_ids: not on a resident asynchronous stepper (its pools hold the ids)");
  if (n != m->n) return fail2d(m, MPMHIP_EINVAL, "upload_ids: n = " + std::to_string(n) + " but the simulation holds " + std::to_string(m->n) + " slots");
  int32_t top = -1;
  for (int64_t i = 0; i < n; i++) {
    if (ids[i] < 0) return fail2d(m, MPMHIP_EINVAL, "upload_ids: ids must be >= 0");
    top = std::max(top, ids[i]);
  }
  if (n == 0) return MPMHIP_OK;
  if (top == INT32_MAX) return fail2d(m, MPMHIP_EINVAL, "upload_ids: id out of range");
  HIPCHK2D(m, hipSetDevice(m->device));
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  std::vector<int32_t> h((size_t)n);
  HIPCHK2D(m, hipMemcpy(h.data(), m->pid, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n; i++) h[i] = h[i] < 0 ? -1 : ids[i];  // (a deleted slot stays deleted)
  HIPCHK2D(m, hipMemcpy(m->pid, h.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
  m->next_pid = std::max(m->next_pid, top + 1);
  return MPMHIP_OK;
}
// the mode's arrays: per node the counters and cell starts (+ 1: start[nodes] is the number of live particles), per particle the
// index, the staged records and a row of impulse sums per 256 sorted positions
static int det2_reserve(mpmhip2d_ctx *m) {
  auto &D = m->det;
  const size_t nodes = (size_t)(m->P.res[0] + 1) * (m->P.res[1] + 1);
  hipError_t e = hipSuccess;
  auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  if (!D.count) {
    A(D.count.alloc(nodes + 1)); A(D.start.alloc(nodes + 1));
    size_t bytes = 0;
    A(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, D.count.get(), D.start.get(), (int)(nodes + 1), m->stream));
    A(D.scan_tmp.alloc(std::max<size_t>(bytes, 16)));
    D.scan_bytes = bytes;
  }
  if (e == hipSuccess && D.cap < m->cap) {
    HIPCHK2D(m, hipStreamSynchronize(m->stream));
    D.cap = 0;
    const size_t c = (size_t)m->cap;
    A(D.off.alloc(c)); A(D.unordered.alloc(c)); A(D.idx.alloc(c)); A(D.key.alloc(c)); A(D.rec.alloc(3 * c));
    A(D.rows.alloc(((c + 255) / 256) * (size_t)mpm2d::DET_ROW));
    if (e == hipSuccess) D.cap = m->cap;
  }
  if (e != hipSuccess) {
    det2_free(m);
    return fail2d(m, MPMHIP_ENOMEM, std::string("deterministic mode: ") + hipGetErrorString(e));
  }
  return MPMHIP_OK;
}
// P2G of the mode (k_mpm2d_det.h): cell sort, staged records, gather; with bodies the stage kernel leaves the impulse rows
static int det2_p2g(mpmhip2d_ctx *m, const mpm2d::RigidArgs2 &R) {
  auto &D = m->det;
  const size_t nodes = (size_t)(m->P.res[0] + 1) * (m->P.res[1] + 1);
  const dim3 pg((unsigned)((m->n + 255) / 256)), wg(256);
  const uint32_t *total = D.start + nodes;
  HIPCHK2D(m, hipMemsetAsync(D.count, 0, sizeof(uint32_t) * (nodes + 1), m->stream));
  hipLaunchKernelGGL(mpm2d::k2d_count, pg, wg, 0, m->stream, m->P, m->n, (const float *)m->x, (const float *)m->v, m->pid, D.key, D.off, D.count,
                     m->n_dead);
  size_t bytes = D.scan_bytes;
  HIPCHK2D(m, hipcub::DeviceScan::ExclusiveSum(D.scan_tmp, bytes, D.count.get(), D.start.get(), (int)(nodes + 1), m->stream));
  hipLaunchKernelGGL(mpm2d::k2d_fill, pg, wg, 0, m->stream, m->n, (const int32_t *)D.key, (const uint32_t *)D.off, (const uint32_t *)D.start,
                     D.unordered);
  hipLaunchKernelGGL(mpm2d::k2d_order, pg, wg, 0, m->stream, m->n, (const int32_t *)D.key, (const int32_t *)m->pid, (const uint32_t *)D.start,
                     (const uint32_t *)D.unordered, D.idx);
  const int nb = (int)m->rigid.bodies.size();
  const dim3 tg((unsigned)((m->P.res[1] + 1 + mpm2d::DET_TJ - 1) / mpm2d::DET_TJ), (unsigned)((m->P.res[0] + 1 + mpm2d::DET_TI - 1) / mpm2d::DET_TI));
  if (R.enabled) {
    hipLaunchKernelGGL(mpm2d::k2d_stage<true>, pg, wg, 0, m->stream, m->P, total, (const uint32_t *)D.idx, (const float *)m->x, m->v,
                       (const float *)m->F, (const float *)m->B, (const float *)m->aux, (const int32_t *)m->gid,
                       (const GroupParams *)m->d_groups, D.rec, R, nb, D.rows);
    hipLaunchKernelGGL(mpm2d::k2d_gather<true>, tg, wg, 0, m->stream, m->P, (const uint32_t *)D.start, (const float4 *)D.rec, m->grid, R);
  } else {
    hipLaunchKernelGGL(mpm2d::k2d_stage<false>, pg, wg, 0, m->stream, m->P, total, (const uint32_t *)D.idx, (const float *)m->x, m->v,
                       (const float *)m->F, (const float *)m->B, (const float *)m->aux, (const int32_t *)m->gid,
                       (const GroupParams *)m->d_groups, D.rec, R, nb, D.rows);
    hipLaunchKernelGGL(mpm2d::k2d_gather<false>, tg, wg, 0, m->stream, m->P, (const uint32_t *)D.start, (const float4 *)D.rec, m->grid, R);
  }
  HIPCHK2D(m, hipGetLastError());
  return MPMHIP_OK;
}
// the impulse rows of the launch before (k2d_stage or k2d_g2p: each is applied before the next one writes) added to the bodies
static void det2_rows_apply(mpmhip2d_ctx *m) {
  const size_t nodes = (size_t)(m->P.res[0] + 1) * (m->P.res[1] + 1);
  hipLaunchKernelGGL(mpm2d::k2d_rows_apply, dim3((unsigned)m->rigid.bodies.size() - 1), dim3(64), 0, m->stream, m->d_rb, (const float *)m->det.rows,
                     (const uint32_t *)(m->det.start + nodes));
}
static int substep2d(mpmhip2d_ctx *m);
int mpmhip2d_substep(mpmhip2d_ctx *m) {  // MPM<2>::substep, src/mpm.cpp:452-575
  if (!m) return MPMHIP_EINVAL;
  if (m->async.resident) return fail2d(m, MPMHIP_EINVAL, "an asynchronous stepper steps with mpmhip2d_async_step (mpmhip2d_step forwards to it)");
  return substep2d(m);
}
static int substep2d(mpmhip2d_ctx *m) {
  HIPCHK2D(m, hipSetDevice(m->device));
  const size_t nodes = (size_t)(m->P.res[0] + 1) * (m->P.res[1] + 1);
  m->P.t = m->t;
  const dim3 pg((unsigned)std::max<int64_t>((m->n + 255) / 256, 1)), gg((unsigned)((nodes + 255) / 256)), wg(256);
  const bool det = m->det.on && m->n > 0;  // (no particles: the default path, which then only clears the grid)
  if (det) {
    if (int rc = det2_reserve(m)) return rc;
  } else {
    HIPCHK2D(m, hipMemsetAsync(m->grid, 0, sizeof(float) * 3 * nodes, m->stream));  // (the mode's gather writes every node)
  }
  const mpm2d::RigidArgs2 R = rigid_args2(m);
  if (R.enabled) {
    if (m->joints.n)  // articulate, between the sort and rasterize_rigid_boundary (src/mpm.cpp:466-471)
      hipLaunchKernelGGL(mpm2d::k2_articulate, dim3(1), dim3(64), 0, m->stream, m->d_rb, m->joints, m->joint_iterations);
    if (int rc = rigid2_pre(m)) return rc;
  }
  if (det) {
    if (int rc = det2_p2g(m, R)) return rc;
    if (R.enabled) det2_rows_apply(m);
  } else {
    if (m->n)
      hipLaunchKernelGGL(mpm2d::k_p2g, pg, wg, 0, m->stream, m->P, m->n, (const float *)m->x, m->v, (const float *)m->F,
                         (const float *)m->B, (const float *)m->aux, (const int32_t *)m->gid, (const int32_t *)m->pid,
                         (const GroupParams *)m->d_groups, m->grid, R);
    if (R.enabled) hipLaunchKernelGGL(mpm2d::k2_rigid_apply_tmp, dim3(1), dim3(64), 0, m->stream, m->d_rb, (int)m->rigid.bodies.size());
  }
  if (R.enabled && m->ls_collision) {
    if (int rc = rigid2_ls_collision(m)) return rc;
  }
  const bool sdf = m->LS.sdf.phi0 != nullptr;  // (a ctx without a sampled set launches what it always did)
  if (sdf) hipLaunchKernelGGL(mpm2d::k_grid_sdf, gg, wg, 0, m->stream, m->P, m->LS, m->grid);
  else hipLaunchKernelGGL(mpm2d::k_grid, gg, wg, 0, m->stream, m->P, m->LS, m->grid);
  if (det && R.enabled) {  // (without bodies k_g2p adds nothing across particles: the default launch is kept)
    hipLaunchKernelGGL(mpm2d::k2d_g2p, pg, wg, 0, m->stream, m->P, m->LS, (const uint32_t *)(m->det.start + nodes), (const uint32_t *)m->det.idx,
                       m->x, m->v, m->F, m->B, m->aux, (const int32_t *)m->gid, m->pid, (const GroupParams *)m->d_groups,
                       (const float *)m->grid, m->n_dead, R, (int)m->rigid.bodies.size(), m->det.rows);
    det2_rows_apply(m);
  } else if (m->n) {
    hipLaunchKernelGGL(mpm2d::k_g2p, pg, wg, 0, m->stream, m->P, m->LS, m->n, m->x, m->v, m->F, m->B, m->aux, (const int32_t *)m->gid,
                       m->pid, (const GroupParams *)m->d_groups, (const float *)m->grid, m->n_dead, R);
    if (R.enabled) hipLaunchKernelGGL(mpm2d::k2_rigid_apply_tmp, dim3(1), dim3(64), 0, m->stream, m->d_rb, (int)m->rigid.bodies.size());
  }
  if (sdf && m->P.particle_collision && m->n)  // the push g2p_particle carries for shapes (LS.n == 0 here: it skipped it)
    hipLaunchKernelGGL(mpm2d::k2_sdf_collide, pg, wg, 0, m->stream, m->P, m->LS.sdf, m->n, m->x.get(), m->v.get(), (const int32_t *)m->pid);
  if (R.enabled) {
    if (int rc = rigid2_advect(m)) return rc;
  }
  HIPCHK2D(m, hipGetLastError());
  m->t += m->P.dt;
  return MPMHIP_OK;
}

// ---- CPIC rigid bodies in 2D: add_particles(type='rigid') of MPM<2> (src/mpm_rigid_body.cpp:130-252, dim = 2 branches)
int mpmhip2d_set_rigid_levelset_collision(mpmhip2d_ctx *m, int32_t enabled) {
  if (!m) return MPMHIP_EINVAL;
  if (enabled && m->LS.sdf.phi0)  // (k2_ls_collide reads shapes)
    return fail2d(m, MPMHIP_EINVAL, "rigid_body_levelset_collision is not supported with a sampled level set");
  m->ls_collision = enabled != 0;
  return MPMHIP_OK;
}
int mpmhip2d_set_rigid_coupling(mpmhip2d_ctx *m, float penalty, float pushing_force) {
  if (!m) return MPMHIP_EINVAL;
  m->penalty = penalty; m->pushing_force = pushing_force;
  return MPMHIP_OK;
}
int mpmhip2d_add_rigid_body(mpmhip2d_ctx *m, const mpmhip2d_rigid_config *cfg, int64_t n_segments, const float *segments) {
  if (!m || !cfg || !segments || n_segments <= 0) return MPMHIP_EINVAL;
  if (m->async.resident) return fail2d(m, MPMHIP_EINVAL, "rigid bodies cannot be combined with asynchronous stepping");
  HIPCHK2D(m, hipSetDevice(m->device));
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  const size_t nodes = (size_t)(m->P.res[0] + 1) * (m->P.res[1] + 1);
  if (!m->rigid_enabled) {
    hipError_t e = hipSuccess;
    auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    A(m->d_rb.alloc((size_t)mpm2d::MAX_RIGID2)); A(m->d_mind.alloc(nodes)); A(m->d_tags.alloc(nodes));
    A(m->d_states.alloc((size_t)m->cap)); A(m->d_bnd.alloc((size_t)m->cap));
    if (e != hipSuccess) return fail2d(m, MPMHIP_ENOMEM, std::string("rigid coupling: ") + hipGetErrorString(e));
    HIPCHK2D(m, hipMemset(m->d_rb, 0, sizeof(mpm2d::Rigid2) * mpm2d::MAX_RIGID2));
    HIPCHK2D(m, hipMemset(m->d_states, 0, sizeof(uint32_t) * (size_t)m->cap));
    HIPCHK2D(m, hipMemset(m->d_bnd, 0, sizeof(mpm2d::Bnd2) * (size_t)m->cap));
    m->rigid.bodies.clear();
    m->rigid.bodies.emplace_back();  // the background body
    m->rigid_enabled = true;
  }
  if ((int)m->rigid.bodies.size() >= mpm2d::MAX_RIGID2) return fail2d(m, MPMHIP_ECAPACITY, "too many rigid bodies");
  mpm2d::Rigid2 D;
  int32_t allocated = 0, body = (int32_t)m->rigid.bodies.size();
  if (const char *why = rigid_setup::add_body<2>(*cfg, n_segments, segments, m->P.dx, m->P.idx, m->P.res, m->t, m->next_pid, m->rigid, D, allocated))
    return fail2d(m, MPMHIP_EINVAL, why);
  m->next_pid += allocated;  // later material particles are numbered behind the boundary particles
  HIPCHK2D(m, m->d_smp.alloc(std::max<size_t>(m->rigid.h_smp.size(), 1)));
  HIPCHK2D(m, m->d_elems.alloc(std::max<size_t>(m->rigid.h_elems.size(), 4)));
  if (!m->rigid.h_smp.empty()) HIPCHK2D(m, hipMemcpy(m->d_smp, m->rigid.h_smp.data(), sizeof(mpm2d::Sample2) * m->rigid.h_smp.size(), hipMemcpyHostToDevice));
  HIPCHK2D(m, hipMemcpy(m->d_elems, m->rigid.h_elems.data(), sizeof(float) * m->rigid.h_elems.size(), hipMemcpyHostToDevice));
  HIPCHK2D(m, hipMemcpy(m->d_rb + body, &D, sizeof D, hipMemcpyHostToDevice));
  return body;
}
// out[10]: position 2, angle (radians), velocity 2, angular velocity, mass, inv_mass, inertia, inv_inertia
// general_action("add_articulation") of MPM<2>: the 'rotation' joint (the only one the reference's 2D scenes use; its 'frozen' and
// 'stepper' are TC_NOT_IMPLEMENTED for dim = 2, src/articulation.cpp:65-67,317)
int mpmhip2d_add_articulation(mpmhip2d_ctx *m, const mpmhip_joint_config *cfg) {
  if (!m || !cfg) return MPMHIP_EINVAL;
  const int nb = m->rigid_enabled ? (int)m->rigid.bodies.size() : 0;
  if (cfg->type != MPMHIP_JOINT_ROTATION) return fail2d(m, MPMHIP_EINVAL, "add_articulation: only type='rotation' is built for 2D simulations");
  if (cfg->obj0 < 1 || cfg->obj0 >= nb) return fail2d(m, MPMHIP_EINVAL, "add_articulation: obj0 = " + std::to_string(cfg->obj0) + " is not a rigid body of this simulation");
  if (cfg->obj1 < 0 || cfg->obj1 >= nb) return fail2d(m, MPMHIP_EINVAL, "add_articulation: obj1 = " + std::to_string(cfg->obj1) + " is not a rigid body of this simulation");
  if (m->joints.n >= mpm2d::MAX_JOINTS2) return fail2d(m, MPMHIP_ECAPACITY, "at most " + std::to_string(mpm2d::MAX_JOINTS2) + " articulations");
  mpm2d::Joint2 &J = m->joints.j[m->joints.n++];
  J.obj0 = cfg->obj0; J.obj1 = cfg->obj1;
  J.I0 = m->rigid.bodies[cfg->obj0].inertia[0];
  J.I1 = cfg->obj1 == 0 ? 1.0f : m->rigid.bodies[cfg->obj1].inertia[0];  // (the background body: inertia 1, set_as_background)
  return MPMHIP_OK;
}
int mpmhip2d_set_articulation_iterations(mpmhip2d_ctx *m, int32_t n) {
  if (!m || n < 0) return MPMHIP_EINVAL;
  m->joint_iterations = n;
  return MPMHIP_OK;
}
int mpmhip2d_rigid_get_state(mpmhip2d_ctx *m, int32_t id, float *out) {
  if (!m || !out) return MPMHIP_EINVAL;
  if (!m->rigid_enabled || id < 1 || id >= (int)m->rigid.bodies.size()) return fail2d(m, MPMHIP_EINVAL, "no such rigid body");
  HIPCHK2D(m, hipSetDevice(m->device));
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  mpm2d::Rigid2 D;
  HIPCHK2D(m, hipMemcpy(&D, m->d_rb + id, sizeof D, hipMemcpyDeviceToHost));
  out[0] = D.pos[0]; out[1] = D.pos[1]; out[2] = D.angle; out[3] = D.vel[0]; out[4] = D.vel[1]; out[5] = D.omega;
  out[6] = D.mass; out[7] = D.inv_mass; out[8] = m->rigid.bodies[id].inertia[0]; out[9] = D.inv_I;
  return MPMHIP_OK;
}
// the body's segments in world space (write_rigid_body's .poly file, src/visualize.cpp:105-130): 4 floats per segment
int64_t mpmhip2d_rigid_get_mesh(mpmhip2d_ctx *m, int32_t id, int64_t cap_segments, float *out) {
  if (!m) return MPMHIP_EINVAL;
  if (!m->rigid_enabled || id < 1 || id >= (int)m->rigid.bodies.size()) return fail2d(m, MPMHIP_EINVAL, "no such rigid body");
  if (hipSetDevice(m->device) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess) return MPMHIP_EHIP;
  mpm2d::Rigid2 D;
  HIPCHK2D(m, hipMemcpy(&D, m->d_rb + id, sizeof D, hipMemcpyDeviceToHost));
  return rigid_setup::world_elements<2>(m->rigid, id, D, cap_segments, out);
}
// world positions of the boundary particles of body id (id < 0: all); returns the count
int64_t mpmhip2d_rigid_get_samples(mpmhip2d_ctx *m, int32_t id, int64_t cap, float *pos) {
  if (!m) return MPMHIP_EINVAL;
  if (!m->rigid_enabled) return 0;
  if (hipSetDevice(m->device) != hipSuccess) return MPMHIP_EHIP;
  const uint32_t ns = (uint32_t)m->rigid.h_smp.size();
  std::vector<float> w((size_t)ns * 2);
  if (ns && pos) {
    DevBuf<float> d;
    HIPCHK2D(m, d.alloc((size_t)ns * 2));
    hipLaunchKernelGGL(mpm2d::k2_sample_positions, dim3((ns + 255) / 256), dim3(256), 0, m->stream, (const mpm2d::Rigid2 *)m->d_rb,
                       (const mpm2d::Sample2 *)m->d_smp, ns, d);
    HIPCHK2D(m, hipMemcpyAsync(w.data(), d, sizeof(float) * w.size(), hipMemcpyDeviceToHost, m->stream));
    HIPCHK2D(m, hipStreamSynchronize(m->stream));
  }
  int64_t n = 0;
  for (size_t s = 0; s < m->rigid.h_smp.size(); s++) {
    if (id >= 0 && m->rigid.h_smp[s].body != id) continue;
    if (n < cap && pos) { pos[2 * n] = w[2 * s]; pos[2 * n + 1] = w[2 * s + 1]; }
    n++;
  }
  return n;
}
// rasterize_rigid_boundary + gather_cdf as a phase (parity tests), then: dense (res+1)^2 grid states / distances, and per
// live particle in slot order states, boundary distance, normal (2), near flag
int mpmhip2d_cdf_phase(mpmhip2d_ctx *m) {
  if (!m) return MPMHIP_EINVAL;
  HIPCHK2D(m, hipSetDevice(m->device));
  if (!(m->rigid_enabled && m->rigid.bodies.size() > 1)) return MPMHIP_OK;
  return rigid2_pre(m);
}
int mpmhip2d_download_cdf(mpmhip2d_ctx *m, uint32_t *states, float *distance) {
  if (!m || !states || !distance) return MPMHIP_EINVAL;
  const size_t nodes = (size_t)(m->P.res[0] + 1) * (m->P.res[1] + 1);
  memset(states, 0, nodes * 4); memset(distance, 0, nodes * 4);
  if (!m->rigid_enabled) return MPMHIP_OK;
  HIPCHK2D(m, hipSetDevice(m->device));
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  std::vector<unsigned long long> hm(nodes);
  std::vector<uint32_t> ht(nodes);
  HIPCHK2D(m, hipMemcpy(hm.data(), m->d_mind, nodes * 8, hipMemcpyDeviceToHost));
  HIPCHK2D(m, hipMemcpy(ht.data(), m->d_tags, nodes * 4, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < nodes; i++) {
    const bool has = hm[i] != ~0ull;
    states[i] = (ht[i] & 0xFFFFFFu) | (has ? ((uint32_t)(hm[i] & 0xFFu) << 24) : 0u);
    if (has) { const uint32_t bits = (uint32_t)(hm[i] >> 32); float d; memcpy(&d, &bits, 4); distance[i] = d * m->P.dx; }
  }
  return MPMHIP_OK;
}
int64_t mpmhip2d_download_colours(mpmhip2d_ctx *m, int64_t capacity, uint32_t *states, float *distance, float *normal, int32_t *near) {
  if (!m) return MPMHIP_EINVAL;
  if (hipSetDevice(m->device) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess) return MPMHIP_EHIP;
  const size_t n = (size_t)m->n;
  std::vector<int32_t> hp(n);
  std::vector<uint32_t> hs(n, 0u);
  std::vector<mpm2d::Bnd2> hb(n);
  memset(hb.data(), 0, sizeof(mpm2d::Bnd2) * n);
  if (n) {
    HIPCHK2D(m, hipMemcpy(hp.data(), m->pid, n * 4, hipMemcpyDeviceToHost));
    if (m->rigid_enabled) {
      HIPCHK2D(m, hipMemcpy(hs.data(), m->d_states, n * 4, hipMemcpyDeviceToHost));
      HIPCHK2D(m, hipMemcpy(hb.data(), m->d_bnd, sizeof(mpm2d::Bnd2) * n, hipMemcpyDeviceToHost));
    }
  }
  int64_t k = 0;
  for (size_t i = 0; i < n; i++) {
    if (hp[i] < 0) continue;
    if (k >= capacity) return fail2d(m, MPMHIP_ECAPACITY, "download buffer too small");
    if (states) states[k] = hs[i];
    if (distance) distance[k] = hb[i].dist;
    if (normal) { normal[2 * k] = hb[i].n[0]; normal[2 * k + 1] = hb[i].n[1]; }
    if (near) near[k] = (int32_t)hb[i].near;
    k++;
  }
  return k;
}

int mpmhip2d_step(mpmhip2d_ctx *m, float dt) {  // MPM<dim>::step, src/mpm.cpp:428-439 (virtual: AsyncMPM<2>::step when the stepper is resident)
  if (!m) return MPMHIP_EINVAL;
  if (m->async.resident) return mpmhip2d_async_step(m, dt);
  if (dt < 0) {
    const int rc = mpmhip2d_substep(m);
    m->request_t = m->t;
    return rc;
  }
  m->request_t += dt;
  while (m->t + m->P.dt < m->request_t)
    if (int rc = mpmhip2d_substep(m)) return rc;
  return MPMHIP_OK;
}

double mpmhip2d_current_time(const mpmhip2d_ctx *m) { return m ? (double)m->t : 0.0; }

int64_t mpmhip2d_num_particles(mpmhip2d_ctx *m) {
  if (!m) return MPMHIP_EINVAL;
  if (hipSetDevice(m->device) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess) return MPMHIP_EHIP;
  unsigned int dead = 0;
  if (hipMemcpy(&dead, m->n_dead, sizeof dead, hipMemcpyDeviceToHost) != hipSuccess) return MPMHIP_EHIP;
  return m->n - (int64_t)dead;
}

// live particles in slot order; any output may be NULL.  Returns the number written or a negative error.
int64_t mpmhip2d_download(mpmhip2d_ctx *m, int64_t capacity, float *x, float *v, float *F, float *B, float *aux, int32_t *gid,
                          int32_t *id) {
  if (!m) return MPMHIP_EINVAL;
  if (hipSetDevice(m->device) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess) return fail2d(m, MPMHIP_EHIP, "synchronise failed");
  const size_t n = (size_t)m->n;
  std::vector<float> hx(2 * n), hv(2 * n), hF(4 * n), hB(4 * n), ha(n);
  std::vector<int32_t> hg(n), hp(n);
  if (n) {
    HIPCHK2D(m, hipMemcpy(hx.data(), m->x, 8 * n, hipMemcpyDeviceToHost)); HIPCHK2D(m, hipMemcpy(hv.data(), m->v, 8 * n, hipMemcpyDeviceToHost));
    HIPCHK2D(m, hipMemcpy(hF.data(), m->F, 16 * n, hipMemcpyDeviceToHost)); HIPCHK2D(m, hipMemcpy(hB.data(), m->B, 16 * n, hipMemcpyDeviceToHost));
    HIPCHK2D(m, hipMemcpy(ha.data(), m->aux, 4 * n, hipMemcpyDeviceToHost)); HIPCHK2D(m, hipMemcpy(hg.data(), m->gid, 4 * n, hipMemcpyDeviceToHost));
    HIPCHK2D(m, hipMemcpy(hp.data(), m->pid, 4 * n, hipMemcpyDeviceToHost));
  }
  int64_t k = 0;
  for (size_t i = 0; i < n; i++) {
    if (hp[i] < 0) continue;
    if (k >= capacity) return fail2d(m, MPMHIP_ECAPACITY, "download buffer too small");
    if (x) { x[2 * k] = hx[2 * i]; x[2 * k + 1] = hx[2 * i + 1]; }
    if (v) { v[2 * k] = hv[2 * i]; v[2 * k + 1] = hv[2 * i + 1]; }
    if (F) for (int q = 0; q < 4; q++) F[4 * k + q] = hF[4 * i + q];
    if (B) for (int q = 0; q < 4; q++) B[4 * k + q] = hB[4 * i + q];
    if (aux) aux[k] = ha[i];
    if (gid) gid[k] = hg[i];
    if (id) id[k] = hp[i];
    k++;
  }
  return k;
}

int mpmhip2d_download_grid(mpmhip2d_ctx *m, float *grid) {  // (v.x, v.y, m) per node of the (res+1)^2 grid after the last substep
  if (!m || !grid) return MPMHIP_EINVAL;
  HIPCHK2D(m, hipSetDevice(m->device));
  HIPCHK2D(m, hipStreamSynchronize(m->stream));
  HIPCHK2D(m, hipMemcpy(grid, m->grid, sizeof(float) * 3 * (size_t)(m->P.res[0] + 1) * (m->P.res[1] + 1), hipMemcpyDeviceToHost));
  return MPMHIP_OK;
}

#include "async_api.h"
#include "frame2d_api.h"
#include "frame_job_api.h"
#include "fields_api.h"
// snapshot_blob.h: its copies of the device-side record geometry
static_assert(snap::RECG_BYTES == sizeof(RecG) && snap::RECP_BYTES == sizeof(RecP) && snap::BROW_BYTES == sizeof(float) * BW, "snapshot_blob.h: records");
static_assert(snap::RECG_GID == offsetof(RecG, gid) && snap::RECG_PID == offsetof(RecG, pid), "snapshot_blob.h: ids of a RecG");
static_assert(snap::REC2_BYTES == 4 * sizeof(float4) && snap::REC2_GID == 3 * sizeof(float4) + offsetof(float4, y) &&
              snap::REC2_ID == 3 * sizeof(float4) + offsetof(float4, z), "snapshot_blob.h: the 2D container record (k_async.h: Store2)");
static_assert(snap::TAG_BYTES == sizeof(uint32_t) && snap::ID_BYTES == sizeof(int32_t) && snap::W3_BYTES == 4 * sizeof(float4) &&
              snap::CONTAINER3_BYTES == sizeof(uint32_t) + sizeof(int32_t) + 2 * 4 * sizeof(float4) &&
              snap::CONTAINER2_BYTES == sizeof(uint32_t) + 4 * sizeof(float4), "snapshot_blob.h: containers (k_async.h: Store3, Store2)");
static_assert(snap::TAG_FREE == AS_FREE && snap::TAG_BACKUP == AS_BACKUP, "snapshot_blob.h: container tags");
static_assert(snap::BODY3_BYTES == sizeof(RigidBodyDev) && snap::JOINT3_BYTES == sizeof(JointDev) && snap::JOINT3_OBJ0 == offsetof(JointDev, obj0) &&
              snap::JOINT3_OBJ1 == offsetof(JointDev, obj1) && snap::MAX_JOINTS3 == (uint32_t)MAX_JOINTS, "snapshot_blob.h: 3D bodies and joints");
static_assert(snap::BODY2_BYTES == sizeof(mpm2d::Rigid2) && snap::JOINTS2_BYTES == sizeof(mpm2d::Joints2) && snap::JOINTS2_N == offsetof(mpm2d::Joints2, n) &&
              snap::JOINTS2_FIRST == offsetof(mpm2d::Joints2, j) && snap::JOINT2_BYTES == sizeof(mpm2d::Joint2) &&
              snap::JOINT2_OBJ0 == offsetof(mpm2d::Joint2, obj0) && snap::JOINT2_OBJ1 == offsetof(mpm2d::Joint2, obj1) &&
              snap::MAX_JOINTS2 == mpm2d::MAX_JOINTS2, "snapshot_blob.h: 2D bodies and joints");
static_assert(snap::P2_BYTES[snap::P2_X] == 2 * sizeof(float) && snap::P2_BYTES[snap::P2_V] == 2 * sizeof(float) && snap::P2_BYTES[snap::P2_F] == 4 * sizeof(float) &&
              snap::P2_BYTES[snap::P2_B] == 4 * sizeof(float) && snap::P2_BYTES[snap::P2_AUX] == sizeof(float) && snap::P2_BYTES[snap::P2_GID] == sizeof(int32_t) &&
              snap::P2_BYTES[snap::P2_PID] == sizeof(int32_t) && snap::RANK_BYTES == sizeof(uint32_t) && snap::COLOUR_BYTES == sizeof(uint32_t) &&
              snap::TABLE_WORD == sizeof(int64_t), "snapshot_blob.h: the 2D object's arrays, the block tables");
#include "snapshot_api.h"
#include "seed_api.h"
#include "region_api.h"

// ------------------------------------------------------------------------------------------------ debug math
int mpmhip_debug_cond_census(mpmhip_ctx *c, double out[MPMHIP_COND_CENSUS_WORDS]) {
  if (!c || !out) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "cond_census inside a substep");
  constexpr int W = 8 + COND_BINS;
  static_assert(W == MPMHIP_COND_CENSUS_WORDS, "census layout");
  DevBuf<unsigned long long> d;
  HIPCHK(c, d.alloc((size_t)W));
  HIPCHK(c, hipMemsetAsync(d, 0, sizeof(unsigned long long) * W, c->stream));
  std::vector<unsigned long long> h((size_t)W);
  if (c->n_slots > 0) {
    hipLaunchKernelGGL(k_cond_census, dim3(particle_grid(c->n_slots)), dim3(256), 0, c->stream, c->P, (const float4 *)c->rg.get(), d);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipMemcpyAsync(h.data(), d, sizeof(unsigned long long) * W, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < W; i++) out[i] = (double)h[i];
  const uint32_t bits = (uint32_t)h[4];
  float mx;
  memcpy(&mx, &bits, 4);
  out[4] = mx;
  return MPMHIP_OK;
}

int mpmhip_debug_svd3(mpmhip_ctx *c, int64_t n, const float *F, float *U, float *S, float *V) {
  if (!c || n <= 0) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<float> dF, dU, dS, dV;
  HIPCHK(c, dF.alloc(9 * n)); HIPCHK(c, dU.alloc(9 * n)); HIPCHK(c, dS.alloc(3 * n)); HIPCHK(c, dV.alloc(9 * n));
  HIPCHK(c, hipMemcpy(dF, F, sizeof(float) * 9 * n, hipMemcpyHostToDevice));
  int rc = run_debug(c, k_debug_svd, n, (const float *)dF, dU.get(), dS.get(), dV.get());
  if (!rc) {
    HIPCHK(c, hipMemcpy(U, dU, sizeof(float) * 9 * n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(S, dS, sizeof(float) * 3 * n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(V, dV, sizeof(float) * 9 * n, hipMemcpyDeviceToHost));
  }
  return rc;
}

static int make_group(mpmhip_ctx *c, int32_t material, const float *params, GroupParams &g) {
  if (material < MPMHIP_VISCO || material > MPMHIP_ELASTIC) return fail(c, MPMHIP_EINVAL, "unknown material id %d", material);
  memset(&g, 0, sizeof g);
  memcpy(g.p, params, sizeof g.p);
  g.type = material;
  return MPMHIP_OK;
}

int mpmhip_debug_force(mpmhip_ctx *c, int32_t material, const float params[MPMHIP_NPARAM], int64_t n, const float *F,
                       const float *aux, float *out) {
  if (!c || n <= 0) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  GroupParams g;
  int rc = make_group(c, material, params, g);
  if (rc) return rc;
  DevBuf<float> dF, dA, dO;
  HIPCHK(c, dF.alloc(9 * n)); HIPCHK(c, dA.alloc(n)); HIPCHK(c, dO.alloc(9 * n));
  HIPCHK(c, hipMemcpy(dF, F, sizeof(float) * 9 * n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dA, aux, sizeof(float) * n, hipMemcpyHostToDevice));
  rc = run_debug(c, k_debug_force, g, n, (const float *)dF, (const float *)dA, dO.get());
  if (!rc) HIPCHK(c, hipMemcpy(out, dO, sizeof(float) * 9 * n, hipMemcpyDeviceToHost));
  return rc;
}

int mpmhip_debug_plasticity(mpmhip_ctx *c, int32_t material, const float params[MPMHIP_NPARAM], int64_t n,
                            const float *cdg, float *F, float *aux, float *next_force) {
  if (!c || n <= 0) return MPMHIP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  GroupParams g;
  int rc = make_group(c, material, params, g);
  if (rc) return rc;
  DevBuf<float> dC, dF, dA, dO;
  HIPCHK(c, dC.alloc(9 * n)); HIPCHK(c, dF.alloc(9 * n)); HIPCHK(c, dA.alloc(n));
  if (next_force) HIPCHK(c, dO.alloc(9 * n));
  HIPCHK(c, hipMemcpy(dC, cdg, sizeof(float) * 9 * n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dF, F, sizeof(float) * 9 * n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dA, aux, sizeof(float) * n, hipMemcpyHostToDevice));
  rc = run_debug(c, k_debug_plasticity, g, n, (const float *)dC, dF.get(), dA.get(), dO.get());
  if (!rc) {
    HIPCHK(c, hipMemcpy(F, dF, sizeof(float) * 9 * n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(aux, dA, sizeof(float) * n, hipMemcpyDeviceToHost));
    if (next_force) HIPCHK(c, hipMemcpy(next_force, dO, sizeof(float) * 9 * n, hipMemcpyDeviceToHost));
  }
  return rc;
}

}  // extern "C"

#include "tiled_api.h"
#include "snapshot_job_api.h"
