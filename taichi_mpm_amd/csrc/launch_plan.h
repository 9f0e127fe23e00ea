// taichi_mpm_amd/csrc/launch_plan.h — which kernel instantiation each phase of a substep launches, and with how many workgroups
// (host only: no HIP header, nothing launched; tests/test_launch_plan_cpu.py drives every rule at both sides of its boundaries
// with plain g++).
// Knobs: every tuning switch of the substep path, read from the environment once per mpmhip_create.  Facts: the few facts of a
// ctx the decisions depend on (mpmhip.hip: facts()).  plan_sort / plan_p2g / plan_grid / plan_g2p: pure functions of the two,
// returning small plain structs; do_sort / do_p2g / do_grid / do_g2p compute their plan, map it to a kernel pointer
// (mpmhip.hip: g2p_kernel and its kin) and launch.  A new kernel form is routed HERE, and its rule is tested without a device.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "../../include/mpmhip.h"  // the material ids

namespace lp {

// what the formulas need of the device side; mpmhip.hip asserts them equal to the real ones (k_sort.h, mpm_common.h, mpm_math.h)
constexpr int RANK_BATCH = 1024;       // slots per workgroup of the rank role
constexpr int BC = 64;                 // cells per block
constexpr uint32_t MAT_ALL = 0x1FEu;   // MPMHIP_VISCO (1) .. MPMHIP_ELASTIC (8)
constexpr uint32_t VISCO_BIT = 1u << MPMHIP_VISCO;

// Below this many slots a per-GPU problem is SMALL: its kernels are bound by latency, not by bytes (1 M particles: the owner list
// takes the grid pass from 17 to 7.5 us, 768 workgroups of k_g2p 51.9 -> 46.1 us, the packed walk costs +7 us of 50)
constexpr int64_t SMALL_SLOTS = 2 << 20;
constexpr int64_t LARGE_SLOTS = 6 << 20;  // from here on k_cell_table takes 64 blocks per chunk (without the key-indexed counters)
constexpr uint32_t KEYED_MAX_BLOCK_SPACE = 1u << 21;  // grids of 2^24 blocks (res > 508) keep the four-launch sort
// particles per active block below which the blocks count as NOT full: k_g2p's chunks stay inside a block, so with 512 particles
// per block (the lattice the reference's benchmark seeds) they are full and it is the faster walk by a few microseconds on most
// boxes; with 350 per block (the same scene after the impact) a third of its lanes idle and the packed walk wins by 30 us
constexpr uint32_t PACKED_FILL = 448;
// k_g2p: 4 096 workgroups at 8 M particles (2 048 / 8 192 measured no better); below ~2 M slots the device's resident set (three
// workgroups per CU = 768) walking ~6 chunks each WITH the record prefetch beats one chunk per workgroup: 51.9 -> 46.1 us at
// 1 M particles (profiles/r04_b_knobs.txt; 512 and 1 024 are slower again)
constexpr int G2P_WGS_SMALL = 768, G2P_WGS_BLOCKS = 4096;
// k_g2p_packed: four times the device's resident set (three workgroups per CU): with equal work items what is left of the launch's
// tail is the partly filled last round — 4 096 workgroups are 5.33 rounds of 768.  At C3, lattice / after impact: 3 072 -> 287 / 336 us,
// 4 096 -> 287 / 352, 6 144 -> 291 / 343, 2 304 -> 296 / 346, 1 536 -> 292 / 350, 768 -> 304 / 350 (profiles/r04_u_g2p_wgs.txt)
constexpr int G2P_PACKED_WGS_PER_CU = 12;
constexpr int GRID_WGS_PER_CAND = 16384, GRID_WGS_PER_BLOCK = 4096;  // the grid pass's walks without the owner list (k_grid.h)

struct Knobs {
  int g2p_wgs = 0;             // workgroups of k_g2p / k_g2p_packed; 0: by size (env MPMHIP_G2P_WGS pins it)
  int p2g_wgs = 16384;         // workgroups of k_p2g (env MPMHIP_P2G_WGS)
  int grid_wgs = 0;            // workgroups of the grid pass; 0: from the last sort's owner count (env MPMHIP_GRID_WGS)
  int grid_walk = -1;          // walk of the substep's grid pass (k_grid.h): 2 owner list, 0 per block / per (block, candidate) as until
                               // round 4, -1 by size and tiling (env MPMHIP_GRID_WALK: A/B)
  int g2p_packed = -1;         // k_g2p_packed instead of k_g2p: -1 by size (from 2 M slots on; no rigid bodies, no tiling), 0 never, 1
                               // wherever it applies (env MPMHIP_G2P_PACKED)
  int rigid_wgs = 2048;        // workgroups of k_p2g_rigid (one per wave slot of the device), twice those of k_g2p_rigid (env
                               // MPMHIP_RIGID_WGS: tuning)
  int rigid_concurrent = 7;    // which pairs run side by side: 1 P2G, 2 G2P, 4 rasterisation | sort (env MPMHIP_RIGID_CONCURRENT; 0: one stream)
  uint32_t rank_runs_mul = 3;  // k_rank takes its LDS-hash path when runs * this > slots (env MPMHIP_RANK_RUNS_MUL: tuning)
  uint32_t rank_wgs_cap = 4096u;  // workgroups of the rank role (k_rank / k_sort_front): MPMHIP_RANK_WGS (tuning)
  int ct_blocks = 0;           // blocks per chunk of k_cell_table: 0 by size, 16, 32, 64 (env MPMHIP_CT_BLOCKS: tuning)
  int cell_order_form = 1;     // env MPMHIP_CELL_ORDER: 1 k_cell_order_blocks (a wave per block through LDS), 0 k_cell_order (a lane per cell)
  int cell_order_wgs = 24;     // env MPMHIP_CELL_ORDER_WGS: workgroups per CU of k_cell_order_blocks' launch
  int scan_grid = 0;           // env MPMHIP_SCAN_GRID: workgroups asked for the chained scans (scan_grid_for cuts it; tuning)
  bool sort_v1 = false;        // env MPMHIP_SORT_V1: the four-launch sort also where the key-indexed table would fit (A/B and tests)

  // read anew by every mpmhip_create (the tests change the environment between two of them)
  static Knobs from_env() {
    Knobs k;
    if (const char *e = getenv("MPMHIP_G2P_WGS")) k.g2p_wgs = atoi(e) > 0 ? atoi(e) : 0;
    if (const char *e = getenv("MPMHIP_P2G_WGS")) k.p2g_wgs = atoi(e) > 0 ? atoi(e) : 16384;
    if (const char *e = getenv("MPMHIP_GRID_WGS")) k.grid_wgs = atoi(e) > 0 ? atoi(e) : 0;
    if (const char *e = getenv("MPMHIP_GRID_WALK")) k.grid_walk = atoi(e);
    if (const char *e = getenv("MPMHIP_G2P_PACKED")) k.g2p_packed = atoi(e);
    if (const char *e = getenv("MPMHIP_RIGID_WGS")) k.rigid_wgs = atoi(e) > 1 ? atoi(e) : 2048;
    if (const char *e = getenv("MPMHIP_RIGID_CONCURRENT")) k.rigid_concurrent = atoi(e);
    if (const char *e = getenv("MPMHIP_RANK_RUNS_MUL")) k.rank_runs_mul = (uint32_t)atoi(e);
    if (const char *e = getenv("MPMHIP_RANK_WGS")) k.rank_wgs_cap = (uint32_t)std::max(1, atoi(e));
    if (const char *e = getenv("MPMHIP_CT_BLOCKS")) k.ct_blocks = atoi(e);
    if (const char *e = getenv("MPMHIP_CELL_ORDER")) k.cell_order_form = atoi(e) != 0;
    if (const char *e = getenv("MPMHIP_CELL_ORDER_WGS")) k.cell_order_wgs = std::max(1, atoi(e));
    if (const char *e = getenv("MPMHIP_SCAN_GRID")) k.scan_grid = atoi(e);
    if (const char *e = getenv("MPMHIP_SORT_V1")) k.sort_v1 = atoi(e) != 0;
    return k;
  }
};

struct Facts {
  int64_t n_slots = 0;      // slots in use (live + deleted)
  uint32_t max_blocks = 0;  // active blocks the ctx has room for
  uint32_t nbw = 1;         // 32-bit words of the active-block bitmap: the block space / 32
  int n_cus = 256;          // compute units of the device
  uint32_t mask = 0;        // bit t set = some particle group is of material t
  // what a recent sort saw, read from the pinned page a few substeps late ({0, 0, 0} before the first has reported)
  uint32_t n_live = 0, n_act = 0, n_own = 0;
  bool keyed_table = false;       // the key-indexed counter table is allocated
  bool tiled = false;             // a brick of a tiled run
  bool has_boxes = false;         // ... with halo boxes
  bool rigid = false;             // CPIC bodies besides the background
  bool deterministic = false;
  bool store_b = false;           // the ctx keeps apic_b beside RecP.A
  bool sampled_levelset = false;  // a sampled signed-distance level set is installed
  bool has_chunk_blk = false;     // the chunk table of the packed walk is allocated
};

// a transfer kernel is instantiated per material SET: one material (bit), every material but visco, all of them, or all of them
// with the deterministic mode's impulse rows (the rigid kernels only)
struct MatSet {
  enum Kind { ONE, NO_VISCO, ALL, ALL_DET } kind;
  uint32_t bit;  // ONE: 1u << material id
};
inline bool operator==(const MatSet &a, const MatSet &b) { return a.kind == b.kind && (a.kind != MatSet::ONE || a.bit == b.bit); }
inline bool single_material(uint32_t mask) { return mask && !(mask & (mask - 1)) && (mask & MAT_ALL); }
// the colour-aware kernels (k_p2g_rigid / k_g2p_rigid).  Deterministic mode: the all-material form with the impulse rows
inline MatSet rigid_mats(const Facts &f) {
  if (f.deterministic) return {MatSet::ALL_DET, 0};
  return single_material(f.mask) ? MatSet{MatSet::ONE, f.mask} : MatSet{MatSet::ALL, 0};
}

// ------------------------------------------------------------------------------------------------ sort
struct SortPlan {
  bool keyed;       // k_sort_front + k_perm_keyed on the key-indexed counters; else k_block_table, k_rank, k_perm
  bool build_list;  // k_cell_table builds neighbour rows + owner list for the grid pass (becomes the ctx's list_valid)
  int ct;           // blocks per chunk of k_cell_table: 16, 32 or 64
  uint32_t bt_chunks, ct_chunks;  // chunks of the two chained scans (their launches are cut to scan_limit(kernel))
  uint32_t rank_wgs;
  int cell_order_form, cell_order_wgs;  // deterministic mode: k_cell_order (0) / k_cell_order_blocks (1) and its workgroups
};
inline SortPlan plan_sort(const Knobs &k, const Facts &f) {
  SortPlan p;
  // key-indexed cell counters: the ranks need no block table and share a launch with it (k_sort_front)
  p.keyed = f.keyed_table && (uint64_t)f.nbw * 32u <= KEYED_MAX_BLOCK_SPACE && !k.sort_v1;
  // blocks per chunk of k_cell_table: few blocks -> finer chunks (shorter chains, more workgroups).  16 below 2 M slots, 64 from 6 M on
  // (16 costs 10 us at 8 M: its 1 100 chunks no longer fit the scans' resident grid), 32 in between — a rank of a 2-brick job
  // holds 4 M particles in 8 788 blocks: 17.4 us with 64 (as long as the whole 8 M problem takes: the kernel is a latency chain)
  // With the key-indexed counters (k_sort_front) 16 is the best or within 3 us of it at every size (profiles/r05_s_ct_blocks.txt: a rank
  // of 4 M 47.5 -> 44 us, C3 after impact 89.6 -> 86.5, the lattice 67.3 -> 64.2 where 32 gives 61.5): the plain table of that form keeps
  // 1 100..1 340 chunks resident in one round.
  p.ct = (k.ct_blocks == 16 || k.ct_blocks == 32 || k.ct_blocks == 64) ? k.ct_blocks
         : (p.keyed || f.n_slots < SMALL_SLOTS ? 16 : (f.n_slots < LARGE_SLOTS ? 32 : 64));
  p.bt_chunks = (f.nbw + 255) / 256;
  p.ct_chunks = (f.max_blocks + p.ct - 1) / p.ct;
  // Owner list of the grid pass (k_sort.h, k_grid.h): below 2 M slots it takes the pass from 17 to 7.5 us (1 M particles) for 2..3 us
  // in k_rank + k_cell_table; a tiled ctx always builds it (the per-block walk with the halo-box code in it thrashes the instruction
  // cache: 31 -> 19 us at 4 M particles per rank); an untiled ctx of 2 M slots and more does not — there the pass is bound by its
  // 180 MB of tile reads either way (30.4 against 30.5 us at 8 M) and the rows cost the sort 8 us (profiles/r05_e_*_census.txt).
  p.build_list = k.grid_walk == 2 || (k.grid_walk < 0 && (f.tiled || f.n_slots < SMALL_SLOTS));
  p.rank_wgs = std::max(1u, std::min<uint32_t>(((uint32_t)f.n_slots + RANK_BATCH - 1) / RANK_BATCH, k.rank_wgs_cap));
  p.cell_order_form = k.cell_order_form;
  // form 0 (A/B): one lane per cell over the whole table; form 1: one wave per active block through LDS, 7 workgroups per CU resident
  // (22 KiB each), a few blocks per wave
  p.cell_order_wgs = k.cell_order_form == 0
                         ? (int)std::min<uint64_t>(8192u, ((uint64_t)f.max_blocks * BC + 255) / 256)
                         : std::max(1, (int)std::min<uint64_t>((uint64_t)f.n_cus * (uint64_t)k.cell_order_wgs, ((uint64_t)f.max_blocks + 3) / 4));
  return p;
}

// workgroups a single-pass scan kernel may be launched with: three eighths of what the device keeps resident of THAT kernel (a
// quarter until round 4: after impact C3 has 21 k active blocks = 335 chunks of k_cell_table, and with 256 workgroups 79 of them
// took a second chunk behind their first — sort 98 -> 88 us, profiles/r04_l_scan_grid.txt); the margin is for kernels of a second
// stream (CPIC) beside the scans.  Per kernel since round 5: the list forms of k_cell_table hold fewer workgroups per CU than the
// plain ones, and the lowest of all of them would cost the plain ones their grid.
// The arithmetic of that bound (tests/test_host_cpu.py drives it through mpmhip_debug_scan_grid).  `per_cu` = what the
// occupancy API answers for the kernel at 256 threads.  That answer can be one workgroup per CU HIGH (MI355X guide: 256-thread blocks
// are admitted up to min(API, 8, ...) per CU, one fewer than the API says at 81..112 SGPRs), so the set that is certainly resident is
// min(per_cu, 8) - 1 per CU (at least 1).  Three eighths of the API's number lies inside it for every per_cu (3/8 p <= p - 1 from
// p = 2 on; p = 1: a third of the CUs), a request from the environment is cut to half the API's number AND to that set.
inline uint32_t scan_resident_set(int n_cus, int per_cu) { return (uint32_t)(std::max(1, n_cus) * std::max(1, std::min(per_cu, 8) - 1)); }
inline uint32_t scan_grid_for(int n_cus, int per_cu, int env_request) {
  per_cu = std::max(1, per_cu);
  int lim = std::max(1, std::max(1, n_cus) * per_cu * 3 / 8);
  if (env_request > 0) lim = std::max(1, std::min(env_request, std::max(1, n_cus) * per_cu / 2));
  return std::min<uint32_t>((uint32_t)lim, scan_resident_set(n_cus, per_cu));
}

// ------------------------------------------------------------------------------------------------ P2G
struct P2GPlan {
  int wgs;         // k_p2g, 64 threads
  bool rigid;      // the blocks near a body go to k_p2g_rigid, beside k_p2g
  int rigid_wgs;   // ... at 64 threads
  MatSet rigid_mats;
};
inline P2GPlan plan_p2g(const Knobs &k, const Facts &f) { return {k.p2g_wgs, f.rigid, k.rigid_wgs, rigid_mats(f)}; }

// ------------------------------------------------------------------------------------------------ grid pass
enum class GridWalk { LIST, PER_BLOCK, PER_CAND };
struct GridPlan {
  GridWalk walk;
  bool sampled;  // the instantiation that reads the sampled level set
  int wgs;
  bool refuse_energy_on_tiled;  // nothing is launched: only the owner-list walk knows which rank counts a halo node's energy
};
// mode 0 (the substep's pass) and modes 4 / 5 (energy) walk the owner list when the last sort built one (plan_sort: small problems
// and every tiled ctx): one wave per touched grid block, launched at the size of the list as the last sort reported it (+ 12 %; the
// walk is a grid-stride loop, so a stale number costs time, never correctness).  Otherwise, and for the dense views (modes 1-3): the
// walks of rounds 1-4 — per block at >= 2 M slots, per (block, candidate) below (small per-GPU problem: latency-bound, see k_grid.h).
inline GridPlan plan_grid(const Knobs &k, const Facts &f, int mode, bool list_valid) {
  GridPlan p{GridWalk::PER_BLOCK, mode == 0 && f.sampled_levelset, 0, false};
  if ((mode == 0 || mode == 4 || mode == 5) && list_valid) {
    uint64_t n_own = f.n_own;
    if (n_own == 0) n_own = std::min<uint64_t>((uint64_t)f.max_blocks * 8u, 32768u);  // (before the first sort has reported)
    p.walk = GridWalk::LIST;
    p.wgs = k.grid_wgs > 0 ? k.grid_wgs : (int)std::min<uint64_t>(8192u, std::max<uint64_t>(64u, (n_own + n_own / 8 + 3) / 4 + 8));
    return p;
  }
  if ((mode == 4 || mode == 5) && f.has_boxes) {
    p.refuse_energy_on_tiled = true;
    return p;
  }
  if (mode == 0 && f.n_slots < SMALL_SLOTS) p.walk = GridWalk::PER_CAND;
  p.wgs = p.walk == GridWalk::PER_CAND ? GRID_WGS_PER_CAND : GRID_WGS_PER_BLOCK;
  if (k.grid_wgs > 0 && mode == 0) p.wgs = k.grid_wgs;
  return p;
}

// ------------------------------------------------------------------------------------------------ G2P
struct G2PPlan {
  bool packed;  // k_g2p_packed alone; else k_g2p, beside k_g2p_rigid on a ctx with bodies
  MatSet mats;  // ONE, NO_VISCO or ALL
  bool store_b, rigid;
  int wgs;      // 256 threads
  MatSet rigid_mats;
  int rigid_wgs;  // ... at 256 threads
};
// Which G2P kernel the plain blocks get (bench.py names the kernel of its roofline after it: mpmhip_debug_g2p_is_packed).
// Material set: one material in the whole ctx (the benchmark configurations, most scene scripts) -> the kernel that carries only
// that material's constitutive code; no visco group -> the set without it (mpmhip.hip: g2p_kernel has the register budgets).  The
// one-material kernels exist only without apic_b.
// Packed chunks (k_g2p_packed.h): -3.5 us of 303 on the lattice of C3, -14 us of 373 after impact; at 1 M particles +7 us of 50
// (768 workgroups with a handful of chunks each: the walk's set-up is not amortised) — hence by size, and by how full the blocks are
// (PACKED_FILL; the numbers come from the sort, a few substeps late).  One-material instantiations only: they stay below the 168
// VGPRs of three workgroups per CU — 163 to 167; the kernel for mixed materials would have 177, the visco one 183: those scenes
// keep k_g2p.
inline G2PPlan plan_g2p(const Knobs &k, const Facts &f, int phase) {
  G2PPlan p;
  bool packed = k.g2p_packed != 0;
  if (k.g2p_packed < 0) packed = f.n_slots >= SMALL_SLOTS && f.n_act > 0 && (uint64_t)f.n_live < (uint64_t)f.n_act * PACKED_FILL;
  p.packed = packed && single_material(f.mask) && f.mask != VISCO_BIT && !f.rigid && !f.store_b && phase == 0 && !f.tiled && f.has_chunk_blk;
  p.store_b = f.store_b;
  p.rigid = f.rigid;
  p.mats = !f.store_b && single_material(f.mask) ? MatSet{MatSet::ONE, f.mask}
                                               : MatSet{(f.mask & VISCO_BIT) ? MatSet::ALL : MatSet::NO_VISCO, 0};
  p.wgs = k.g2p_wgs > 0 ? k.g2p_wgs
                        : (f.n_slots < SMALL_SLOTS ? G2P_WGS_SMALL : (p.packed ? G2P_PACKED_WGS_PER_CU * f.n_cus : G2P_WGS_BLOCKS));
  p.rigid_mats = rigid_mats(f);
  p.rigid_wgs = k.rigid_wgs / 2;
  return p;
}

// ------------------------------------------------------------------------------------------------ which transfer kernels
// The instantiations of the transfer kernels a substep launches, as eight words (mpmhip_debug_transfer_plan; the tests assert the
// form they mean to cover before they compare numbers): [0] packed, [1] kind and [2] bit of the set k_g2p / k_g2p_packed carry,
// [3] STORE_B, [4] RIGID, [5] kind and [6] bit of the set of k_p2g_rigid / k_g2p_rigid, [7] P2G launches k_p2g_rigid on that set
inline void transfer_plan_words(const Knobs &k, const Facts &f, int32_t out[8]) {
  const G2PPlan g = plan_g2p(k, f, 0);
  const P2GPlan p = plan_p2g(k, f);
  out[0] = g.packed;
  out[1] = (int32_t)g.mats.kind;
  out[2] = g.mats.kind == MatSet::ONE ? (int32_t)g.mats.bit : 0;
  out[3] = g.store_b;
  out[4] = g.rigid;
  out[5] = (int32_t)g.rigid_mats.kind;
  out[6] = g.rigid_mats.kind == MatSet::ONE ? (int32_t)g.rigid_mats.bit : 0;
  out[7] = p.rigid && p.rigid_mats == g.rigid_mats;
}

}  // namespace lp
