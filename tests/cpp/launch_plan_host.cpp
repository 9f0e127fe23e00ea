// tests/cpp/launch_plan_host.cpp — taichi_mpm_amd/csrc/launch_plan.h on the host, header only: the environment switches (Knobs)
// and the plans of the four phases of a substep at both sides of every boundary of their rules.  The rules are restated here from
// the record (the host code as it stood before the header existed), not taken from the header.  Every scenario returns 0 or the
// line of the first check that failed; tests/test_launch_plan_cpu.py runs them through ctypes, and main() runs them all as a
// program of its own (built with -fsanitize=address,undefined).
#include "../../taichi_mpm_amd/csrc/launch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond) do { if (!(cond)) return __LINE__; } while (0)

using namespace lp;

namespace {
constexpr int64_t M = 1 << 20;
const int64_t SLOTS[] = {0, 1, 2 * M - 1, 2 * M, 6 * M - 1, 6 * M, 8 * M};
// masks: empty, each single material, visco alone (among them), sand + visco, sand + elastic
std::vector<uint32_t> masks() {
  std::vector<uint32_t> m = {0u};
  for (int t = MPMHIP_VISCO; t <= MPMHIP_ELASTIC; t++) m.push_back(1u << t);
  m.push_back(1u << MPMHIP_SAND | 1u << MPMHIP_VISCO);
  m.push_back(1u << MPMHIP_SAND | 1u << MPMHIP_ELASTIC);
  return m;
}
bool single(uint32_t m) { return m == 2u || m == 4u || m == 8u || m == 16u || m == 32u || m == 64u || m == 128u || m == 256u; }

const char *const NAMES[] = {"MPMHIP_G2P_WGS", "MPMHIP_P2G_WGS", "MPMHIP_GRID_WGS", "MPMHIP_GRID_WALK", "MPMHIP_G2P_PACKED",
                             "MPMHIP_RIGID_WGS", "MPMHIP_RIGID_CONCURRENT", "MPMHIP_RANK_RUNS_MUL", "MPMHIP_RANK_WGS", "MPMHIP_CT_BLOCKS",
                             "MPMHIP_CELL_ORDER", "MPMHIP_CELL_ORDER_WGS", "MPMHIP_SCAN_GRID", "MPMHIP_SORT_V1"};
void unset_all() { for (const char *n : NAMES) unsetenv(n); }
Knobs with(const char *name, const char *value) {
  unset_all();
  setenv(name, value, 1);
  const Knobs k = Knobs::from_env();
  unsetenv(name);
  return k;
}
int is_default(const Knobs &k) {
  CHECK(k.g2p_wgs == 0 && k.p2g_wgs == 16384 && k.grid_wgs == 0 && k.grid_walk == -1 && k.g2p_packed == -1);
  CHECK(k.rigid_wgs == 2048 && k.rigid_concurrent == 7 && k.rank_runs_mul == 3u && k.rank_wgs_cap == 4096u && k.ct_blocks == 0);
  CHECK(k.cell_order_form == 1 && k.cell_order_wgs == 24 && k.scan_grid == 0 && !k.sort_v1);
  return 0;
}
}  // namespace

extern "C" {
// every switch unset, at a value inside its clamp and at one outside; nothing is remembered between two reads
int lp_env() {
  unset_all();
  CHECK(is_default(Knobs()) == 0);
  CHECK(is_default(Knobs::from_env()) == 0);
  CHECK(with("MPMHIP_G2P_WGS", "1024").g2p_wgs == 1024 && with("MPMHIP_G2P_WGS", "0").g2p_wgs == 0 && with("MPMHIP_G2P_WGS", "-5").g2p_wgs == 0);
  CHECK(with("MPMHIP_P2G_WGS", "8192").p2g_wgs == 8192 && with("MPMHIP_P2G_WGS", "0").p2g_wgs == 16384 && with("MPMHIP_P2G_WGS", "-1").p2g_wgs == 16384);
  CHECK(with("MPMHIP_GRID_WGS", "512").grid_wgs == 512 && with("MPMHIP_GRID_WGS", "0").grid_wgs == 0 && with("MPMHIP_GRID_WGS", "-7").grid_wgs == 0);
  CHECK(with("MPMHIP_GRID_WALK", "0").grid_walk == 0 && with("MPMHIP_GRID_WALK", "2").grid_walk == 2 && with("MPMHIP_GRID_WALK", "-1").grid_walk == -1);
  CHECK(with("MPMHIP_GRID_WALK", "7").grid_walk == 7);  // (not clamped: the plans read 2, 0 and < 0)
  CHECK(with("MPMHIP_G2P_PACKED", "1").g2p_packed == 1 && with("MPMHIP_G2P_PACKED", "0").g2p_packed == 0 && with("MPMHIP_G2P_PACKED", "-1").g2p_packed == -1);
  CHECK(with("MPMHIP_RIGID_WGS", "4096").rigid_wgs == 4096 && with("MPMHIP_RIGID_WGS", "2").rigid_wgs == 2);
  CHECK(with("MPMHIP_RIGID_WGS", "1").rigid_wgs == 2048 && with("MPMHIP_RIGID_WGS", "0").rigid_wgs == 2048);
  CHECK(with("MPMHIP_RIGID_CONCURRENT", "0").rigid_concurrent == 0 && with("MPMHIP_RIGID_CONCURRENT", "3").rigid_concurrent == 3);
  CHECK(with("MPMHIP_RANK_RUNS_MUL", "5").rank_runs_mul == 5u && with("MPMHIP_RANK_RUNS_MUL", "0").rank_runs_mul == 0u);
  CHECK(with("MPMHIP_RANK_WGS", "100").rank_wgs_cap == 100u && with("MPMHIP_RANK_WGS", "0").rank_wgs_cap == 1u && with("MPMHIP_RANK_WGS", "-3").rank_wgs_cap == 1u);
  CHECK(with("MPMHIP_CT_BLOCKS", "32").ct_blocks == 32 && with("MPMHIP_CT_BLOCKS", "48").ct_blocks == 48);  // (48: kept, ignored by plan_sort)
  CHECK(with("MPMHIP_CELL_ORDER", "0").cell_order_form == 0 && with("MPMHIP_CELL_ORDER", "1").cell_order_form == 1 && with("MPMHIP_CELL_ORDER", "5").cell_order_form == 1);
  CHECK(with("MPMHIP_CELL_ORDER_WGS", "8").cell_order_wgs == 8 && with("MPMHIP_CELL_ORDER_WGS", "0").cell_order_wgs == 1 && with("MPMHIP_CELL_ORDER_WGS", "-2").cell_order_wgs == 1);
  CHECK(with("MPMHIP_SCAN_GRID", "100").scan_grid == 100 && with("MPMHIP_SCAN_GRID", "-1").scan_grid == -1);
  CHECK(with("MPMHIP_SORT_V1", "1").sort_v1 && !with("MPMHIP_SORT_V1", "0").sort_v1);
  // a switch touches its own field only, and the next read does not remember it
  Knobs k = with("MPMHIP_RIGID_WGS", "512");
  k.rigid_wgs = 2048;
  CHECK(is_default(k) == 0);
  CHECK(is_default(Knobs::from_env()) == 0);
  return 0;
}

int lp_sort() {
  for (int64_t n : SLOTS)
    for (int keyed_table = 0; keyed_table < 2; keyed_table++)
      for (uint32_t nbw : {1u, 1u << 16, 1u << 19})  // block spaces of 32 (rounded up), 2^21 and 2^24
        for (int v1 = 0; v1 < 2; v1++)
          for (int ctb : {0, 16, 32, 64, 48})
            for (int walk : {-1, 0, 2})
              for (int tiled = 0; tiled < 2; tiled++) {
                Knobs k;
                k.sort_v1 = v1 != 0; k.ct_blocks = ctb; k.grid_walk = walk;
                Facts f;
                f.n_slots = n; f.keyed_table = keyed_table != 0; f.nbw = nbw; f.tiled = tiled != 0; f.max_blocks = 21000;
                const SortPlan p = plan_sort(k, f);
                const bool keyed = keyed_table && nbw <= (1u << 16) && !v1;
                CHECK(p.keyed == keyed);
                const int ct = (ctb == 16 || ctb == 32 || ctb == 64) ? ctb : ((keyed || n < 2 * M) ? 16 : (n < 6 * M ? 32 : 64));
                CHECK(p.ct == ct);
                CHECK(p.build_list == (walk == 2 || (walk < 0 && (tiled || n < 2 * M))));
                CHECK(p.bt_chunks == (nbw + 255) / 256 && p.ct_chunks == (21000u + ct - 1) / ct);
              }
  // rank role: ceil(n / 1024) workgroups inside [1, cap]
  for (uint32_t cap : {1u, 100u, 4096u}) {
    Knobs k;
    k.rank_wgs_cap = cap;
    Facts f;
    const int64_t ns[] = {0, 1, 1024, 1025, 100 * 1024, 100 * 1024 + 1, 2 * M - 1, 2 * M, 6 * M - 1, 6 * M, 8 * M};
    for (int64_t n : ns) {
      f.n_slots = n;
      const uint32_t want = (uint32_t)((n + 1023) / 1024);
      CHECK(plan_sort(k, f).rank_wgs == (want < 1u ? 1u : (want > cap ? cap : want)));
    }
  }
  // cell order (deterministic mode): form 0 min(8192, ceil(64 max_blocks / 256)), form 1 max(1, min(n_cus * wgs, ceil(max_blocks / 4)))
  for (uint32_t mb : {0u, 1u, 3u, 4u, 5u, 21000u, 32767u, 32768u, 32769u, 1u << 21})
    for (int n_cus : {1, 256, 304})
      for (int wgs : {1, 24}) {
        Knobs k;
        k.cell_order_wgs = wgs;
        Facts f;
        f.max_blocks = mb; f.n_cus = n_cus;
        k.cell_order_form = 0;
        const uint64_t c0 = ((uint64_t)mb * 64 + 255) / 256;
        CHECK(plan_sort(k, f).cell_order_form == 0 && plan_sort(k, f).cell_order_wgs == (int)(c0 < 8192 ? c0 : 8192));
        k.cell_order_form = 1;
        const uint64_t a = (uint64_t)n_cus * wgs, b = ((uint64_t)mb + 3) / 4, c1 = a < b ? a : b;
        CHECK(plan_sort(k, f).cell_order_form == 1 && plan_sort(k, f).cell_order_wgs == (int)(c1 < 1 ? 1 : c1));
      }
  return 0;
}

int lp_p2g() {
  for (uint32_t mask : masks())
    for (int rigid = 0; rigid < 2; rigid++)
      for (int det = 0; det < 2; det++)
        for (int wgs : {16384, 8192})
          for (int rw : {2048, 2, 4096}) {
            Knobs k;
            k.p2g_wgs = wgs; k.rigid_wgs = rw;
            Facts f;
            f.mask = mask; f.rigid = rigid != 0; f.deterministic = det != 0;
            const P2GPlan p = plan_p2g(k, f);
            CHECK(p.wgs == wgs && p.rigid == (rigid != 0) && p.rigid_wgs == rw);
            if (det) CHECK(p.rigid_mats.kind == MatSet::ALL_DET);
            else if (single(mask)) CHECK(p.rigid_mats.kind == MatSet::ONE && p.rigid_mats.bit == mask);  // (visco alone included)
            else CHECK(p.rigid_mats.kind == MatSet::ALL);
          }
  return 0;
}

int lp_grid() {
  for (int mode = 0; mode <= 5; mode++)
    for (int list_valid = 0; list_valid < 2; list_valid++)
      for (int64_t n : SLOTS)
        for (int boxes = 0; boxes < 2; boxes++)
          for (int sdf = 0; sdf < 2; sdf++)
            for (int gw : {0, 512})
              for (uint32_t n_own : {0u, 1u, 200u, 100000u})
                for (uint32_t mb : {100u, 4096u, 21000u}) {
                  Knobs k;
                  k.grid_wgs = gw;
                  Facts f;
                  f.n_slots = n; f.has_boxes = boxes != 0; f.sampled_levelset = sdf != 0; f.n_own = n_own; f.max_blocks = mb;
                  const GridPlan p = plan_grid(k, f, mode, list_valid != 0);
                  const bool energy = mode == 4 || mode == 5;
                  if ((mode == 0 || energy) && list_valid) {
                    uint64_t o = n_own;
                    if (o == 0) o = (uint64_t)mb * 8 < 32768 ? (uint64_t)mb * 8 : 32768;
                    uint64_t w = (o + o / 8 + 3) / 4 + 8;
                    w = w < 64 ? 64 : (w > 8192 ? 8192 : w);
                    CHECK(p.walk == GridWalk::LIST && !p.refuse_energy_on_tiled);
                    CHECK(p.wgs == (gw > 0 ? gw : (int)w));
                    CHECK(p.sampled == (mode == 0 && sdf));
                  } else if (energy && boxes) {
                    CHECK(p.refuse_energy_on_tiled);
                  } else {
                    const bool per_cand = mode == 0 && n < 2 * M;
                    CHECK(!p.refuse_energy_on_tiled && p.walk == (per_cand ? GridWalk::PER_CAND : GridWalk::PER_BLOCK));
                    CHECK(p.wgs == ((gw > 0 && mode == 0) ? gw : (per_cand ? 16384 : 4096)));
                    CHECK(p.sampled == (mode == 0 && sdf));
                  }
                }
  // the list walk's launch by hand: nothing reported yet on a small and on a large ctx, one owner, 200, 10^5 (the cap)
  Knobs k;
  Facts f;
  f.max_blocks = 100; f.n_own = 0;
  CHECK(plan_grid(k, f, 0, true).wgs == 233);  // 800 owners assumed: (800 + 100 + 3) / 4 + 8
  f.max_blocks = 21000;
  CHECK(plan_grid(k, f, 0, true).wgs == 8192);  // 32 768 assumed: 9 224, cut
  f.n_own = 1;
  CHECK(plan_grid(k, f, 4, true).wgs == 64);
  f.n_own = 200;
  CHECK(plan_grid(k, f, 5, true).wgs == 65);  // (200 + 25 + 3) / 4 + 8
  f.n_own = 100000;
  CHECK(plan_grid(k, f, 0, true).wgs == 8192);
  return 0;
}

int lp_g2p() {
  struct Fill { uint32_t n_live, n_act; };
  const Fill fills[] = {{0, 0}, {448 * 21000 - 1, 21000}, {448 * 21000, 21000}, {5, 0}};
  for (int64_t n : SLOTS)
    for (uint32_t mask : masks())
      for (const Fill &fill : fills)
        for (int pk : {-1, 0, 1})
          for (int flags = 0; flags < 32; flags++)
            for (int phase = 0; phase <= 2; phase++)
              for (int gw : {0, 1000})
                for (int n_cus : {256, 304}) {
                  Knobs k;
                  k.g2p_packed = pk; k.g2p_wgs = gw;
                  Facts f;
                  f.n_slots = n; f.mask = mask; f.n_live = fill.n_live; f.n_act = fill.n_act; f.n_cus = n_cus;
                  f.rigid = flags & 1; f.store_b = flags & 2; f.tiled = flags & 4; f.has_chunk_blk = !(flags & 8); f.deterministic = flags & 16;
                  const G2PPlan p = plan_g2p(k, f, phase);
                  bool want = pk != 0;
                  if (pk < 0) want = n >= 2 * M && fill.n_act > 0 && (uint64_t)fill.n_live < 448ull * fill.n_act;
                  const bool visco = (mask & (1u << MPMHIP_VISCO)) != 0;
                  const bool packed = want && single(mask) && !visco && !f.rigid && !f.store_b && phase == 0 && !f.tiled && f.has_chunk_blk;
                  CHECK(p.packed == packed);
                  CHECK(p.store_b == f.store_b && p.rigid == f.rigid);
                  if (!f.store_b && single(mask)) CHECK(p.mats.kind == MatSet::ONE && p.mats.bit == mask);  // (visco alone included)
                  else CHECK(p.mats.kind == (visco ? MatSet::ALL : MatSet::NO_VISCO));  // (the empty mask: NO_VISCO)
                  CHECK(p.wgs == (gw > 0 ? gw : (n < 2 * M ? 768 : (packed ? 12 * n_cus : 4096))));
                  if (f.deterministic) CHECK(p.rigid_mats.kind == MatSet::ALL_DET);
                  else if (single(mask)) CHECK(p.rigid_mats.kind == MatSet::ONE && p.rigid_mats.bit == mask);
                  else CHECK(p.rigid_mats.kind == MatSet::ALL);
                  CHECK(p.rigid_wgs == 1024);
                }
  Knobs k;
  k.rigid_wgs = 2;
  CHECK(plan_g2p(k, Facts(), 0).rigid_wgs == 1);
  k.rigid_wgs = 4097;
  CHECK(plan_g2p(k, Facts(), 0).rigid_wgs == 2048);
  return 0;
}

// the configurations the project measures, written out by hand: the default bench line (256^3, 8 M sand particles, apic_b discarded,
// 256 CUs) on the seeded lattice and after the impact, and a 1 M-particle ctx
int lp_known_configurations() {
  const Knobs k;
  Facts f;
  f.n_slots = 8 * M; f.max_blocks = 178858; f.nbw = (1u << 21) / 32; f.n_cus = 256; f.mask = 1u << MPMHIP_SAND;
  f.keyed_table = true; f.has_chunk_blk = true;
  const SortPlan s = plan_sort(k, f);
  CHECK(s.keyed && !s.build_list && s.ct == 16 && s.rank_wgs == 4096u && s.bt_chunks == 256u && s.ct_chunks == 11179u);
  CHECK(plan_grid(k, f, 0, s.build_list).walk == GridWalk::PER_BLOCK && plan_grid(k, f, 0, s.build_list).wgs == 4096);
  CHECK(plan_p2g(k, f).wgs == 16384 && !plan_p2g(k, f).rigid);
  G2PPlan g = plan_g2p(k, f, 0);  // before the first sort has reported: per block
  CHECK(!g.packed && g.mats.kind == MatSet::ONE && g.mats.bit == (1u << MPMHIP_SAND) && g.wgs == 4096 && !g.store_b && !g.rigid);
  f.n_live = 8 * M; f.n_act = 16384;  // the lattice: 512 per block, full
  CHECK(!plan_g2p(k, f, 0).packed);
  f.n_act = 24000;  // after the impact: 350 per block
  g = plan_g2p(k, f, 0);
  CHECK(g.packed && g.wgs == 3072 && g.mats.kind == MatSet::ONE);
  f.keyed_table = false;  // (a device that could not spare the table: the four launches, 64 blocks per chunk at this size)
  CHECK(!plan_sort(k, f).keyed && plan_sort(k, f).ct == 64);
  f.keyed_table = true;
  f.n_slots = M; f.n_live = M; f.n_act = 2448; f.n_own = 9000;
  CHECK(plan_sort(k, f).build_list && plan_sort(k, f).rank_wgs == 1024u);
  CHECK(plan_grid(k, f, 0, true).walk == GridWalk::LIST && plan_grid(k, f, 0, true).wgs == 2540);  // (9000 + 1125 + 3) / 4 + 8
  CHECK(!plan_g2p(k, f, 0).packed && plan_g2p(k, f, 0).wgs == 768);
  return 0;
}

// The header's answer for one (Facts, Knobs) pair in the eight words of mpmhip_debug_transfer_plan: tests/test_launch_plan_cpu.py
// sweeps it to enumerate the forms of the transfer kernels a ctx can be given, and holds them against tests/kernel_forms.py.
// flags: 1 rigid, 2 store_b, 4 tiled, 8 deterministic, 16 no chunk table
void lp_transfer_plan(uint32_t mask, int64_t n_slots, uint32_t n_live, uint32_t n_act, int flags, int g2p_packed, int32_t out[8]) {
  Knobs k;
  k.g2p_packed = g2p_packed;
  Facts f;
  f.mask = mask; f.n_slots = n_slots; f.n_live = n_live; f.n_act = n_act;
  f.rigid = flags & 1; f.store_b = flags & 2; f.tiled = flags & 4; f.deterministic = flags & 8; f.has_chunk_blk = !(flags & 16);
  transfer_plan_words(k, f, out);
}

// the words by hand: the bench line after the impact, a mixed ctx beside a body with apic_b kept, the deterministic mode
int lp_transfer_words() {
  int32_t w[8];
  lp_transfer_plan(1u << MPMHIP_SAND, 8 * M, 8 * M, 24000, 0, -1, w);
  CHECK(w[0] == 1 && w[1] == 0 && w[2] == (1 << MPMHIP_SAND) && w[3] == 0 && w[4] == 0 && w[5] == 0 && w[6] == (1 << MPMHIP_SAND) && w[7] == 0);
  lp_transfer_plan(1u << MPMHIP_SAND | 1u << MPMHIP_VISCO, 4000, 0, 0, 1 | 2, 1, w);
  CHECK(w[0] == 0 && w[1] == 2 && w[2] == 0 && w[3] == 1 && w[4] == 1 && w[5] == 2 && w[6] == 0 && w[7] == 1);
  lp_transfer_plan(1u << MPMHIP_SAND | 1u << MPMHIP_ELASTIC, 4000, 0, 0, 1 | 8, -1, w);
  CHECK(w[0] == 0 && w[1] == 1 && w[2] == 0 && w[3] == 0 && w[4] == 1 && w[5] == 3 && w[6] == 0 && w[7] == 1);
  lp_transfer_plan(1u << MPMHIP_VISCO, 4000, 0, 0, 1, 1, w);  // visco alone: its own kernels, never the packed walk
  CHECK(w[0] == 0 && w[1] == 0 && w[2] == (1 << MPMHIP_VISCO) && w[4] == 1 && w[5] == 0 && w[6] == (1 << MPMHIP_VISCO) && w[7] == 1);
  return 0;
}

// (moved with the plans; mpmhip_debug_scan_grid forwards here and tests/test_host_cpu.py sweeps it through that export)
int lp_scan_grid() {
  CHECK(scan_resident_set(256, 5) == 1024u && scan_grid_for(256, 5, 0) == 480u && scan_grid_for(256, 5, 10000) == 640u);
  CHECK(scan_resident_set(256, 1) == 256u && scan_grid_for(256, 1, 0) == 96u && scan_grid_for(256, 0, 0) == 96u);
  CHECK(scan_resident_set(256, 12) == 1792u && scan_grid_for(256, 12, 0) == 1152u && scan_grid_for(0, 4, 7) == 2u);
  return 0;
}
}

int main() {
  int (*const all[])() = {lp_env, lp_sort, lp_p2g, lp_grid, lp_g2p, lp_known_configurations, lp_transfer_words, lp_scan_grid};
  const char *const names[] = {"lp_env", "lp_sort", "lp_p2g", "lp_grid", "lp_g2p", "lp_known_configurations", "lp_transfer_words", "lp_scan_grid"};
  int failed = 0;
  for (size_t i = 0; i < sizeof all / sizeof all[0]; i++)
    if (const int line = all[i]()) {
      std::printf("%s: check at line %d failed\n", names[i], line);
      failed = 1;
    }
  if (!failed) std::printf("launch_plan: %zu scenarios ok\n", sizeof all / sizeof all[0]);
  return failed;
}
