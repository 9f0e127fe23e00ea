// tests/cpp/tiled_plan_host.cpp — taichi_mpm_amd/csrc/tiled_plan.h on the host, header only: the planner of a tiled run.  Wrappers
// through which tests/test_tiled_plan_cpu.py holds plans, slack and schedule against the Python model (taichi_mpm_amd/tiled.py:
// Partition) and checks the invariants of plans with per-rank occupancy on partitions it draws; and scenarios whose numbers are
// written out by hand: plans and interiors, the arena, the migration table, the decisions after a migration, the validation.
// Every scenario returns 0 or the line of the first check that failed; main() runs them all, and the invariants on partitions of
// its own, as a program of its own (built with -fsanitize=address,undefined).
#include "../../taichi_mpm_amd/csrc/tiled_plan.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(cond) do { if (!(cond)) return __LINE__; } while (0)

using namespace tplan;

namespace {
// a partition as the tests hand it over (ctypes mirror: tests/test_tiled_plan_cpu.py: Spec)
struct Spec {
  int32_t res[3], dims[3], cuts[3][MPMHIP_MAX_PARTS + 1], margin;
};
std::string make(const Spec &s, int rank, Partition &part) {
  const int32_t *const cuts[3] = {s.cuts[0], s.cuts[1], s.cuts[2]};
  return part.init(s.res, s.dims, cuts, s.margin, rank);
}
Spec spec(int rx, int ry, int rz, int dx, int dy, int dz, int margin) {
  Spec s;
  memset(&s, 0, sizeof s);
  const int res[3] = {rx, ry, rz}, dims[3] = {dx, dy, dz};
  for (int a = 0; a < 3; a++) {
    s.res[a] = res[a]; s.dims[a] = dims[a];
    for (int k = 0; k <= dims[a]; k++) s.cuts[a][k] = k == dims[a] ? res[a] : (res[a] * k) / dims[a];  // even cuts
  }
  s.margin = margin;
  return s;
}
bool same3(const int *v, int a, int b, int c) { return v[0] == a && v[1] == b && v[2] == c; }
bool same6(const int *v, int a, int b, int c, int d, int e, int f) { return same3(v, a, b, c) && same3(v + 3, d, e, f); }
bool in_box(const int *lo, const int *hi, int x, int y, int z) { return x >= lo[0] && x < hi[0] && y >= lo[1] && y < hi[1] && z >= lo[2] && z < hi[2]; }

// a migration table [world][ROW] as the ranks publish it
struct Table {
  int world;
  std::vector<uint32_t> h;
  explicit Table(int w) : world(w), h((size_t)w * ROW, 0) {
    for (int r = 0; r < w; r++) { row(r, 1 << 30, 1 << 30, 1 << 30, -(1 << 30), -(1 << 30), -(1 << 30)); h[(size_t)r * ROW + w + 7] = 1000; }  // no particles
  }
  void row(int r, int l0, int l1, int l2, int h0, int h1, int h2) {
    const int b[6] = {l0, l1, l2, h0, h1, h2};
    for (int k = 0; k < 6; k++) h[(size_t)r * ROW + world + k] = (uint32_t)b[k];
  }
  void count(int r, int s, uint32_t n) { h[(size_t)r * ROW + s] = n; }
  void speed(int r, float v) { memcpy(&h[(size_t)r * ROW + world + 6], &v, 4); }
  void room(int r, uint32_t n) { h[(size_t)r * ROW + world + 7] = n; }
  Mig decode(int me) const { Mig M; M.decode(h.data(), world, me); return M; }
};
}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------- wrappers
// "" or the validator's message
const char *tp_validate(const Spec *s, int rank) {
  static std::string msg;
  Partition part;
  msg = make(*s, rank, part);
  return msg.c_str();
}
// the linked plan of `rank`: boxes[i] = peer, lo3, hi3; offs[i] = vol, off, peer_off.  Returns the number of boxes, -1 - fault kind,
// or -100 if the partition is refused
int tp_plan(const Spec *s, const int *clip_lo, const int *clip_hi, const int *occ, int rank, uint64_t halo_cap, int cap, int *boxes,
            uint64_t *offs, uint64_t *total) {
  Partition part;
  if (!make(*s, rank, part).empty()) return -100;
  Plan p = plan(part, clip_lo, clip_hi, occ, rank);
  const PlanFault f = link(p, part, clip_lo, clip_hi, occ, rank, halo_cap);
  if (f.kind != PlanFault::NONE) return -1 - (int)f.kind;
  *total = p.total;
  for (int i = 0; i < (int)p.boxes.size() && i < cap; i++) {
    const Box &b = p.boxes[i];
    boxes[7 * i] = b.peer;
    for (int a = 0; a < 3; a++) { boxes[7 * i + 1 + a] = b.lo[a]; boxes[7 * i + 4 + a] = b.hi[a]; }
    offs[3 * i] = b.vol; offs[3 * i + 1] = b.off; offs[3 * i + 2] = b.peer_off;
  }
  return (int)p.boxes.size();
}
int tp_clip_slack(int margin) { return clip_slack(margin); }
int64_t tp_next_interval(int migrate_interval, int adaptive_cap, int margin, float speed) { return next_interval(migrate_interval, adaptive_cap, margin, speed); }

// the invariants of all ranks' plans under a clip box and occupancy boxes (occ: [world][6] or null), by enumeration of nodes
int tp_invariants(const Spec *s, const int *clip_lo, const int *clip_hi, const int *occ) {
  Partition part;
  CHECK(make(*s, 0, part).empty());
  const int world = part.world();
  std::vector<Plan> plans((size_t)world);
  std::vector<int> nb((size_t)world * 6);
  for (int r = 0; r < world; r++) {
    plans[r] = plan(part, clip_lo, clip_hi, occ, r);
    CHECK(link(plans[r], part, clip_lo, clip_hi, occ, r, ~0ull).kind == PlanFault::NONE);
    node_box(part, clip_lo, clip_hi, occ, r, &nb[(size_t)r * 6], &nb[(size_t)r * 6 + 3]);
  }
  const int nblk[3] = {(part.res[0] + 1) / 4 + 1, (part.res[1] + 1) / 4 + 1, (part.res[2] + 1) / 4 + 1};
  std::vector<char> touched;
  for (int r = 0; r < world; r++) {
    const Plan &p = plans[r];
    const int *rlo = &nb[(size_t)r * 6], *rhi = rlo + 3;
    // sorted by peer, tiling [0, total) without gaps; box(R, S) and box(S, R) are the same node set, each at the other's peer_off
    std::vector<int> of_peer((size_t)world, -1);
    uint64_t run = 0;
    for (size_t i = 0; i < p.boxes.size(); i++) {
      const Box &b = p.boxes[i];
      CHECK(b.peer >= 0 && b.peer < world && b.peer != r && (i == 0 || b.peer > p.boxes[i - 1].peer));
      CHECK(b.off == run && b.vol == (uint64_t)(b.hi[0] - b.lo[0]) * (b.hi[1] - b.lo[1]) * (b.hi[2] - b.lo[2]) && b.vol > 0);
      run += b.vol;
      of_peer[b.peer] = (int)i;
      const Box *q = nullptr;
      for (const Box &c : plans[b.peer].boxes) if (c.peer == r) q = &c;
      CHECK(q && same3(q->lo, b.lo[0], b.lo[1], b.lo[2]) && same3(q->hi, b.hi[0], b.hi[1], b.hi[2]));
      CHECK(q->off == b.peer_off && q->peer_off == b.off);
      // the 4^3 blocks the box touches, counted by marking the block of every node
      touched.assign((size_t)nblk[0] * nblk[1] * nblk[2], 0);
      uint32_t count = 0;
      for (int x = b.lo[0]; x < b.hi[0]; x++)
        for (int y = b.lo[1]; y < b.hi[1]; y++)
          for (int z = b.lo[2]; z < b.hi[2]; z++) {
            char &t = touched[((size_t)(x / 4) * nblk[1] + y / 4) * nblk[2] + z / 4];
            count += !t;
            t = 1;
          }
      const int dim[3] = {b.hi[0] - b.lo[0], b.hi[1] - b.lo[1], b.hi[2] - b.lo[2]};
      CHECK(box_blocks_of(b.lo, dim) == count);
    }
    CHECK(run == p.total);
    const Interior I = interior_of(part, clip_lo, clip_hi, occ, r, p);
    CHECK(I.boff.size() == p.boxes.size() && I.nodes == p.total);
    uint32_t blocks = 0;
    for (size_t i = 0; i < p.boxes.size(); i++) {
      const Box &b = p.boxes[i];
      const int dim[3] = {b.hi[0] - b.lo[0], b.hi[1] - b.lo[1], b.hi[2] - b.lo[2]};
      CHECK(I.boff[i] == blocks);
      blocks += box_blocks_of(b.lo, dim);
    }
    CHECK(I.box_blocks == blocks);
    // every node of the rank's node box and one layer around it (inside the grid): in box(R, S) exactly when in both cut node
    // boxes; in the interior only if in the node box and in no box
    int elo[3], ehi[3];
    for (int a = 0; a < 3; a++) { elo[a] = std::max(0, std::min(rlo[a], I.lo[a]) - 1); ehi[a] = std::min(part.res[a] + 1, std::max(rhi[a], I.hi[a]) + 1); }
    for (const Box &b : p.boxes)  // (a box outside that hull would go unseen below)
      for (int a = 0; a < 3; a++) CHECK(b.lo[a] >= rlo[a] && b.hi[a] <= rhi[a]);
    for (int x = elo[0]; x < ehi[0]; x++)
      for (int y = elo[1]; y < ehi[1]; y++)
        for (int z = elo[2]; z < ehi[2]; z++) {
          const bool in_r = in_box(rlo, rhi, x, y, z);
          bool in_any = false;
          for (int q = 0; q < world; q++) {
            if (q == r) continue;
            const bool both = in_r && in_box(&nb[(size_t)q * 6], &nb[(size_t)q * 6 + 3], x, y, z);
            const bool boxed = of_peer[q] >= 0 && in_box(p.boxes[of_peer[q]].lo, p.boxes[of_peer[q]].hi, x, y, z);
            CHECK(both == boxed);
            in_any = in_any || boxed;
          }
          if (in_box(I.lo, I.hi, x, y, z)) CHECK(in_r && !in_any);
        }
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------- plans and interiors by hand
// (a) two bricks cut at x = 32 on a 64^3 grid, margin 2, the whole grid as clip box, no occupancy: one face box
int tp_two_bricks() {
  Partition part;
  CHECK(make(spec(64, 64, 64, 2, 1, 1, 2), 0, part).empty());
  const int lo[3] = {0, 0, 0}, hi[3] = {65, 65, 65};
  int pc[3], blo[3], bhi[3];
  part.coords(1, pc);
  part.brick(1, blo, bhi);
  CHECK(part.world() == 2 && same3(pc, 1, 0, 0) && same3(blo, 32, 0, 0) && same3(bhi, 64, 64, 64));
  int nlo[3], nhi[3];
  node_box(part, lo, hi, nullptr, 0, nlo, nhi);
  CHECK(same3(nlo, 0, 0, 0) && same3(nhi, 36, 65, 65));
  node_box(part, lo, hi, nullptr, 1, nlo, nhi);
  CHECK(same3(nlo, 30, 0, 0) && same3(nhi, 65, 65, 65));
  for (int r = 0; r < 2; r++) {
    Plan p = plan(part, lo, hi, nullptr, r);
    CHECK(link(p, part, lo, hi, nullptr, r, 25350).kind == PlanFault::NONE);
    CHECK(p.boxes.size() == 1 && p.total == 25350);
    const Box &b = p.boxes[0];
    CHECK(b.peer == 1 - r && same3(b.lo, 30, 0, 0) && same3(b.hi, 36, 65, 65) && b.vol == 25350 && b.off == 0 && b.peer_off == 0);
    const Interior I = interior_of(part, lo, hi, nullptr, r, p);  // the node box minus the slab
    if (r == 0) CHECK(same3(I.lo, 0, 0, 0) && same3(I.hi, 30, 65, 65));
    else CHECK(same3(I.lo, 36, 0, 0) && same3(I.hi, 65, 65, 65));
    CHECK(I.boff.size() == 1 && I.boff[0] == 0 && I.box_blocks == 2 * 17 * 17 && I.nodes == 25350);
    // what can be wrong with a plan comes back as a result
    Plan q = plan(part, lo, hi, nullptr, r);
    CHECK(link(q, part, lo, hi, nullptr, r, 25349).kind == PlanFault::EXCEEDS_ARENA);
  }
  return 0;
}
// (b) the same partition, rank 0's occupancy a strict sub-box of its brick in y and z: the face box spans the CUT node box on y and z
// and leaves an interior that stops at the box's low x face; against the uncut node box (brick +- margin, clipped to the grid only:
// what mpmhip_set_halo hands over) the same box ends inside y and z and takes the whole interior away.  Both pinned.
int tp_occupancy_cut_interior() {
  Partition part;
  CHECK(make(spec(64, 64, 64, 2, 1, 1, 2), 0, part).empty());
  const int lo[3] = {0, 0, 0}, hi[3] = {65, 65, 65};
  const int occ[12] = {0, 10, 12, 65, 40, 44, 0, 0, 0, 65, 65, 65};
  Plan p = plan(part, lo, hi, occ, 0);
  CHECK(link(p, part, lo, hi, occ, 0, 1u << 20).kind == PlanFault::NONE);
  CHECK(p.boxes.size() == 1 && p.total == 5760);
  CHECK(p.boxes[0].peer == 1 && same3(p.boxes[0].lo, 30, 10, 12) && same3(p.boxes[0].hi, 36, 40, 44));
  const Interior cut = interior_of(part, lo, hi, occ, 0, p);
  CHECK(same3(cut.lo, 0, 10, 12) && same3(cut.hi, 30, 40, 44));
  const int ulo[3] = {0, 0, 0}, uhi[3] = {36, 65, 65};
  const Interior uncut = interior(ulo, uhi, p.boxes.data(), p.boxes.size());
  CHECK(same3(uncut.lo, 0, 0, 0) && same3(uncut.hi, 0, 0, 0));
  CHECK(cut.box_blocks == uncut.box_blocks && cut.box_blocks == 2 * 8 * 8 && cut.nodes == 5760 && uncut.nodes == 5760);  // x 30..35, y 10..39, z 12..43
  return 0;
}
// (c) three ranks in a row: the middle rank's box to each side leaves an interior between them
int tp_three_in_a_row() {
  Partition part;
  CHECK(make(spec(96, 16, 16, 3, 1, 1, 2), 0, part).empty());
  const int lo[3] = {0, 0, 0}, hi[3] = {97, 17, 17};
  Plan p[3];
  for (int r = 0; r < 3; r++) {
    p[r] = plan(part, lo, hi, nullptr, r);
    CHECK(link(p[r], part, lo, hi, nullptr, r, 3468).kind == PlanFault::NONE);
  }
  CHECK(p[0].boxes.size() == 1 && p[1].boxes.size() == 2 && p[2].boxes.size() == 1 && p[1].total == 3468 && p[0].total == 1734);
  CHECK(p[1].boxes[0].peer == 0 && same3(p[1].boxes[0].lo, 30, 0, 0) && same3(p[1].boxes[0].hi, 36, 17, 17) && p[1].boxes[0].off == 0);
  CHECK(p[1].boxes[1].peer == 2 && same3(p[1].boxes[1].lo, 62, 0, 0) && same3(p[1].boxes[1].hi, 68, 17, 17) && p[1].boxes[1].off == 1734);
  CHECK(p[1].boxes[0].peer_off == 0 && p[1].boxes[1].peer_off == 0);
  CHECK(p[0].boxes[0].peer == 1 && p[0].boxes[0].peer_off == 0 && p[2].boxes[0].peer == 1 && p[2].boxes[0].peer_off == 1734);
  const Interior I = interior_of(part, lo, hi, nullptr, 1, p[1]);
  CHECK(same3(I.lo, 36, 0, 0) && same3(I.hi, 62, 17, 17));
  CHECK(I.boff[0] == 0 && I.boff[1] == 2 * 5 * 5 && I.box_blocks == 2 * 2 * 5 * 5);  // x 30..35 and 62..67: two blocks each; 0..16: five
  return 0;
}
// (d) a box strictly inside the node box on one axis: no interior.  So for a box that spans the node box on all three
int tp_no_interior() {
  const int nlo[3] = {0, 0, 0}, nhi[3] = {20, 20, 20};
  Box b;
  memset(&b, 0, sizeof b);
  b.lo[0] = 5; b.hi[0] = 10; b.hi[1] = 20; b.hi[2] = 20;
  Interior I = interior(nlo, nhi, &b, 1);
  CHECK(same3(I.lo, 0, 0, 0) && same3(I.hi, 0, 0, 0) && I.box_blocks == 2 * 5 * 5 && I.nodes == 5 * 20 * 20);  // x 5..9: blocks 1 and 2
  b.lo[0] = 0; b.hi[0] = 20;
  I = interior(nlo, nhi, &b, 1);
  CHECK(same3(I.lo, 0, 0, 0) && same3(I.hi, 0, 0, 0));
  I = interior(nlo, nhi, (const Box *)nullptr, 0);  // no box: the node box
  CHECK(same3(I.lo, 0, 0, 0) && same3(I.hi, 20, 20, 20) && I.box_blocks == 0 && I.nodes == 0);
  return 0;
}

// ---------------------------------------------------------------------------------------------- arena
int tp_arena() {
  const Arena A(1000, 65536);
  // flags 4096 | 2 reduction tables of 64 rows of 16 doubles | 2 migration tables of 64 rows of 72 words | 2 receive buffers of
  // 1000 float4 (16000 bytes, rounded up to 63 * 256) | 65536 records of 176 bytes
  CHECK(A.flags == 0 && A.red[0] == 4096 && A.red[1] == 12288);
  CHECK(A.table[0] == 20480 && A.table[1] == 38912 && A.table_bytes == 18432);
  CHECK(A.recv[0] == 57344 && A.recv[1] == 73472 && A.recv_bytes == 16128);
  CHECK(A.inbox == 89600 && A.inbox_bytes == 11534336 && A.total == 11623936);
  CHECK(FLAG_BYTES == 4096 && RED_BYTES == 16384 && ROW == 72 && MAX_WORLD == 64 && MIG_FLOAT4 == 11);
  const size_t sec[8][2] = {{A.flags, FLAG_BYTES}, {A.red[0], RED_BYTES / 2}, {A.red[1], RED_BYTES / 2}, {A.table[0], A.table_bytes},
                            {A.table[1], A.table_bytes}, {A.recv[0], A.recv_bytes}, {A.recv[1], A.recv_bytes}, {A.inbox, A.inbox_bytes}};
  for (int i = 0; i < 8; i++) {
    CHECK(sec[i][0] % 256 == 0);
    CHECK(i == 0 || sec[i][0] == sec[i - 1][0] + sec[i - 1][1]);  // in this order, back to back: no two overlap
  }
  CHECK(sec[7][0] + sec[7][1] == A.total);
  // the layout is a function of the two capacities alone, and the capacity of the job's partition alone: every rank's is the same
  Partition part;
  uint64_t cap[2] = {0, 0};
  for (int r = 0; r < 2; r++) {
    CHECK(make(spec(64, 64, 64, 2, 1, 1, 2), r, part).empty());
    CHECK(worst_halo_cap(part, &cap[r]) == nullptr);
  }
  CHECK(cap[0] == 25350 && cap[1] == 25350);
  // one rank: no box, one node of capacity
  CHECK(make(spec(16, 16, 16, 1, 1, 1, 2), 0, part).empty());
  CHECK(worst_halo_cap(part, &cap[0]) == nullptr && cap[0] == 1);
  // 2048^3 cut in two: the face box is 2049^2 nodes times 2 margin + 2 layers: 510 layers stay below 2^31 nodes, 512 do not
  CHECK(make(spec(2048, 2048, 2048, 2, 1, 1, 254), 0, part).empty());
  CHECK(worst_halo_cap(part, &cap[0]) == nullptr && cap[0] == 2141184510ull);
  CHECK(make(spec(2048, 2048, 2048, 2, 1, 1, 255), 0, part).empty());
  cap[0] = 7;
  const char *why = worst_halo_cap(part, &cap[0]);
  CHECK(why && std::string(why) == "halo boxes too large" && cap[0] == 7);
  return 0;
}

// ---------------------------------------------------------------------------------------------- migration table
// three ranks; rank 2 has no particles (lo > hi) and sends nothing
Table table3() {
  Table T(3);
  T.row(0, 4, 5, 6, 10, 11, 12); T.count(0, 1, 2); T.count(0, 2, 1); T.speed(0, 0.25f); T.room(0, 100);
  T.row(1, 20, 5, 6, 30, 11, 12); T.count(1, 0, 3); T.count(1, 2, 5); T.speed(1, 0.5f); T.room(1, 3);
  T.room(2, 50);
  return T;
}
int tp_mig_table() {
  const Table T = table3();
  const int64_t n_out[3] = {3, 8, 0}, n_in[3] = {3, 2, 6};
  const uint64_t send_off[3][3] = {{0, 0, 2}, {0, 3, 3}, {0, 0, 0}};
  const uint64_t ahead[3][3] = {{0, 0, 0}, {0, 2, 1}, {3, 2, 6}};  // [sender][destination]
  const int64_t counts[3][3] = {{0, 2, 1}, {3, 0, 5}, {0, 0, 0}};
  for (int me = 0; me < 3; me++) {
    const Mig M = T.decode(me);
    CHECK(M.world == 3 && M.total == 11 && M.n_out == n_out[me] && M.n_in == n_in[me] && M.speed == 0.5f);
    CHECK(same3(M.lo, 4, 5, 6) && same3(M.hi, 30, 11, 12));
    CHECK(same6(&M.rank_bounds[0], 4, 5, 6, 10, 11, 12) && same6(&M.rank_bounds[6], 20, 5, 6, 30, 11, 12));
    CHECK(!nonempty(&M.rank_bounds[12]) && nonempty(&M.rank_bounds[0]));
    CHECK(M.room[0] == 100 && M.room[1] == 3 && M.room[2] == 50);
    for (int r = 0; r < 3; r++)
      for (int s = 0; s < 3; s++) CHECK(M.count(r, s) == counts[r][s] && M.ahead[(size_t)r * 3 + s] == ahead[r][s]);
    for (int s = 0; s < 3; s++) CHECK(M.send_off[s] == send_off[me][s]);
    CHECK(M.admission().dest == -1);
  }
  // an inbox one record too small: refused, naming the destination, its arrivals and its room, for every rank alike
  const uint32_t arrivals[3] = {3, 2, 6};
  for (int d = 0; d < 3; d++) {
    Table U = table3();
    U.room(d, arrivals[d] - 1);
    for (int me = 0; me < 3; me++) {
      const Mig::Overflow o = U.decode(me).admission();
      CHECK(o.dest == d && o.arriving == arrivals[d] && o.room == arrivals[d] - 1);
    }
    U.room(d, arrivals[d]);
    CHECK(U.decode(0).admission().dest == -1);
  }
  // nobody has particles: joint bounds stay empty
  const Mig E = Table(2).decode(0);
  CHECK(E.total == 0 && E.lo[0] > E.hi[0] && E.speed == 0.0f);
  return 0;
}

// ---------------------------------------------------------------------------------------------- after a migration
// what tests/test_gpu_tiled.py observes on the device, replayed: res 64, two bricks cut at x = 32, margin 2
int tp_after_two_blobs() {
  Partition part;
  CHECK(make(spec(64, 64, 64, 2, 1, 1, 2), 0, part).empty());
  const int full_lo[3] = {0, 0, 0}, full_hi[3] = {65, 65, 65};
  // the planning scan of a job's first substep: no occupancy yet, two blobs far from the cut
  Table T(2);
  T.row(0, 12, 29, 29, 18, 35, 35);
  T.row(1, 46, 29, 29, 52, 35, 35);
  After A = after_migration(T.decode(0), full_lo, full_hi, nullptr, part);
  CHECK(A.kind == After::REPLAN && clip_slack(part.margin) == 12);
  CHECK(same3(A.clip_lo, 0, 17, 17) && same3(A.clip_hi, 65, 49, 49));
  CHECK(same6(&A.occ[0], 0, 17, 17, 32, 49, 49) && same6(&A.occ[6], 34, 17, 17, 65, 49, 49));
  for (int r = 0; r < 2; r++) CHECK(plan(part, A.clip_lo, A.clip_hi, A.occ.data(), r).boxes.empty());
  const After first = A;
  // rank 0 moves towards the cut: still held (30 + 2 <= 32), but no room ahead (30 + 4 + 3 > 32): a re-plan, and now they share a box
  T.row(0, 24, 29, 29, 30, 35, 35);
  A = after_migration(T.decode(1), first.clip_lo, first.clip_hi, first.occ.data(), part);
  CHECK(A.kind == After::REPLAN);
  CHECK(same3(A.clip_lo, 12, 17, 17) && same3(A.clip_hi, 65, 49, 49));
  CHECK(same6(&A.occ[0], 12, 17, 17, 44, 49, 49) && same6(&A.occ[6], 34, 17, 17, 65, 49, 49));
  for (int r = 0; r < 2; r++) {
    const Plan p = plan(part, A.clip_lo, A.clip_hi, A.occ.data(), r);
    CHECK(p.boxes.size() == 1 && p.total == 2048 && same3(p.boxes[0].lo, 34, 17, 17) && same3(p.boxes[0].hi, 36, 49, 49));
  }
  // beyond the occupancy in one step: the error, with who, where and the six numbers of the message
  T.row(0, 27, 29, 29, 33, 35, 35);
  A = after_migration(T.decode(0), first.clip_lo, first.clip_hi, first.occ.data(), part);
  CHECK(A.kind == After::LEFT && A.rank == 0 && A.axis == 0 && A.cells[0] == 27 && A.cells[1] == 33 && A.nodes[0] == 0 && A.nodes[1] == 32);
  T.row(0, 24, 29, 10, 30, 35, 35);  // ... and below the low side of z
  A = after_migration(T.decode(0), first.clip_lo, first.clip_hi, first.occ.data(), part);
  CHECK(A.kind == After::LEFT && A.rank == 0 && A.axis == 2 && A.cells[0] == 10 && A.cells[1] == 35 && A.nodes[0] == 17 && A.nodes[1] == 49);
  // without occupancy boxes the clip box stands in for them
  A = after_migration(T.decode(0), first.clip_lo, first.clip_hi, nullptr, part);
  CHECK(A.kind == After::LEFT && A.rank == 0 && A.axis == 2 && A.nodes[0] == 17 && A.nodes[1] == 49);
  // a side where the box ends at the grid is exempt: looking back (ohi == res + 1) and looking ahead (olo == 0, ohi == res + 1)
  T.row(0, 2, 29, 29, 10, 35, 35);
  T.row(1, 50, 29, 29, 64, 35, 35);
  A = after_migration(T.decode(0), first.clip_lo, first.clip_hi, first.occ.data(), part);
  CHECK(A.kind == After::KEEP);
  T.row(1, 38, 29, 29, 52, 35, 35);  // (the same distance from an inner side is not: 38 - 4 - 1 < 34)
  A = after_migration(T.decode(0), first.clip_lo, first.clip_hi, first.occ.data(), part);
  CHECK(A.kind == After::REPLAN);
  // nobody has particles: nothing to decide
  CHECK(after_migration(Table(2).decode(0), full_lo, full_hi, nullptr, part).kind == After::KEEP);
  return 0;
}
int tp_after_shrink() {
  Partition part;
  CHECK(make(spec(64, 64, 64, 2, 1, 1, 2), 0, part).empty());
  const int lo[3] = {0, 0, 0}, hi[3] = {65, 65, 65};
  const int occ[12] = {0, 0, 0, 65, 65, 65, 0, 0, 0, 65, 65, 65};  // the whole clip box
  // clusters far apart: the boxes in use (2 * 25350 nodes) against none at all
  Table T(2);
  T.row(0, 12, 29, 29, 18, 35, 35);
  T.row(1, 46, 29, 29, 52, 35, 35);
  After A = after_migration(T.decode(0), lo, hi, occ, part);
  CHECK(A.kind == After::REPLAN && same6(&A.occ[0], 0, 17, 17, 32, 49, 49) && same6(&A.occ[6], 34, 17, 17, 65, 49, 49));
  // clusters at the cut that fill y and z: the fresh boxes are the same 2 * 25350 nodes, and 2 * then >= now keeps the plan
  T.row(0, 20, 2, 2, 29, 60, 60);
  T.row(1, 34, 2, 2, 45, 60, 60);
  A = after_migration(T.decode(0), lo, hi, occ, part);
  CHECK(A.kind == After::KEEP);
  CHECK(same3(A.clip_lo, 8, 0, 0) && same3(A.clip_hi, 59, 65, 65) && same6(&A.occ[0], 8, 0, 0, 43, 65, 65) && same6(&A.occ[6], 22, 0, 0, 59, 65, 65));
  // ... two layers less in y: 2 * 6 * 63 * 65 = 49140 nodes, and 2 * 49140 >= 50700 is no halving either
  T.row(0, 20, 2, 2, 29, 49, 60);
  T.row(1, 34, 2, 2, 45, 49, 60);
  A = after_migration(T.decode(0), lo, hi, occ, part);
  CHECK(A.kind == After::KEEP && A.occ[4] == 63);
  // half of it and one node less: x 30..35 (6) times y 0..31 (32) times z 0..64 (65) = 12480 per rank, 4 * 12480 < 50700
  T.row(0, 20, 2, 2, 29, 18, 60);
  T.row(1, 34, 2, 2, 45, 18, 60);
  A = after_migration(T.decode(0), lo, hi, occ, part);
  CHECK(A.kind == After::REPLAN && A.occ[4] == 32);
  return 0;
}
int tp_after_arrivals() {
  Partition part;
  CHECK(make(spec(96, 64, 64, 3, 1, 1, 2), 0, part).empty());
  const int lo[3] = {0, 0, 0}, hi[3] = {97, 65, 65};
  // rank 1 sends rank 0 five records: rank 0's box takes rank 1's bounds in; rank 2 has no particles and gets none
  Table T(3);
  T.row(0, 12, 29, 29, 18, 35, 35);
  T.row(1, 30, 27, 29, 40, 33, 37);
  T.count(1, 0, 5);
  for (int me = 0; me < 3; me++) {
    const After A = after_migration(T.decode(me), lo, hi, nullptr, part);
    CHECK(A.kind == After::REPLAN && A.occ.size() == 18);
    CHECK(same3(A.clip_lo, 0, 15, 17) && same3(A.clip_hi, 54, 49, 51));
    CHECK(same6(&A.occ[0], 0, 15, 17, 54, 49, 51));
    CHECK(same6(&A.occ[6], 18, 15, 17, 54, 47, 51));
    CHECK(same6(&A.occ[12], 0, 0, 0, 0, 0, 0));
    CHECK(plan(part, A.clip_lo, A.clip_hi, A.occ.data(), 2).boxes.empty() && plan(part, A.clip_lo, A.clip_hi, A.occ.data(), 1).boxes.size() == 1);
  }
  // a rank without particles that receives some holds them from then on
  T.count(1, 2, 1);
  const After A = after_migration(T.decode(0), lo, hi, nullptr, part);
  CHECK(A.kind == After::REPLAN && same6(&A.occ[12], 18, 15, 17, 54, 47, 51));
  return 0;
}

// ---------------------------------------------------------------------------------------------- schedule
int tp_schedule() {
  CHECK(next_interval(4, 64, 4, 0.0f) == 64 && next_interval(4, 64, 4, 1e-12f) == 64);
  CHECK(next_interval(4, 64, 4, 0.1f) == 19);   // 0.5 * 4 / 0.1 (as a float: a little above 0.1)
  CHECK(next_interval(4, 64, 4, 5.0f) == 4);    // never sooner than the CFL schedule
  CHECK(next_interval(2, 0, 4, 0.001f) == 2);   // a fixed interval: no cap
  CHECK(next_interval(4, 64, 4, INFINITY) == 4 && next_interval(4, 64, 4, NAN) == 4);
  return 0;
}

// ---------------------------------------------------------------------------------------------- validation
int tp_validation() {
  const Spec good = spec(64, 48, 32, 2, 3, 1, 2);
  Partition part;
  CHECK(make(good, 5, part).empty());
  CHECK(part.world() == 6 && part.margin == 2 && same3(part.res, 64, 48, 32) && same3(part.dims, 2, 3, 1) && part.cuts[1][2] == 32);
  Spec s = good;
  s.dims[1] = 0;
  CHECK(make(s, 0, part) == "dims[1]=0 outside [1,16]");
  s.dims[1] = 17;
  CHECK(make(s, 0, part) == "dims[1]=17 outside [1,16]");
  s = good; s.cuts[1][2] = 16;
  CHECK(make(s, 0, part) == "cuts of axis 1 are not increasing");
  s = good; s.cuts[0][0] = 1;
  CHECK(make(s, 0, part) == "cuts of axis 0 do not cover [0,res)");
  s = good; s.cuts[2][1] = 31;
  CHECK(make(s, 0, part) == "cuts of axis 2 do not cover [0,res)");
  s = good; s.cuts[2][1] = 40;  // (beyond the grid is fine)
  CHECK(make(s, 0, part).empty());
  CHECK(make(good, -1, part) == "rank -1 of 6" && make(good, 6, part) == "rank 6 of 6");
  s = good; s.margin = 0;
  CHECK(make(s, 0, part) == "margin must be >= 1 cell");
  // one predicate for "halo boxes travel by peer writes"
  CHECK(peer_wire(MPMHIP_WIRE_IPC, false) && peer_wire(MPMHIP_WIRE_LOCAL, false) && !peer_wire(MPMHIP_WIRE_LOCAL, true) && !peer_wire(MPMHIP_WIRE_RCCL, false));
  return 0;
}
}

// the invariants on partitions of the program's own (the Python test draws many more): uneven cuts, a sub-box as clip box, occupancy
// boxes of which some are empty
static int invariants_of_own() {
  uint32_t seed = 12345;
  auto rnd = [&](int n) { seed = seed * 1664525u + 1013904223u; return (int)((seed >> 8) % (uint32_t)n); };
  const int dims[4][3] = {{2, 1, 1}, {2, 2, 2}, {1, 3, 1}, {4, 2, 1}};
  for (int it = 0; it < 12; it++) {
    Spec s;
    memset(&s, 0, sizeof s);
    int clip_lo[3], clip_hi[3];
    for (int a = 0; a < 3; a++) {
      s.res[a] = 8 + rnd(17); s.dims[a] = dims[it % 4][a];
      for (int k = 1; k <= s.dims[a]; k++) s.cuts[a][k] = s.cuts[a][k - 1] + 1 + rnd(2 * s.res[a] / s.dims[a]);
      s.cuts[a][s.dims[a]] = std::max(s.cuts[a][s.dims[a]], s.res[a]);
      clip_lo[a] = it % 2 ? rnd(s.res[a] / 2) : 0;
      clip_hi[a] = it % 2 ? clip_lo[a] + 1 + rnd(s.res[a] + 1 - clip_lo[a]) : s.res[a] + 1;
    }
    s.margin = 1 + rnd(4);
    const int world = s.dims[0] * s.dims[1] * s.dims[2];
    std::vector<int> occ((size_t)world * 6, 0);
    for (int r = 0; r < world; r++)
      if (rnd(4))
        for (int a = 0; a < 3; a++) { occ[r * 6 + a] = rnd(s.res[a]); occ[r * 6 + 3 + a] = occ[r * 6 + a] + 1 + rnd(s.res[a] + 1 - occ[r * 6 + a]); }
    if (const int line = tp_invariants(&s, clip_lo, clip_hi, it % 3 ? occ.data() : nullptr)) return line;
  }
  return 0;
}

int main() {
  int (*const all[])() = {tp_two_bricks, tp_occupancy_cut_interior, tp_three_in_a_row, tp_no_interior, tp_arena, tp_mig_table, tp_after_two_blobs,
                          tp_after_shrink, tp_after_arrivals, tp_schedule, tp_validation, invariants_of_own};
  const char *const names[] = {"tp_two_bricks", "tp_occupancy_cut_interior", "tp_three_in_a_row", "tp_no_interior", "tp_arena", "tp_mig_table",
                               "tp_after_two_blobs", "tp_after_shrink", "tp_after_arrivals", "tp_schedule", "tp_validation", "invariants_of_own"};
  int failed = 0;
  for (size_t i = 0; i < sizeof all / sizeof all[0]; i++)
    if (const int line = all[i]()) {
      std::printf("%s: check at line %d failed\n", names[i], line);
      failed = 1;
    }
  if (!failed) std::printf("tiled_plan: %zu scenarios ok\n", sizeof all / sizeof all[0]);
  return failed;
}
