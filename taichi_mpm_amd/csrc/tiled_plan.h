// taichi_mpm_amd/csrc/tiled_plan.h — the planner of a tiled (multi-GPU) run: every decision of the native data plane (tiled_api.h)
// and of the tiling section of mpmhip.hip that is host arithmetic.  Plain C++17, no HIP: every function is a function of its
// arguments (no globals, no environment), so the same lines compile for the host in tests/cpp/tiled_plan_host.cpp, are held there
// against the Python model (taichi_mpm_amd/tiled.py: Partition) and run under the sanitizers.
//
//   partition   dims bricks with cell cut planes cuts[a]; rank = (px * dims[1] + py) * dims[2] + pz
//   plan        box(R, S) = node_box(R) ∩ node_box(S), node_box(R) = [brick.lo - margin, brick.hi + margin + 2) clipped to the clip
//               box AND to rank R's own occupancy box; sorted by peer.  Every rank can compute every rank's plan, so a writer knows
//               where a box lives in its reader's buffers (link)
//   interior    the part of a node box that no halo box touches: what the overlap split runs beside the exchange
//   arena       [flags | reduction tables | table 0 | table 1 | recv 0 | recv 1 | inbox], laid out alike on every rank of a job
//   rows        a job with CPIC rigid bodies: where the ranks' impulse rows live behind the nodes of recv 0 / recv 1, and their epoch words
//   migration   the table [world][ROW] every rank reads: counts, bounds, speed, inbox room; who writes where into which inbox
//   after it    do the occupancy boxes still hold the particles, will they until the next check, are they much too wide
//   re-cut      new cut planes from the live particles' histograms; the rounds and the capacity rule of the redistribution behind them
//   schedule    substeps until the next migration
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mpmhip.h"

#if !defined(MPM_HD)
#if defined(__HIPCC__)
#define MPM_HD __host__ __device__ __forceinline__
#else
#define MPM_HD inline
#endif
#endif

namespace tplan {

// grid blocks (4^3 nodes) a halo box [lo, lo + dim) touches per axis, and in all (the kernels' definition too: mpm_common.h)
MPM_HD int box_blocks_axis(int lo, int dim) { return ((lo + dim - 1) >> 2) - (lo >> 2) + 1; }
MPM_HD uint32_t box_blocks_of(const int lo[3], const int dim[3]) {
  return (uint32_t)box_blocks_axis(lo[0], dim[0]) * (uint32_t)box_blocks_axis(lo[1], dim[1]) * (uint32_t)box_blocks_axis(lo[2], dim[2]);
}

// halo boxes by peer writes: the IPC and the local wire — unless the local job carries them by RCCL self-sends (loop_rccl)
inline bool peer_wire(int wire, bool loop_rccl) { return (wire == MPMHIP_WIRE_IPC || wire == MPMHIP_WIRE_LOCAL) && !loop_rccl; }

// ------------------------------------------------------------------------------------------------ partition
struct Partition {
  int dims[3] = {1, 1, 1};
  int cuts[3][MPMHIP_MAX_PARTS + 1] = {};
  int margin = 1;
  int res[3] = {0, 0, 0};

  // fills the partition; the message of the first rule that does not hold (mpmhip_set_partition), or "" if all do
  std::string init(const int res_[3], const int32_t dims_[3], const int32_t *const cuts_[3], int margin_, int rank) {
    char buf[96];
    int w = 1;
    for (int a = 0; a < 3; a++) {
      if (dims_[a] < 1 || dims_[a] > MPMHIP_MAX_PARTS) return snprintf(buf, sizeof buf, "dims[%d]=%d outside [1,%d]", a, dims_[a], MPMHIP_MAX_PARTS), buf;
      dims[a] = dims_[a];
      res[a] = res_[a];
      w *= dims_[a];
      for (int k = 0; k <= dims_[a]; k++) {
        cuts[a][k] = cuts_[a][k];
        if (k > 0 && cuts_[a][k] <= cuts_[a][k - 1]) return snprintf(buf, sizeof buf, "cuts of axis %d are not increasing", a), buf;
      }
      if (cuts_[a][0] != 0 || cuts_[a][dims_[a]] < res_[a]) return snprintf(buf, sizeof buf, "cuts of axis %d do not cover [0,res)", a), buf;
    }
    if (rank < 0 || rank >= w) return snprintf(buf, sizeof buf, "rank %d of %d", rank, w), buf;
    if (margin_ < 1) return "margin must be >= 1 cell";
    margin = margin_;
    return "";
  }
  int world() const { return dims[0] * dims[1] * dims[2]; }
  void coords(int rank, int pc[3]) const {
    pc[0] = rank / (dims[1] * dims[2]); pc[1] = (rank / dims[2]) % dims[1]; pc[2] = rank % dims[2];
  }
  void brick(int rank, int lo[3], int hi[3]) const {  // cells
    int pc[3];
    coords(rank, pc);
    for (int a = 0; a < 3; a++) { lo[a] = cuts[a][pc[a]]; hi[a] = cuts[a][pc[a] + 1]; }
  }
};

// ------------------------------------------------------------------------------------------------ plan
struct Box { int peer; int lo[3], hi[3]; uint64_t vol, off, peer_off; };  // off / peer_off: float4 nodes into this rank's / the peer's buffers
struct Plan { std::vector<Box> boxes; uint64_t total = 0; };              // boxes sorted by peer; total = nodes of all of them

inline bool nonempty(const int *b) { return b[0] <= b[3] && b[1] <= b[4] && b[2] <= b[5]; }  // [6] = lo3, hi3 (inclusive bounds)

// node box of `rank` under a clip box (occ: [world][6] = lo3, hi3 of every rank's occupancy box in nodes, or nullptr: the clip box only)
inline void node_box(const Partition &part, const int clip_lo[3], const int clip_hi[3], const int *occ, int rank, int lo[3], int hi[3]) {
  int blo[3], bhi[3];
  part.brick(rank, blo, bhi);
  for (int a = 0; a < 3; a++) {
    lo[a] = std::max(clip_lo[a], blo[a] - part.margin);
    hi[a] = std::min(clip_hi[a], bhi[a] + part.margin + 2);
    if (occ) { lo[a] = std::max(lo[a], occ[rank * 6 + a]); hi[a] = std::min(hi[a], occ[rank * 6 + 3 + a]); }
  }
}
// halo boxes of `rank`, sorted by peer, with their offsets (float4 nodes) in the rank's buffers; peer_off is link()'s
inline Plan plan(const Partition &part, const int clip_lo[3], const int clip_hi[3], const int *occ, int rank) {
  Plan out;
  int alo[3], ahi[3];
  node_box(part, clip_lo, clip_hi, occ, rank, alo, ahi);
  const int world = part.world();
  for (int s = 0; s < world; s++) {
    if (s == rank) continue;
    int blo[3], bhi[3];
    node_box(part, clip_lo, clip_hi, occ, s, blo, bhi);
    Box b;
    bool any = true;
    for (int a = 0; a < 3; a++) {
      b.lo[a] = std::max(alo[a], blo[a]);
      b.hi[a] = std::min(ahi[a], bhi[a]);
      any = any && b.lo[a] < b.hi[a];
    }
    if (!any) continue;
    b.peer = s;
    b.vol = (uint64_t)(b.hi[0] - b.lo[0]) * (b.hi[1] - b.lo[1]) * (b.hi[2] - b.lo[2]);
    b.off = out.total;
    b.peer_off = 0;
    out.total += b.vol;
    out.boxes.push_back(b);
  }
  return out;
}
// where each box of `rank` lives in its peer's buffers: the peer's own plan.  What can be wrong with a plan comes back as a result
struct PlanFault { enum Kind { NONE, TOO_MANY_BOXES, EXCEEDS_ARENA, NO_COUNTERPART } kind = NONE; int peer = -1; };
inline PlanFault link(Plan &mine, const Partition &part, const int clip_lo[3], const int clip_hi[3], const int *occ, int rank, uint64_t halo_cap) {
  PlanFault f;
  if (mine.boxes.size() > MPMHIP_MAX_HALO_BOXES) { f.kind = PlanFault::TOO_MANY_BOXES; return f; }
  if (mine.total > halo_cap) { f.kind = PlanFault::EXCEEDS_ARENA; return f; }
  for (auto &b : mine.boxes) {
    bool found = false;
    for (const auto &q : plan(part, clip_lo, clip_hi, occ, b.peer).boxes)
      if (q.peer == rank) { b.peer_off = q.off; found = true; }
    if (!found) { f.kind = PlanFault::NO_COUNTERPART; f.peer = b.peer; return f; }
  }
  return f;
}

// ------------------------------------------------------------------------------------------------ interior
// The overlap-free interior [lo, hi) of the node box [nlo, nhi) among halo boxes (any type with lo[3], hi[3]): along every axis where
// a box is a proper sub-range of the node box the interior ends at the box; a box that spans the node box along an axis leaves the
// interior alone on that axis.  A box that ends inside the node box on both sides of an axis, or spans it on all three, leaves no
// interior (lo == hi).  boff: first grid block of each box in the concatenated block numbering (k_halo_pack: one wave per block).
struct Interior {
  int lo[3], hi[3];
  std::vector<uint32_t> boff;
  uint32_t box_blocks = 0;
  uint64_t nodes = 0;
};
template <class B>
Interior interior(const int nlo[3], const int nhi[3], const B *boxes, size_t n) {
  Interior I;
  for (int a = 0; a < 3; a++) { I.lo[a] = nlo[a]; I.hi[a] = nhi[a]; }
  I.boff.resize(n);
  bool empty = false;
  for (size_t i = 0; i < n; i++) {
    const B &b = boxes[i];
    bool proper = false;
    int dim[3];
    for (int a = 0; a < 3; a++) {
      dim[a] = b.hi[a] - b.lo[a];
      if (b.lo[a] <= nlo[a] && b.hi[a] >= nhi[a]) continue;
      proper = true;
      if (b.lo[a] <= nlo[a]) I.lo[a] = std::max(I.lo[a], (int)b.hi[a]);
      else if (b.hi[a] >= nhi[a]) I.hi[a] = std::min(I.hi[a], (int)b.lo[a]);
      else empty = true;
    }
    if (!proper) empty = true;
    I.boff[i] = I.box_blocks;
    const int lo[3] = {b.lo[0], b.lo[1], b.lo[2]};
    I.box_blocks += box_blocks_of(lo, dim);
    I.nodes += (uint64_t)dim[0] * dim[1] * dim[2];
  }
  if (empty) for (int a = 0; a < 3; a++) I.hi[a] = I.lo[a];
  return I;
}
// ... of a rank's planned boxes: the node box as the boxes were cut from it, clip box and occupancy included (work outside it
// does not exist: the rank has no particle there)
inline Interior interior_of(const Partition &part, const int clip_lo[3], const int clip_hi[3], const int *occ, int rank, const Plan &p) {
  int nlo[3], nhi[3];
  node_box(part, clip_lo, clip_hi, occ, rank, nlo, nhi);
  for (int a = 0; a < 3; a++) nhi[a] = std::max(nhi[a], nlo[a]);
  return interior(nlo, nhi, p.boxes.data(), p.boxes.size());
}

// ------------------------------------------------------------------------------------------------ arena
constexpr int MAX_WORLD = MPMHIP_MAX_HALO_BOXES;      // every other rank can be a halo peer
constexpr uint32_t ROW = MAX_WORLD + 8;               // words of a migration row: [counts(world) | lo3 | hi3 | speed | inbox capacity], padded
constexpr size_t FLAG_BYTES = 4096;                   // halo epochs [world] | table epochs [world] | record epochs [world] | reduction epochs [world]
constexpr int RED_N = MPMHIP_REDUCE_MAX_VALUES;       // doubles of one rank's row of a reduction (mpmhip_tiled_reduce)
constexpr size_t RED_BYTES = 2 * sizeof(double) * RED_N * MAX_WORLD;  // two tables of [world] rows (parity of the reduction)
constexpr size_t RED_PIN_WORD = 8192;                 // the staging of a reduction in the ctx's pinned page (behind the migration table)
constexpr size_t NODE_BYTES = 16;                     // a halo node travels as one float4
constexpr size_t MIG_FLOAT4 = 11;                     // float4 per migration record
static_assert(4 * MIG_FLOAT4 == MPMHIP_MIGRATE_FLOATS, "a migration record is MPMHIP_MIGRATE_FLOATS floats");

// ONE device allocation per rank, sized for the worst case (halo_cap: clip = the whole grid), so that it is allocated — and, for the
// IPC wire, mapped by the peers — exactly once.  Byte offsets from the arena's base; the tables are sized for MAX_WORLD ranks
// whatever the job's world, so every rank of every job with the same two capacities lays its arena out alike.
struct Arena {
  uint64_t halo_cap = 0, inbox_cap = 0;  // float4 nodes of one receive buffer; records of the inbox
  size_t flags = 0, red[2] = {0, 0}, table[2] = {0, 0}, recv[2] = {0, 0}, inbox = 0;
  size_t table_bytes = 0, recv_bytes = 0, inbox_bytes = 0, total = 0;
  Arena() {}
  Arena(uint64_t halo_cap_, uint64_t inbox_cap_) : halo_cap(halo_cap_), inbox_cap(inbox_cap_) {
    table_bytes = ((sizeof(uint32_t) * ROW * MAX_WORLD + 255) / 256) * 256;
    recv_bytes = ((NODE_BYTES * halo_cap + 255) / 256) * 256;
    inbox_bytes = NODE_BYTES * MIG_FLOAT4 * inbox_cap;
    red[0] = FLAG_BYTES; red[1] = red[0] + RED_BYTES / 2;
    table[0] = FLAG_BYTES + RED_BYTES; table[1] = table[0] + table_bytes;
    recv[0] = table[1] + table_bytes; recv[1] = recv[0] + recv_bytes;
    inbox = recv[1] + recv_bytes;
    total = inbox + inbox_bytes;
  }
};
// worst-case halo volume over all ranks: the clip box = the whole grid.  Returns why the partition is refused, or nullptr
inline const char *worst_halo_cap(const Partition &part, uint64_t *halo_cap) {
  const int full_lo[3] = {0, 0, 0}, full_hi[3] = {part.res[0] + 1, part.res[1] + 1, part.res[2] + 1};
  uint64_t cap = 0;
  for (int r = 0; r < part.world(); r++) {
    const Plan p = plan(part, full_lo, full_hi, nullptr, r);
    if (p.boxes.size() > MPMHIP_MAX_HALO_BOXES) return "too many halo boxes";
    cap = std::max(cap, p.total);
  }
  if (cap >= (1ull << 31)) return "halo boxes too large";
  *halo_cap = std::max<uint64_t>(cap, 1);
  return nullptr;
}

// ------------------------------------------------------------------------------------------------ impulse rows (bodies on a job)
// Every rank of a job with CPIC rigid bodies holds all bodies.  What a rank's colour-aware transfer kernels hand the bodies is the
// rank's ROW: impulse and torque of every body, IMP_ROW_FLOATS floats.  Twice a substep — behind the rigid P2G (exchange 0) and
// behind the rigid G2P (exchange 1) — the rows of all ranks reach every rank, which adds them in RANK ORDER and applies the sum.
// The rows live in the arena BEHIND the halo nodes: a job with bodies asks Arena() for a halo capacity larger by rows_extra_cap(world)
// float4s, the planner links its boxes against the capacity without them (rows_node_cap), and the table of exchange x and parity p
// begins rows_table_off(...) float4s into recv[p].  Arena(halo_cap, inbox) itself is what it was: a job without bodies asks for
// the capacity it asked for before.  The rows' epochs have words of their own in the flag page, behind the four arrays of [MAX_WORLD].
constexpr int IMP_ROW_FLOATS = 72;   // = MAX_RIGID * 6 (rigid_records.h; asserted where both are seen)
constexpr int IMP_ROW_FLOAT4 = IMP_ROW_FLOATS / 4;
constexpr int ROW_EXCHANGES = 2;     // 0: behind the rigid P2G, 1: behind the rigid G2P
static_assert(IMP_ROW_FLOATS % 4 == 0, "a row is whole float4s");
// float4s of one table: the rows of `world` ranks of one exchange and one parity
MPM_HD uint64_t rows_table_float4(int world) { return (uint64_t)world * IMP_ROW_FLOAT4; }
// float4s a job with bodies adds to the halo capacity it asks Arena() for: both exchanges' tables (the two recv buffers are the parities)
MPM_HD uint64_t rows_extra_cap(int world) { return ROW_EXCHANGES * rows_table_float4(world); }
// the halo capacity left for the nodes of an arena whose capacity includes the rows (bodies) or does not
MPM_HD uint64_t rows_node_cap(uint64_t halo_cap, int world, bool bodies) { return bodies ? halo_cap - rows_extra_cap(world) : halo_cap; }
// where rank `rank`'s row of exchange `exchange` begins, in float4s from recv[parity] of an arena with bodies
MPM_HD uint64_t rows_off(uint64_t halo_cap, int world, int exchange, int rank) {
  return rows_node_cap(halo_cap, world, true) + (uint64_t)exchange * rows_table_float4(world) + (uint64_t)rank * IMP_ROW_FLOAT4;
}
// the word of the flag page in which rank `rank` publishes the epoch of its row of `exchange` (on every rank's page)
MPM_HD uint32_t rows_flag_word(int exchange, int rank) { return (uint32_t)((4 + exchange) * MAX_WORLD + rank); }
static_assert((4 + ROW_EXCHANGES) * MAX_WORLD * sizeof(uint32_t) <= FLAG_BYTES, "the rows' epochs fit the flag page");

// ------------------------------------------------------------------------------------------------ migration table
struct Mig {
  int world = 0;
  std::vector<int64_t> counts;   // [world][world]: records rank r sends to rank s
  std::vector<int> rank_bounds;  // [world][6]: lo3, hi3 base cells of every rank's particles, before the records moved (none: lo > hi)
  std::vector<uint32_t> room;    // [world]: records every rank's inbox holds
  std::vector<uint64_t> ahead;   // [world][world]: records of ranks below r in the inbox of s — where r's records go there
  std::vector<uint64_t> send_off;  // [world]: where this rank's records for s begin in its send buffer (grouped by destination)
  int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // joint bounds of the ranks that have particles
  float speed = 0.0f;
  int64_t total = 0, n_out = 0, n_in = 0;  // records on the move in the whole job; out of / into rank `me`

  int64_t count(int r, int s) const { return counts[(size_t)r * world + s]; }
  // the [world][ROW] words of the table as rank `me` read them
  void decode(const uint32_t *h, int world_, int me) {
    world = world_;
    counts.assign((size_t)world * world, 0);
    rank_bounds.assign((size_t)world * 6, 0);
    room.assign((size_t)world, 0);
    ahead.assign((size_t)world * world, 0);
    send_off.assign((size_t)world, 0);
    total = 0;
    for (int a = 0; a < 3; a++) { lo[a] = 1 << 30; hi[a] = -(1 << 30); }
    speed = 0.0f;
    for (int r = 0; r < world; r++) {
      const uint32_t *row = h + (size_t)r * ROW;
      for (int s = 0; s < world; s++) { counts[(size_t)r * world + s] = row[s]; total += row[s]; }
      int *rb = &rank_bounds[(size_t)r * 6];
      for (int k = 0; k < 6; k++) rb[k] = (int)row[world + k];
      if (nonempty(rb))  // (a rank without particles reports lo > hi)
        for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], rb[a]); hi[a] = std::max(hi[a], rb[3 + a]); }
      float s;
      memcpy(&s, &row[world + 6], 4);
      if (s > speed) speed = s;
      room[r] = row[world + 7];
    }
    n_out = 0; n_in = 0;
    uint64_t soff = 0;
    for (int s = 0; s < world; s++) {
      n_out += count(me, s); n_in += count(s, me);
      send_off[s] = soff;
      soff += (uint64_t)count(me, s);
      for (int r = 1; r < world; r++) ahead[(size_t)r * world + s] = ahead[(size_t)(r - 1) * world + s] + (uint64_t)count(r - 1, s);
    }
  }
  // every rank sees every inbox: the first destination whose arrivals exceed its room (dest < 0: none), the same on every rank
  struct Overflow { int dest = -1; int64_t arriving = 0; uint32_t room = 0; };
  Overflow admission() const {
    Overflow o;
    for (int s = 0; s < world; s++) {
      int64_t arriving = 0;
      for (int r = 0; r < world; r++) arriving += count(r, s);
      if (arriving > (int64_t)room[s]) { o.dest = s; o.arriving = arriving; o.room = room[s]; return o; }
    }
    return o;
  }
};

// ------------------------------------------------------------------------------------------------ after a migration
// slack of a freshly cut clip box around the particles: the room the look-ahead test asks for (2 margin + 3) and as much again, so
// that a re-plan is not followed by the next one a migration later
inline int clip_slack(int margin) { return std::max(8, 4 * margin + 4); }

// The occupancy boxes: do they still hold every node the particles can touch before the next check?
// A particle with base cell b touches the nodes b .. b + 2; the table carries every rank's base-cell bounds (M.rank_bounds; M.lo / M.hi
// bound ALL ranks' live particles), taken BEFORE this migration's records moved: a rank's particles after it lie inside its own
// bounds joined with those of every rank that sent it records.
struct After {
  enum Kind { KEEP, REPLAN, LEFT } kind = KEEP;
  int rank = -1, axis = -1, cells[2] = {0, 0}, nodes[2] = {0, 0};  // LEFT: who left what (base cells [c0, c1), boxes cut to nodes [n0, n1))
  int clip_lo[3] = {0, 0, 0}, clip_hi[3] = {0, 0, 0};              // REPLAN: the fresh clip box ...
  std::vector<int> occ;                                            // ... and occupancy boxes [world][6]
};
// occ: the occupancy boxes in force, or nullptr while there are none (only the clip box, which then stands in for every rank's box)
inline After after_migration(const Mig &M, const int clip_lo[3], const int clip_hi[3], const int *occ, const Partition &part) {
  After A;
  if (!(M.lo[0] <= M.hi[0] && M.lo[1] <= M.hi[1] && M.lo[2] <= M.hi[2])) return A;  // (no particle anywhere)
  const int world = M.world;
  const int *res = part.res;
  // (a) Looking back: the halo boxes of the substeps since the last check were cut to these boxes, so mass splatted outside a rank's
  //     box was never exchanged.  The schedule lets the particles travel margin cells between two checks if their top speed
  //     at most doubles, and (b) keeps 2 margin + 1 cells of room, but a particle deep inside a brick that speeds up further
  //     (it trips no margin test: error bit 2 only watches the brick's own faces) could have left the box unseen: that is an
  //     error here, not a silent loss.
  for (int r = 0; r < world; r++) {
    const int *rb = &M.rank_bounds[(size_t)r * 6];
    if (!nonempty(rb)) continue;
    for (int a = 0; a < 3; a++) {
      const int olo = occ ? occ[(size_t)r * 6 + a] : clip_lo[a], ohi = occ ? occ[(size_t)r * 6 + 3 + a] : clip_hi[a];
      // (a side where the box ends at the grid itself holds everything there is: with clean_boundary off, or on the clamped generic
      // path, base cells reach res - 1, and no halo mass can lie beyond the last node)
      if (rb[a] < olo || (rb[3 + a] + 2 > ohi && ohi != res[a] + 1)) {
        A.kind = After::LEFT; A.rank = r; A.axis = a;
        A.cells[0] = rb[a]; A.cells[1] = rb[3 + a]; A.nodes[0] = olo; A.nodes[1] = ohi;
        return A;
      }
    }
  }
  // every rank's bounds once this migration's records have arrived
  std::vector<int> post(M.rank_bounds);
  for (int r = 0; r < world; r++)
    for (int s = 0; s < world; s++) {
      if (s == r || M.count(s, r) == 0) continue;
      const int *sb = &M.rank_bounds[(size_t)s * 6];
      for (int a = 0; a < 3; a++) {
        post[(size_t)r * 6 + a] = std::min(post[(size_t)r * 6 + a], sb[a]);
        post[(size_t)r * 6 + 3 + a] = std::max(post[(size_t)r * 6 + 3 + a], sb[3 + a]);
      }
    }
  // (b) Looking ahead: room for a travel of 2 margin cells on every side (the schedule plans for margin)
  bool covers = occ != nullptr;
  const int room = 2 * part.margin;
  for (int r = 0; r < world && covers; r++) {
    const int *pb = &post[(size_t)r * 6];
    if (!nonempty(pb)) continue;
    for (int a = 0; a < 3; a++) {
      const int olo = occ[(size_t)r * 6 + a], ohi = occ[(size_t)r * 6 + 3 + a];
      covers = covers && (pb[a] - room - 1 >= olo || olo == 0);
      covers = covers && (pb[3 + a] + room + 3 <= ohi || ohi == res[a] + 1);
    }
  }
  // fresh boxes: the bounds with clip_slack cells around them (a rank without particles: an empty box — it neither sends nor gathers)
  const int s = clip_slack(part.margin);
  A.occ.assign((size_t)world * 6, 0);
  for (int a = 0; a < 3; a++) { A.clip_lo[a] = std::max(0, M.lo[a] - s); A.clip_hi[a] = std::min(res[a] + 1, M.hi[a] + s + 2); }
  for (int r = 0; r < world; r++) {
    const int *pb = &post[(size_t)r * 6];
    if (!nonempty(pb)) continue;
    for (int a = 0; a < 3; a++) {
      A.occ[(size_t)r * 6 + a] = std::max(0, pb[a] - s);
      A.occ[(size_t)r * 6 + 3 + a] = std::min(res[a] + 1, pb[3 + a] + s + 2);
    }
  }
  // ... and a re-plan also when the boxes in use have become much too wide (clusters that have drifted apart; the first check of a
  // job, whose boxes are the global clip box of the set-up): all ranks' plans together, which every rank computes alike
  bool shrink = false;
  if (covers) {
    uint64_t now = 0, then = 0;
    for (int r = 0; r < world; r++) {
      now += plan(part, clip_lo, clip_hi, occ, r).total;
      then += plan(part, A.clip_lo, A.clip_hi, A.occ.data(), r).total;
    }
    shrink = 2 * then < now;
  }
  if (!covers || shrink) A.kind = After::REPLAN;
  return A;
}

// ------------------------------------------------------------------------------------------------ re-cutting a running job
// Cell cut planes [0, c1, .., res] along one axis so that every part holds about the same number of particles — tiled.balanced_cuts
// restated exactly: the cut lies behind the first cell whose cumulative count reaches total k / parts (compared as integers: cum parts
// >= total k); a cut at the lower edge of an EMPTY stretch moves to its middle (clusters that do not touch: along the face of the
// lower cluster every particle that moves up a cell would cross); every part keeps at least one cell; an empty histogram gives the
// even split.  Needs 1 <= parts <= res; cuts_out holds parts + 1 entries.
inline void balanced_cuts(int res, int parts, const int64_t *hist, int *cuts_out) {
  int64_t total = 0;
  for (int i = 0; i < res; i++) total += hist[i];
  cuts_out[0] = 0;
  int i = 0;
  int64_t cum = hist[0];  // counts of the cells 0 .. i
  for (int k = 1; k < parts; k++) {
    int c;
    if (total == 0) {
      c = (int)((int64_t)res * k / parts);
    } else {
      while (cum * parts < total * k) cum += hist[++i];  // (ends: the last cell's cumulative count is the total)
      c = i + 1;
      if (c < res && hist[c] == 0) {
        int nz = c;
        while (nz < res && hist[nz] == 0) nz++;
        if (nz < res) c += (nz - c) / 2;
      }
    }
    c = std::max(c, cuts_out[k - 1] + 1);
    c = std::min(c, res - (parts - k));
    cuts_out[k] = c;
  }
  cuts_out[parts] = res;
}

// The round rule of a redistribution (mpmhip_tiled_redistribute): a re-cut may send a destination far more records than its inbox
// holds, so the records travel in rounds.  left[src * world + dst] = records src still holds for dst (the table every rank reads),
// room[dst] = what dst's inbox takes this round: destination dst admits its sources in ascending rank order until the inbox is full,
// and a source never sends more than it has.  Every rank computes the same quotas from the same table, as Mig::admission is computed
// from it.  While room[dst] >= 1, a round moves at least one record for every destination that still expects some: the rounds end.
// Returns the records the round moves in the whole job.
inline int64_t round_quotas(int world, const int64_t *left, const uint32_t *room, int64_t *q) {
  int64_t moved = 0;
  for (int dst = 0; dst < world; dst++) {
    int64_t free_ = (int64_t)room[dst];
    for (int src = 0; src < world; src++) {
      const int64_t n = src == dst ? 0 : std::min(left[(size_t)src * world + dst], free_);
      q[(size_t)src * world + dst] = n;
      free_ -= n;
      moved += n;
    }
  }
  return moved;
}
// the rounds the rule needs for a table while every inbox offers the same room in every round (-1: a destination without room expects records)
inline int64_t rounds_needed(int world, const int64_t *counts, const uint32_t *room) {
  std::vector<int64_t> left(counts, counts + (size_t)world * world), q((size_t)world * world);
  for (int r = 0; r < world; r++) left[(size_t)r * world + r] = 0;
  int64_t rounds = 0;
  for (;;) {
    int64_t todo = 0;
    for (int64_t v : left) todo += v;
    if (todo == 0) return rounds;
    if (round_quotas(world, left.data(), room, q.data()) == 0) return -1;
    for (size_t i = 0; i < left.size(); i++) left[i] -= q[i];
    rounds++;
  }
}
// The capacity rule: from the same table every rank knows every rank's live count after the move, live - out + in.  The first rank
// that exceeds its capacity, its count after the move and by how much it exceeds (rank < 0: all fit).
struct Growth { int rank = -1; int64_t need = 0, excess = 0; };
inline int64_t live_after(int world, const int64_t *counts, const int64_t *live, int r) {
  int64_t n = live[r];
  for (int s = 0; s < world; s++)
    if (s != r) n += counts[(size_t)s * world + r] - counts[(size_t)r * world + s];
  return n;
}
inline Growth capacity_check(int world, const int64_t *counts, const int64_t *live, const int64_t *cap) {
  Growth g;
  for (int r = 0; r < world; r++) {
    const int64_t n = live_after(world, counts, live, r);
    if (n > cap[r]) { g.rank = r; g.need = n; g.excess = n - cap[r]; return g; }
  }
  return g;
}
// The table of a redistribution's scan carries two words more than a migration's, in places a migration leaves idle: the diagonal
// counts[r][r] = rank r's live records, and the speed word = its capacity.  Takes them out of the [world][ROW] words (h is changed:
// what is left decodes as a migration table without a speed).
inline void split_recut_table(uint32_t *h, int world, int64_t *live, int64_t *cap) {
  for (int r = 0; r < world; r++) {
    uint32_t *row = h + (size_t)r * ROW;
    live[r] = row[r]; cap[r] = row[world + 6];
    row[r] = 0; row[world + 6] = 0;
  }
}

// ------------------------------------------------------------------------------------------------ schedule
// substeps until the next migration: after one every particle is inside its brick and needs margin / speed substeps to cross the
// margin; half of that leaves room for the speed to double in between; never sooner than the CFL schedule (migrate_interval),
// never later than the cap
inline int64_t next_interval(int migrate_interval, int adaptive_cap, int margin, float speed) {
  int64_t n = migrate_interval;
  if (adaptive_cap > n && std::isfinite(speed))
    n = std::max<int64_t>(n, std::min<int64_t>(adaptive_cap, (int64_t)(0.5 * margin / std::max(speed, 1e-9f))));
  return n;
}

}  // namespace tplan
