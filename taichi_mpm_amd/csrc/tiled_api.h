// taichi_mpm_amd/csrc/tiled_api.h — the native data plane of a tiled (multi-GPU) run: plan, buffers, wires, migration
// and the per-substep loop (include/mpmhip.h: "Multi-GPU tiling, the native data plane").  Host code of libmpmhip,
// included by mpmhip.hip.  The reference has no multi-process code (dead `#ifdef TC_USE_MPI`, src/mpm.cpp:6-8): the contract
// is SURVEY section 8(e) — bricks, halo sum after P2G, particle migration after G2P, a few scalars per migration.
//
// Every decision that is host arithmetic — plan, interior, arena layout, migration table, re-plan rules, schedule — is tiled_plan.h's
// (namespace tplan, tested on the host); the functions here ask it and then do the device work.
//
//   plan      box(R, S) = node_box(R) ∩ node_box(S), node_box(R) = [brick.lo - margin, brick.hi + margin + 2) clipped to the
//             occupied part of the grid AND to rank R's own occupancy box (the nodes R's particles can touch before the next
//             migration check: every rank's particle bounds travel in the migration table, so all ranks hold all boxes) — R has
//             no mass outside it to send and nothing outside it to gather, so clusters that do not meet exchange nothing
//             (configs[4]: 8 - 39 MB per rank and substep of empty slabs around the cuts before round 6).
//   arena     ONE device allocation per rank: flag words, two migration tables, two receive buffers (parity of the substep),
//             the migration inbox.
//   epochs    substep e: the writer stores into recv[e & 1] of the reader and then publishes e in the reader's word
//             flag[writer]; the reader waits for flag >= e before reading.  Two buffers suffice: a writer reaches substep
//             e + 2 only after it has seen the reader's epoch e + 1, which the reader publishes after its reads of substep e.
//             Migrations carry their own epoch m (tables alternate by m & 1; records wait for the whole table of m, which
//             every rank contributes to only after its import of m - 1).
//   bodies    a job with CPIC rigid bodies: every rank holds all bodies; the ranks' impulse rows travel twice a substep and are added
//             in rank order (the section "impulse rows" below; layout in tiled_plan.h, kernels in k_rigid_rows.h).
#pragma once
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl is dlopen'ed, libmpmhip does not link it

namespace {

struct RcclApi {
  void *handle = nullptr;
  std::string error;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclCommAbort) CommAbort = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
};

RcclApi *rccl_api() {
  static RcclApi api;
  static bool tried = false;
  if (tried) return &api;
  tried = true;
  const char *names[] = {getenv("MPMHIP_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  for (const char *n : names) {
    if (!n || !*n) continue;
    api.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (api.handle) break;
    api.error = dlerror();
  }
  if (!api.handle) return &api;
  bool ok = true;
  auto sym = [&](const char *name) { void *p = dlsym(api.handle, name); if (!p) { ok = false; api.error = std::string("missing symbol ") + name; } return p; };
  api.GetUniqueId = (decltype(api.GetUniqueId))sym("ncclGetUniqueId");
  api.CommInitRank = (decltype(api.CommInitRank))sym("ncclCommInitRank");
  api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
  api.CommAbort = (decltype(api.CommAbort))sym("ncclCommAbort");
  api.Send = (decltype(api.Send))sym("ncclSend");
  api.Recv = (decltype(api.Recv))sym("ncclRecv");
  api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
  api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
  api.AllGather = (decltype(api.AllGather))sym("ncclAllGather");
  api.AllReduce = (decltype(api.AllReduce))sym("ncclAllReduce");
  api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
  if (!ok) { dlclose(api.handle); api.handle = nullptr; }
  return &api;
}

#define NCCLCHK(c, call)                                                                                   \
  do {                                                                                                     \
    ncclResult_t r_ = (call);                                                                              \
    if (r_ != ncclSuccess) return fail((c), MPMHIP_EHIP, "%s failed: %s", #call, rccl_api()->GetErrorString(r_)); \
  } while (0)

static_assert(sizeof(float4) == tplan::NODE_BYTES, "a halo node travels as one float4");
// a rank's arena as a process addresses it (its own allocation, or a peer's mapped one): every rank lays its arena out alike
void tn_carve(mpmhip_ctx::TiledNative::Peer &P, char *base, const tplan::Arena &A) {
  P.flags = reinterpret_cast<uint32_t *>(base + A.flags);
  for (int k = 0; k < 2; k++) {
    P.red[k] = reinterpret_cast<double *>(base + A.red[k]);
    P.table[k] = reinterpret_cast<uint32_t *>(base + A.table[k]);
    P.recv[k] = reinterpret_cast<float4 *>(base + A.recv[k]);
  }
  P.inbox = reinterpret_cast<float4 *>(base + A.inbox);
}
// the partition as the planner reads it (c->T carries what the kernels need of it)
tplan::Partition tn_part(const mpmhip_ctx *c) {
  tplan::Partition part;
  static_assert(sizeof part.cuts == sizeof c->T.cuts && sizeof part.dims == sizeof c->T.dims, "Tiling and tplan::Partition hold the same cuts");
  memcpy(part.dims, c->T.dims, sizeof part.dims);
  memcpy(part.cuts, c->T.cuts, sizeof part.cuts);
  memcpy(part.res, c->P.res, sizeof part.res);
  part.margin = c->T.margin;
  return part;
}
const int *tn_occ(const mpmhip_ctx::TiledNative &N) { return N.occ_valid ? N.occ.data() : nullptr; }
bool tn_peer_wire(const mpmhip_ctx::TiledNative &N) { return tplan::peer_wire(N.wire, N.loop_rccl); }

int tn_wait(mpmhip_ctx *c, const uint32_t *words, const std::vector<int> &who, int *d_idx, uint32_t epoch) {
  if (who.empty()) return MPMHIP_OK;
  hipLaunchKernelGGL(k_epoch_wait, dim3(1), dim3(64), 0, c->stream, words, (const int *)d_idx, (int)who.size(), epoch,
                     c->tn.timeout_ticks, c->cnt);
  return launch_check(c, "epoch_wait");
}

// (re)build this rank's plan for the current clip box and occupancy and upload the device box tables; no allocation
int tn_apply_plan(mpmhip_ctx *c) {
  auto &N = c->tn;
  Tiling &T = c->T;
  const tplan::Partition part = tn_part(c);
  N.plan = tplan::plan(part, N.clip_lo, N.clip_hi, tn_occ(N), T.rank);
  // (a job with bodies keeps its impulse rows behind the nodes of the receive buffers: the boxes are held against what is left)
  const uint64_t node_cap = tplan::rows_node_cap(N.lay.halo_cap, N.world, N.rows);
  const tplan::PlanFault f = tplan::link(N.plan, part, N.clip_lo, N.clip_hi, tn_occ(N), T.rank, node_cap);
  const size_t n = N.plan.boxes.size();
  if (f.kind == tplan::PlanFault::TOO_MANY_BOXES) return fail(c, MPMHIP_EINVAL, "too many halo boxes (%zu)", n);
  if (f.kind == tplan::PlanFault::EXCEEDS_ARENA) return fail(c, MPMHIP_ECAPACITY, "internal: halo plan of %llu nodes exceeds the arena (%llu)", (unsigned long long)N.plan.total, (unsigned long long)node_cap);
  if (f.kind == tplan::PlanFault::NO_COUNTERPART) return fail(c, MPMHIP_EINVAL, "internal: halo box towards rank %d has no counterpart", f.peer);
  // the overlap-free interior of this rank's node box — the node box as the boxes were cut from it (tiled_plan.h: interior_of;
  // until round 6 the uncut brick box stood here, and at configs[3] over 8 bricks every block was boundary work) — and the device tables
  HIPCHK(c, hipStreamSynchronize(c->stream));
  T.n_boxes = 0; T.box_nodes = 0; T.box_blocks = 0;
  const tplan::Interior I = tplan::interior_of(part, N.clip_lo, N.clip_hi, tn_occ(N), T.rank, N.plan);
  for (int a = 0; a < 3; a++) { T.int_lo[a] = I.lo[a]; T.int_hi[a] = I.hi[a]; }
  const bool peer_wire = tn_peer_wire(N);
  std::vector<DevBox> hb[2] = {std::vector<DevBox>(n), std::vector<DevBox>(n)};
  std::vector<int> idx(n);
  for (size_t i = 0; i < n; i++) {
    const auto &b = N.plan.boxes[i];
    for (int par = 0; par < 2; par++) {
      DevBox &d = hb[par][i];
      for (int a = 0; a < 3; a++) { d.lo[a] = b.lo[a]; d.dim[a] = b.hi[a] - b.lo[a]; }
      d.peer = b.peer; d.off = (uint32_t)b.off; d.boff = I.boff[i];
      if (peer_wire) {
        const auto &P = N.peers[b.peer];
        d.send = P.recv[par] ? P.recv[par] + b.peer_off : nullptr;  // (nullptr until the peers are connected)
        d.recv = N.recv[par] + b.off;
        d.flag = P.flags ? P.flags + T.rank : nullptr;
      } else {
        d.send = N.send + b.off;
        d.recv = N.recv[0] + b.off;
        d.flag = nullptr;
      }
    }
    idx[i] = b.peer;
  }
  if (n) {
    for (int par = 0; par < 2; par++) HIPCHK(c, hipMemcpy(N.d_boxes[par], hb[par].data(), sizeof(DevBox) * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(N.d_halo_idx, idx.data(), sizeof(int) * n, hipMemcpyHostToDevice));
  }
  N.halo_peers = idx;
  T.n_boxes = (int)n; T.box_nodes = (uint32_t)N.plan.total; T.box_blocks = I.box_blocks;
  c->d_boxes_cur = N.d_boxes[peer_wire ? (N.epoch & 1) : 0];
  return MPMHIP_OK;
}

bool tn_connected(const mpmhip_ctx *c) {
  const auto &N = c->tn;
  if (N.wire == MPMHIP_WIRE_RCCL) return N.comm != nullptr;
  return N.connected;
}

// ------------------------------------------------------------------------------------------------ the halo exchange
// begin: which box table the pack / grid kernels of this substep use (parity of the epoch) — called by mpmhip_substep_begin
void tn_begin_substep(mpmhip_ctx *c) {
  auto &N = c->tn;
  N.epoch++;
  c->d_boxes_cur = N.d_boxes[tn_peer_wire(N) ? (N.epoch & 1) : 0];
}

int tn_exchange_start(mpmhip_ctx *c) {
  auto &N = c->tn;
  if (N.plan.boxes.empty()) return MPMHIP_OK;
  if (N.wire != MPMHIP_WIRE_RCCL && !N.loop_rccl) {  // peer wires: k_halo_pack wrote the boxes into the peers' buffers; publish the epoch
    N.wait_merged = N.wire == MPMHIP_WIRE_IPC && !c->ov_active;
    if (N.wait_merged) {  // (nothing runs between signal and wait: one launch; see k_epoch_signal_wait)
      hipLaunchKernelGGL(k_epoch_signal_wait, dim3(1), dim3(64), 0, c->stream, c->d_boxes_cur, (int)N.plan.boxes.size(), (const uint32_t *)N.flags,
                         (const int *)N.d_halo_idx, (int)N.halo_peers.size(), N.epoch, N.timeout_ticks, c->cnt);
      return launch_check(c, "epoch_signal_wait");
    }
    if (N.defer_signal && !c->ov_active) {  // (mpmhip_tiled_advance_group publishes every rank's epoch with one launch)
      N.signal_deferred = true;
      return MPMHIP_OK;
    }
    hipLaunchKernelGGL(k_epoch_signal, dim3(1), dim3(64), 0, c->stream, c->d_boxes_cur, (int)N.plan.boxes.size(), N.epoch);
    return launch_check(c, "epoch_signal");
  }
  RcclApi *R = rccl_api();
  hipStream_t st = c->stream;
  if (c->ov_active) {  // the exchange runs beside the interior kernels: side stream, fenced by events
    HIPCHK(c, hipEventRecord(N.ev_a, c->stream));
    HIPCHK(c, hipStreamWaitEvent(N.side, N.ev_a, 0));
    st = N.side;
  }
  NCCLCHK(c, R->GroupStart());
  for (const auto &b : N.plan.boxes) {
    if (N.loop_rccl) {
      // one-GPU pre-flight of this very path (MPMHIP_WIRE_LOCAL_RCCL): the rank's communicator has ONE rank, every box is a send to
      // itself whose receive is aimed at the box's place in the peer ctx's receive buffer (same process: a plain pointer) — the same
      // group of RCCL kernels on the same stream behind the same fences, with the peer's recv[0] as the single receive buffer
      NCCLCHK(c, R->Send(N.send + b.off, (size_t)b.vol * 4, ncclFloat, 0, (ncclComm_t)N.comm, st));
      NCCLCHK(c, R->Recv(N.peers[b.peer].recv[0] + b.peer_off, (size_t)b.vol * 4, ncclFloat, 0, (ncclComm_t)N.comm, st));
      continue;
    }
    NCCLCHK(c, R->Send(N.send + b.off, (size_t)b.vol * 4, ncclFloat, b.peer, (ncclComm_t)N.comm, st));
    NCCLCHK(c, R->Recv(N.recv[0] + b.off, (size_t)b.vol * 4, ncclFloat, b.peer, (ncclComm_t)N.comm, st));
  }
  NCCLCHK(c, R->GroupEnd());
  if (st != c->stream) HIPCHK(c, hipEventRecord(N.ev_b, st));
  N.exch_on_side = st != c->stream;
  return MPMHIP_OK;
}

int tn_exchange_wait(mpmhip_ctx *c) {
  auto &N = c->tn;
  if (N.plan.boxes.empty()) return MPMHIP_OK;
  if (N.loop_rccl) {
    // (this rank's boxes were written by its PEERS' groups: their events; its own group read its send buffer: its own event.  The
    // ranks of a local job share one stream and advance together — begin of every rank, then the ends —, so every event has been
    // recorded for this substep when the first end waits)
    if (N.exch_on_side) HIPCHK(c, hipStreamWaitEvent(c->stream, N.ev_b, 0));
    for (int p : N.halo_peers) {
      mpmhip_ctx *q = N.local_ctx[(size_t)p];
      if (q->tn.exch_on_side) HIPCHK(c, hipStreamWaitEvent(c->stream, q->tn.ev_b, 0));
    }
    return MPMHIP_OK;
  }
  if (N.wire == MPMHIP_WIRE_RCCL) {
    if (N.exch_on_side) HIPCHK(c, hipStreamWaitEvent(c->stream, N.ev_b, 0));
    return MPMHIP_OK;
  }
  if (N.wait_merged) return MPMHIP_OK;  // (tn_exchange_start's launch has waited already)
  return tn_wait(c, N.flags, N.halo_peers, N.d_halo_idx, N.epoch);
}

// ------------------------------------------------------------------------------------------------ impulse rows (bodies on a job)
// Every rank holds all bodies; a rank's colour-aware transfer kernels collect what ITS particles hand them.  Twice a substep — exchange
// 0 behind the rigid P2G, exchange 1 behind the rigid G2P — the rank's row goes to every rank (tn_row_out) and, once the rows of all
// ranks are there, every rank adds them in rank order and applies the sum (tn_rows_apply): DESIGN section 5, "Bodies on a job".
//   peer wires   k_rigid_row_out writes the row into every rank's table (its own included) and publishes the exchange's epoch in
//                every rank's flag page; k_rigid_rows_world waits for all ranks' epochs (the bounded wait of the halo boxes)
//   RCCL         the row is staged and travels as one send / receive pair per peer (an all-reduce would add in its own order);
//                stream order is the wait.  MPMHIP_WIRE_LOCAL_RCCL: the same pairs as self-sends aimed at the peer ctx's table
//   epochs       one counter per exchange; the tables of parity (epoch & 1) live in recv[parity], behind the nodes.  A rank reaches
//                epoch e + 2 of an exchange only after it has seen every rank's epoch e + 1, published behind that rank's reads of e.
// No host synchronisation: everything is enqueued on the ctx's stream.  The ranks of a local job share the device's queues, so
// mpmhip_tiled_advance_group enqueues EVERY rank's tn_row_out of an exchange before the first tn_rows_apply of it.
float *tn_rows_at(const mpmhip_ctx::TiledNative &N, const mpmhip_ctx::TiledNative::Peer &P, int par, int exchange, int rank) {
  return reinterpret_cast<float *>(P.recv[par] + tplan::rows_off(N.lay.halo_cap, N.world, exchange, rank));
}
bool tn_rows_by_rccl(const mpmhip_ctx::TiledNative &N) { return N.wire == MPMHIP_WIRE_RCCL || N.loop_rccl; }

int tn_row_out(mpmhip_ctx *c, int x) {
  auto &N = c->tn;
  auto &R = c->rigid;
  const int me = c->T.rank, world = N.world, nb = (int)R.store.bodies.size();
  const uint32_t epoch = ++N.row_epoch[x];
  const int par = (int)(epoch & 1u);
  if (c->deterministic)  // (the rows of the flagged blocks, in k_rigid_rows_apply's fixed order, stand in for the atomics' sums)
    rows_launch_sum(c->stream, nb, c->P, (const Counters *)c->cnt, (const uint8_t *)R.d_blk_rigid, (const float *)R.d_imp_rows, R.d_rb);
  RowPut L;
  memset(&L, 0, sizeof L);
  const bool by_rccl = tn_rows_by_rccl(N);
  for (int p = 0; p < world; p++) {
    if (by_rccl && p != me) continue;  // (its own row a rank always writes itself)
    L.dst[p] = tn_rows_at(N, N.peers[p], par, x, me);
    L.flag[p] = by_rccl ? nullptr : N.peers[p].flags + tplan::rows_flag_word(x, me);
  }
  rows_launch_out(c->stream, R.d_rb, nb, L, world, by_rccl ? N.d_row_stage.get() : nullptr, epoch);
  if (int rc = launch_check(c, "rigid_row_out")) return rc;
  if (!by_rccl || world == 1) return MPMHIP_OK;
  RcclApi *A = rccl_api();
  NCCLCHK(c, A->GroupStart());
  for (int p = 0; p < world; p++) {
    if (p == me) continue;
    if (N.loop_rccl) {  // (one-rank communicator: a send to itself whose receive is aimed at the peer ctx's table — tn_exchange_start)
      NCCLCHK(c, A->Send(N.d_row_stage.get(), tplan::IMP_ROW_FLOATS, ncclFloat, 0, (ncclComm_t)N.comm, c->stream));
      NCCLCHK(c, A->Recv(tn_rows_at(N, N.peers[p], par, x, me), tplan::IMP_ROW_FLOATS, ncclFloat, 0, (ncclComm_t)N.comm, c->stream));
      continue;
    }
    NCCLCHK(c, A->Send(N.d_row_stage.get(), tplan::IMP_ROW_FLOATS, ncclFloat, p, (ncclComm_t)N.comm, c->stream));
    NCCLCHK(c, A->Recv(tn_rows_at(N, N.peers[me], par, x, p), tplan::IMP_ROW_FLOATS, ncclFloat, p, (ncclComm_t)N.comm, c->stream));
  }
  NCCLCHK(c, A->GroupEnd());
  return MPMHIP_OK;
}

int tn_rows_apply(mpmhip_ctx *c, int x) {
  auto &N = c->tn;
  auto &R = c->rigid;
  const int me = c->T.rank;
  const uint32_t epoch = N.row_epoch[x];
  // (the RCCL wires: the receives were enqueued on this stream — MPMHIP_WIRE_LOCAL_RCCL: on the ONE stream the ranks share — in front of this launch)
  const int n_wait = tn_rows_by_rccl(N) ? 0 : N.world;
  rows_launch_apply(c->stream, R.d_rb, (int)R.store.bodies.size(), tn_rows_at(N, N.peers[me], (int)(epoch & 1u), x, 0), N.world,
                    N.flags + tplan::rows_flag_word(x, 0), n_wait, epoch, N.timeout_ticks, c->cnt);
  return launch_check(c, "rigid_rows_world");
}

// ------------------------------------------------------------------------------------------------ migration
// phase A: scan (leavers per destination, bounds, top speed) and publish this rank's row of the table
// recut_room < 0: a migration.  >= 0: the scan of a redistribution round (k_recut_count: no margin check; the row also carries this
// rank's live records and its capacity, tiled_plan.h: split_recut_table) which offers recut_room records of its inbox
int tn_mig_a(mpmhip_ctx *c, int64_t recut_room = -1) {
  auto &N = c->tn;
  const int world = N.world;
  int rc = ensure_counts(c, world);
  if (rc) return rc;
  N.mig_epoch++;
  hipLaunchKernelGGL(k_scan_init, dim3((world + 8 + 255) / 256), dim3(256), 0, c->stream, c->d_counts, world,
                     (uint32_t)std::min<uint64_t>(recut_room >= 0 ? (uint64_t)recut_room : N.lay.inbox_cap, 0xFFFFFFFFull));
  int grid = particle_grid(c->n_slots);
  if (grid > 128) grid = 128;
  if (recut_room >= 0) {
    hipLaunchKernelGGL(k_recut_count, dim3(grid), dim3(256), 0, c->stream, c->P, c->T, (const float4 *)c->rg.get(), c->d_counts,
                       reinterpret_cast<int *>(c->d_counts + world));
    uint32_t *pin = c->h_pinned + 1024 + 2 * tplan::MAX_WORLD;  // (behind the cursors of a round's pack; read by the copy below, waited for in tn_recut_b)
    *pin = (uint32_t)c->cap;
    HIPCHK(c, hipMemcpyAsync(c->d_counts + world + 6, pin, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  } else {
    hipLaunchKernelGGL(k_leaver_count, dim3(grid), dim3(256), 0, c->stream, c->P, c->T, (const float4 *)c->rg.get(), (const float4 *)c->rp.get(),
                       c->d_counts, reinterpret_cast<int *>(c->d_counts + world), c->cnt);
  }
  if ((rc = launch_check(c, recut_room >= 0 ? "recut_count" : "leaver_count"))) return rc;
  uint32_t *table = N.table[N.mig_epoch & 1];
  if (N.wire == MPMHIP_WIRE_RCCL) {
    HIPCHK(c, hipMemcpyAsync(N.row, c->d_counts, sizeof(uint32_t) * (world + 8), hipMemcpyDeviceToDevice, c->stream));
    NCCLCHK(c, rccl_api()->AllGather(N.row, table, tplan::ROW, ncclUint32, (ncclComm_t)N.comm, c->stream));
    return MPMHIP_OK;
  }
  PutList L;
  memset(&L, 0, sizeof L);
  for (int p = 0; p < world; p++) {
    L.src[p] = c->d_counts;
    L.dst[p] = (p == c->T.rank ? table : N.peers[p].table[N.mig_epoch & 1]) + (size_t)c->T.rank * tplan::ROW;
    L.flag[p] = (p == c->T.rank ? N.flags : N.peers[p].flags) + tplan::MAX_WORLD + c->T.rank;
    L.words[p] = (uint32_t)world + 8;
  }
  hipLaunchKernelGGL(k_put, dim3(world, 1), dim3(256), 0, c->stream, L, N.mig_epoch, N.d_done);
  return launch_check(c, "put (migration row)");
}

int tn_send_records(mpmhip_ctx *c);
// phase B: read the table (the ONE synchronisation of a migration), pack the leavers and send them
int tn_mig_b(mpmhip_ctx *c) {
  auto &N = c->tn;
  const int world = N.world, me = c->T.rank;
  int rc;
  uint32_t *table = N.table[N.mig_epoch & 1];
  if (N.wire != MPMHIP_WIRE_RCCL && (rc = tn_wait(c, N.flags + tplan::MAX_WORLD, N.all_ranks, N.d_all_idx, N.mig_epoch))) return rc;
  uint32_t *h = c->h_pinned + 2048;  // behind the counters and the cursors of mpmhip_export_leavers
  HIPCHK(c, hipMemcpyAsync(h, table, sizeof(uint32_t) * tplan::ROW * world, hipMemcpyDeviceToHost, c->stream));
  Counters hc;
  if ((rc = read_counters(c, hc))) return rc;  // synchronises; reports a margin violation or a wait that timed out
  auto &M = N.mig;
  M.decode(h, world, me);
  if (M.total == 0) return MPMHIP_OK;
  // records: grouped by destination in mig_send (k_leaver_pack), then one message per destination
  if ((size_t)M.n_out > N.mig_send_cap) {
    N.mig_send_cap = (size_t)M.n_out + (size_t)M.n_out / 2 + 4096;
    HIPCHK(c, N.mig_send.alloc(N.mig_send_cap * tplan::MIG_FLOAT4));
  }
  const auto over = M.admission();  // every rank sees every inbox: all refuse together, BEFORE anybody writes beyond one
  if (over.dest >= 0)
    return fail(c, MPMHIP_ECAPACITY, "migration: %lld particles arriving at rank %d exceed its inbox of %u records (mpmhip_tiled_config.inbox_records)",
                (long long)over.arriving, over.dest, over.room);
  if (M.n_out && (rc = mpmhip_export_leavers(c, world, &M.counts[(size_t)me * world], N.mig_send))) return rc;
  N.migrated_out += M.n_out;
  return tn_send_records(c);
}

// the records packed into mig_send on their way, one message per destination, as the decoded table N.mig says: this rank's records
// for s begin at send_off[s]; in the inbox of s they lie behind those of the ranks below this one (ahead)
int tn_send_records(mpmhip_ctx *c) {
  auto &N = c->tn;
  auto &M = N.mig;
  const int world = N.world, me = c->T.rank;
  if (N.wire == MPMHIP_WIRE_RCCL) {
    RcclApi *R = rccl_api();
    NCCLCHK(c, R->GroupStart());
    for (int s = 0; s < world; s++) {
      const int64_t ns = M.count(me, s), nr = M.count(s, me);
      if (s != me && ns) NCCLCHK(c, R->Send(N.mig_send + M.send_off[s] * tplan::MIG_FLOAT4, (size_t)ns * MPMHIP_MIGRATE_FLOATS, ncclFloat, s, (ncclComm_t)N.comm, c->stream));
      if (s != me && nr) NCCLCHK(c, R->Recv(N.inbox + M.ahead[(size_t)s * world + me] * tplan::MIG_FLOAT4, (size_t)nr * MPMHIP_MIGRATE_FLOATS, ncclFloat, s, (ncclComm_t)N.comm, c->stream));
    }
    NCCLCHK(c, R->GroupEnd());
    return MPMHIP_OK;
  }
  PutList L;
  memset(&L, 0, sizeof L);
  uint32_t most = 0;
  for (int s = 0; s < world; s++) {
    L.src[s] = s == me ? nullptr : reinterpret_cast<const uint32_t *>(N.mig_send + M.send_off[s] * tplan::MIG_FLOAT4);
    L.dst[s] = s == me ? nullptr : reinterpret_cast<uint32_t *>(N.peers[s].inbox + M.ahead[(size_t)me * world + s] * tplan::MIG_FLOAT4);
    L.words[s] = s == me ? 0u : (uint32_t)(M.count(me, s) * MPMHIP_MIGRATE_FLOATS);
    L.flag[s] = (s == me ? N.flags : N.peers[s].flags) + 2 * tplan::MAX_WORLD + me;
    most = std::max(most, L.words[s]);
  }
  const int chunks = (int)std::min<uint32_t>(64u, std::max<uint32_t>(1u, most / (256 * 16)));
  hipLaunchKernelGGL(k_put, dim3(world, chunks), dim3(256), 0, c->stream, L, N.mig_epoch, N.d_done);
  return launch_check(c, "put (migration records)");
}

// phase C: import the arrivals, keep the halo boxes wrapped around the particles, schedule the next migration
int tn_mig_c(mpmhip_ctx *c) {
  auto &N = c->tn;
  auto &M = N.mig;
  int rc;
  if (M.total > 0) {
    if (N.wire != MPMHIP_WIRE_RCCL && (rc = tn_wait(c, N.flags + 2 * tplan::MAX_WORLD, N.all_ranks, N.d_all_idx, N.mig_epoch))) return rc;
    if (M.n_in && (rc = mpmhip_import_particles(c, M.n_in, N.inbox))) return rc;
    if (c->n_slots > (int64_t)(0.85 * (double)c->cap)) c->compact_requested = true;  // dead slots (leavers) pile up
  }
  if (!N.initial_scan) N.migrations++;
  // do the occupancy boxes still hold the particles, will they until the next check, are they much too wide? (tiled_plan.h)
  tplan::After A = tplan::after_migration(M, N.clip_lo, N.clip_hi, tn_occ(N), tn_part(c));
  if (A.kind == tplan::After::LEFT)
    return fail(c, MPMHIP_ECAPACITY, "tiled run: particles of rank %d left the clipped halo region on axis %d between two migrations (base cells "
                "[%d, %d), halo boxes cut to nodes [%d, %d)): their top speed more than doubled since the last check — halo sums "
                "of the substeps in between may be incomplete; lower mpmhip_tiled_config.migrate_cap or set migrate_interval",
                A.rank, A.axis, A.cells[0], A.cells[1], A.nodes[0], A.nodes[1]);
  if (A.kind == tplan::After::REPLAN) {
    for (int a = 0; a < 3; a++) { N.clip_lo[a] = A.clip_lo[a]; N.clip_hi[a] = A.clip_hi[a]; }
    N.occ.swap(A.occ);
    N.occ_valid = true;
    if ((rc = tn_apply_plan(c))) return rc;
    N.replans++;
  }
  if (N.initial_scan) return MPMHIP_OK;  // (the scan in front of a job's first substep plans, it does not move the schedule)
  N.next_migration = N.k + tplan::next_interval(N.migrate_interval, N.adaptive_cap, c->T.margin, M.speed);
  return MPMHIP_OK;
}

// ------------------------------------------------------------------------------------------------ redistribution (after a re-cut)
// mpmhip_tiled_redistribute: every live particle to the rank that owns its base cell under the partition in force, with the
// migration's machinery — scan, table, pack, the wire's record transfer, import — in ROUNDS (tiled_plan.h: round_quotas), so that
// the inbox the job was set up with is enough; no margin check (k_recut_count); the capacity rule (capacity_check) before anything
// moves.  A round is the three phases of a migration; the ranks of a local job run each phase rank by rank.
struct RecutRun {
  int64_t sent = 0, received = 0, rounds = 0, need = 0;  // info[4] of the call
  int64_t moving = 0;   // records the round in flight moves in the whole job (0: the scan found no leaver, or the call was refused)
  int refused = 0;      // MPMHIP_ECAPACITY: every rank returns it together
  bool any = false;     // joint bounds of all live particles, from the first round's table
  int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
};
// phase A of a round: make room (compact when the slots behind the live records do not hold an inbox), offer it, scan
int tn_recut_a(mpmhip_ctx *c) {
  auto &N = c->tn;
  int rc;
  if (c->rec.sorted() && (rc = invalidate_keys(c))) return rc;  // (k_import appends behind records that are not mid-substep)
  const int64_t inbox = (int64_t)std::min<uint64_t>(N.lay.inbox_cap, 0x7fffffffull);
  if (c->n_slots > 0 && c->n_slots + inbox > c->cap) {  // leavers of earlier rounds (and deleted particles) left dead slots: drop them
    c->compact_requested = true;
    if ((rc = do_sort(c)) || (rc = invalidate_keys(c))) return rc;
  }
  return tn_mig_a(c, std::max<int64_t>(0, std::min<int64_t>(inbox, c->cap - c->n_slots)));
}
// phase B: the table, the capacity rule (first round), this round's quotas, pack and send
int tn_recut_b(mpmhip_ctx *c, RecutRun &R) {
  auto &N = c->tn;
  const int world = N.world, me = c->T.rank;
  int rc;
  R.moving = 0;
  uint32_t *table = N.table[N.mig_epoch & 1];
  if (N.wire != MPMHIP_WIRE_RCCL && (rc = tn_wait(c, N.flags + tplan::MAX_WORLD, N.all_ranks, N.d_all_idx, N.mig_epoch))) return rc;
  uint32_t *h = c->h_pinned + 2048;
  HIPCHK(c, hipMemcpyAsync(h, table, sizeof(uint32_t) * tplan::ROW * world, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  uint32_t err = 0;  // (only a wait that timed out ends the call: the error word is otherwise left as it is)
  HIPCHK(c, hipMemcpy(&err, &c->cnt->error, sizeof err, hipMemcpyDeviceToHost));
  if (err & 16u) { Counters hc; return read_counters(c, hc); }
  std::vector<int64_t> live((size_t)world), cap((size_t)world);
  tplan::split_recut_table(h, world, live.data(), cap.data());
  auto &M = N.mig;
  M.decode(h, world, me);
  if (R.rounds == 0 && !R.any && M.lo[0] <= M.hi[0]) {  // (no particle anywhere: lo > hi)
    R.any = true;
    for (int a = 0; a < 3; a++) { R.lo[a] = M.lo[a]; R.hi[a] = M.hi[a]; }
  }
  if (M.total == 0) return MPMHIP_OK;
  if (R.rounds == 0) {
    const tplan::Growth g = tplan::capacity_check(world, M.counts.data(), live.data(), cap.data());
    if (g.rank >= 0) {
      const int64_t mine = tplan::live_after(world, M.counts.data(), live.data(), me);
      R.need = mine > cap[(size_t)me] ? mine : 0;
      R.refused = MPMHIP_ECAPACITY;
      return fail(c, MPMHIP_ECAPACITY, "redistribute: rank %d holds %lld particles after the move, %lld more than its capacity of %lld (mpmhip_reserve "
                  "on the ranks whose info[3] is set, then repeat the call on every rank); nothing has moved", g.rank, (long long)g.need,
                  (long long)g.excess, (long long)cap[(size_t)g.rank]);
    }
  }
  std::vector<int64_t> q((size_t)world * world);
  R.moving = tplan::round_quotas(world, M.counts.data(), M.room.data(), q.data());
  if (R.moving == 0)
    return fail(c, MPMHIP_ECAPACITY, "redistribute: %lld particles are left to move and no rank that expects some has a free slot (mpmhip_reserve)",
                (long long)M.total);
  // the round's own table: the quotas in the place of the counts (send offsets, places in the inboxes, n_in / n_out follow)
  for (int r = 0; r < world; r++)
    for (int s = 0; s < world; s++) h[(size_t)r * tplan::ROW + s] = (uint32_t)q[(size_t)r * world + s];
  M.decode(h, world, me);
  if ((size_t)M.n_out > N.mig_send_cap) {
    N.mig_send_cap = (size_t)M.n_out + (size_t)M.n_out / 2 + 4096;
    HIPCHK(c, N.mig_send.alloc(N.mig_send_cap * tplan::MIG_FLOAT4));
  }
  if (M.n_out) {
    if (!N.d_recut) HIPCHK(c, N.d_recut.alloc((size_t)2 * tplan::MAX_WORLD));
    uint32_t *pin = c->h_pinned + 1024;  // (read by the copy below; the next write comes behind the next round's synchronisation)
    for (int s = 0; s < world; s++) { pin[s] = (uint32_t)M.send_off[s]; pin[world + s] = (uint32_t)(M.send_off[s] + (uint64_t)M.count(me, s)); }
    HIPCHK(c, hipMemcpyAsync(N.d_recut, pin, sizeof(uint32_t) * 2 * world, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_recut_pack, dim3(particle_grid(c->n_slots)), dim3(256), 0, c->stream, c->P, c->T, world, (float4 *)c->rg.get(),
                       (const float4 *)c->rp.get(), (const float4 *)c->rb.get(), c->key, N.d_recut.get(), (float4 *)N.mig_send.get(), c->cnt);
    if ((rc = launch_check(c, "recut_pack"))) return rc;
  }
  R.sent += M.n_out;
  return tn_send_records(c);
}
// phase C: import the round's arrivals
int tn_recut_c(mpmhip_ctx *c, RecutRun &R) {
  auto &N = c->tn;
  auto &M = N.mig;
  int rc;
  if (R.moving == 0) return MPMHIP_OK;
  if (N.wire != MPMHIP_WIRE_RCCL && (rc = tn_wait(c, N.flags + 2 * tplan::MAX_WORLD, N.all_ranks, N.d_all_idx, N.mig_epoch))) return rc;
  if (M.n_in && (rc = mpmhip_import_particles(c, M.n_in, N.inbox))) return rc;
  R.received += M.n_in;
  R.rounds++;
  return MPMHIP_OK;
}
// behind the last round: the plan goes stale as behind a brick seeding call (seed_api.h: appended_to_job) — the next advance begins
// with the planning scan — and until then the clip box holds every node a particle of the job can touch
int tn_recut_done(mpmhip_ctx *c, const RecutRun &R) {
  auto &N = c->tn;
  if (R.any) {
    const int s = tplan::clip_slack(c->T.margin);
    for (int a = 0; a < 3; a++) {
      N.clip_lo[a] = std::max(0, std::min(N.clip_lo[a], R.lo[a] - s));
      N.clip_hi[a] = std::min(c->P.res[a] + 1, std::max(N.clip_hi[a], R.hi[a] + s + 2));
    }
  }
  N.occ_valid = false;
  if (c->n_slots > (int64_t)(0.85 * (double)c->cap)) c->compact_requested = true;  // (as tn_mig_c: the leavers' slots)
  return tn_apply_plan(c);  // (synchronises)
}
int tn_redistribute(mpmhip_ctx *const *ctxs, int n_ctx, int64_t *info) {
  std::vector<RecutRun> runs((size_t)n_ctx);
  int rc = MPMHIP_OK;
  auto report = [&]() {
    for (int r = 0; r < n_ctx && info; r++) {
      const RecutRun &R = runs[(size_t)r];
      info[4 * r] = R.sent; info[4 * r + 1] = R.received; info[4 * r + 2] = R.rounds; info[4 * r + 3] = R.need;
    }
  };
  for (;;) {
    for (int ph = 0; ph < 3; ph++)
      for (int r = 0; r < n_ctx; r++) {
        mpmhip_ctx *c = ctxs[r];
        HIPCHK(c, hipSetDevice(c->device));
        const int e = ph == 0 ? tn_recut_a(c) : (ph == 1 ? tn_recut_b(c, runs[(size_t)r]) : tn_recut_c(c, runs[(size_t)r]));
        // (the capacity rule refuses on EVERY rank, each with its own need: the phase goes on over the ranks of a local job)
        if (e && !(e == MPMHIP_ECAPACITY && runs[(size_t)r].refused)) { report(); return e; }
        if (e) rc = e;
      }
    if (rc || runs[0].moving == 0) break;
  }
  report();
  if (rc) return rc;
  for (int r = 0; r < n_ctx; r++)
    if ((rc = tn_recut_done(ctxs[r], runs[(size_t)r]))) return rc;
  return MPMHIP_OK;
}

// ------------------------------------------------------------------------------------------------ reductions
// SURVEY section 8(e) collective (3): a few scalars over all ranks (energy, live particles, the sticky error word).
//   RCCL       ncclAllReduce on a device row, read back
//   peer wires every rank writes its row into every rank's table (k_put: the writer of the last row piece publishes the
//              reduction's epoch), waits for the world's epochs, reads the table back and reduces it in RANK ORDER on the host —
//              every rank gets the bit-identical result.  Tables alternate by the parity of the reduction: a rank reaches
//              reduction r + 2 only after it has read the table of r + 1, which every rank fills after its read of r.
// put: this rank's share on its way (no host synchronisation); finish: wait, read back, reduce.
int tn_reduce_put(mpmhip_ctx *c, const double *vals, int n, int op) {
  auto &N = c->tn;
  if (n < 1 || n > tplan::RED_N) return fail(c, MPMHIP_EINVAL, "reduce: 1 .. %d values", tplan::RED_N);
  if (op != MPMHIP_REDUCE_SUM && op != MPMHIP_REDUCE_MAX && op != MPMHIP_REDUCE_MIN) return fail(c, MPMHIP_EINVAL, "reduce: unknown operation %d", op);
  N.red_epoch++;
  double *h = reinterpret_cast<double *>(c->h_pinned + tplan::RED_PIN_WORD);
  for (int i = 0; i < tplan::RED_N; i++) h[i] = i < n ? vals[i] : 0.0;
  HIPCHK(c, hipMemcpyAsync(N.d_red, h, sizeof(double) * tplan::RED_N, hipMemcpyHostToDevice, c->stream));
  if (N.wire == MPMHIP_WIRE_RCCL && N.comm) {  // (also with one rank: the binding is exercised on every box)
    const ncclRedOp_t rop = op == MPMHIP_REDUCE_SUM ? ncclSum : (op == MPMHIP_REDUCE_MAX ? ncclMax : ncclMin);
    NCCLCHK(c, rccl_api()->AllReduce(N.d_red, N.d_red, (size_t)n, ncclDouble, rop, (ncclComm_t)N.comm, c->stream));
    return MPMHIP_OK;
  }
  if (N.world == 1) return MPMHIP_OK;
  PutList L;
  memset(&L, 0, sizeof L);
  const int par = (int)(N.red_epoch & 1u);
  for (int p = 0; p < N.world; p++) {
    const auto &P = N.peers[p];
    L.src[p] = reinterpret_cast<const uint32_t *>(N.d_red.get());
    L.dst[p] = reinterpret_cast<uint32_t *>(P.red[par] + (size_t)c->T.rank * tplan::RED_N);
    L.flag[p] = P.flags + 3 * tplan::MAX_WORLD + c->T.rank;
    L.words[p] = 2u * (uint32_t)tplan::RED_N;
  }
  hipLaunchKernelGGL(k_put, dim3(N.world, 1), dim3(256), 0, c->stream, L, N.red_epoch, N.d_done);
  return launch_check(c, "put (reduction row)");
}
int tn_reduce_finish(mpmhip_ctx *c, double *vals, int n, int op) {
  auto &N = c->tn;
  double *h = reinterpret_cast<double *>(c->h_pinned + tplan::RED_PIN_WORD);
  if (N.world == 1 || N.wire == MPMHIP_WIRE_RCCL) {
    HIPCHK(c, hipMemcpyAsync(h, N.d_red, sizeof(double) * tplan::RED_N, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; i++) vals[i] = h[i];
    return MPMHIP_OK;
  }
  int rc = tn_wait(c, N.flags + 3 * tplan::MAX_WORLD, N.all_ranks, N.d_all_idx, N.red_epoch);
  if (rc) return rc;
  const int par = (int)(N.red_epoch & 1u);
  HIPCHK(c, hipMemcpyAsync(h, N.peers[c->T.rank].red[par], sizeof(double) * tplan::RED_N * N.world, hipMemcpyDeviceToHost, c->stream));
  Counters hc;
  if ((rc = read_counters(c, hc))) return rc;  // synchronises; reports a wait that timed out
  for (int i = 0; i < n; i++) {
    double v = h[i];
    for (int r = 1; r < N.world; r++) {
      const double w = h[(size_t)r * tplan::RED_N + i];
      v = op == MPMHIP_REDUCE_SUM ? v + w : (op == MPMHIP_REDUCE_MAX ? std::max(v, w) : std::min(v, w));
    }
    vals[i] = v;
  }
  return MPMHIP_OK;
}

int tn_check_ready(mpmhip_ctx *c, const char *who) {
  if (!c->tn.on) return fail(c, MPMHIP_EINVAL, "%s needs mpmhip_tiled_setup first", who);
  if (!tn_connected(c)) return fail(c, MPMHIP_EINVAL, "%s: the wire is not connected (mpmhip_comm_init / mpmhip_tiled_ipc_connect / mpmhip_tiled_connect_local)", who);
  return MPMHIP_OK;
}

// the whole job's energy on one rank (mpmhip_calculate_energy of a tiled ctx): this rank's share with the peers' halo sums, then
// the sum over the ranks.  out = {kinetic, potential, particles without potential_energy()}
int tn_energy(mpmhip_ctx *c, double out[3]) {
  int rc = tn_check_ready(c, "calculate_energy");
  if (rc) return rc;
  if (c->tn.wire == MPMHIP_WIRE_LOCAL) return fail(c, MPMHIP_EINVAL, "ranks of a local job compute their energy together: mpmhip_calculate_energy_group");
  if (c->tn.rows) return fail(c, MPMHIP_EINVAL, "calculate_energy of a tiled job with rigid bodies is not supported (its rasterization hands the bodies impulses)");
  if ((rc = energy_begin(c)) || (rc = tn_exchange_start(c)) || (rc = tn_exchange_wait(c)) || (rc = energy_end(c, out))) return rc;
  if ((rc = tn_reduce_put(c, out, 3, MPMHIP_REDUCE_SUM))) return rc;
  return tn_reduce_finish(c, out, 3, MPMHIP_REDUCE_SUM);
}

// the arena, with the mappings of the peers' arenas
void tn_drop_arena(mpmhip_ctx::TiledNative &N) {
  for (auto &p : N.peers)
    if (p.ipc_base) (void)hipIpcCloseMemHandle(p.ipc_base);
  N.peers.clear();
  (void)hipFree(N.arena);  // the one array the host layer frees by hand (TiledNative::arena)
  N.arena = nullptr;
  N.handle_valid = false;
}

// keep_ipc (an IPC job set up again, mpmhip_tiled_setup): the arena, its handle and the mappings of the peers' arenas stay in the
// ctx for the new set-up to take over or release.  Freeing an exported arena and exporting / opening a fresh one in the same
// processes is not reliable in the HIP runtime: a re-wired two-rank job then waited in vain for its peer's epochs, or the export
// of the fresh arena failed (bench.py --wire both on ranks that share a GPU, tests/test_gpu_tiled.py)
void tn_release(mpmhip_ctx *c, bool keep_ipc) {
  auto &N = c->tn;
  keep_ipc = keep_ipc && N.wire == MPMHIP_WIRE_IPC && N.arena;
  if (!keep_ipc) tn_drop_arena(N);
  if (N.side) { (void)hipStreamSynchronize(N.side); (void)hipStreamDestroy(N.side); }
  if (N.ev_a) (void)hipEventDestroy(N.ev_a);
  if (N.ev_b) (void)hipEventDestroy(N.ev_b);
  if (N.comm && rccl_api()->handle) (void)rccl_api()->CommDestroy((ncclComm_t)N.comm);
  mpmhip_ctx::TiledNative kept;
  if (keep_ipc) {
    kept.wire = N.wire;
    kept.arena = N.arena;
    kept.lay = N.lay;
    kept.peers.swap(N.peers);
    memcpy(kept.handle, N.handle, sizeof kept.handle);
    kept.handle_valid = N.handle_valid;
  }
  N = std::move(kept);  // (releases this set-up's own arrays)
}

void tn_free(mpmhip_ctx *c) { tn_release(c, false); }

}  // namespace

extern "C" {

int mpmhip_comm_unique_id(uint8_t id[MPMHIP_COMM_ID_BYTES]) {
  if (!id) return MPMHIP_EINVAL;
  RcclApi *R = rccl_api();
  if (!R->handle) return fail(nullptr, MPMHIP_EHIP, "librccl could not be loaded: %s", R->error.c_str());
  ncclUniqueId u;
  static_assert(sizeof u == MPMHIP_COMM_ID_BYTES, "ncclUniqueId size");
  ncclResult_t r = R->GetUniqueId(&u);
  if (r != ncclSuccess) return fail(nullptr, MPMHIP_EHIP, "ncclGetUniqueId failed: %s", R->GetErrorString(r));
  memcpy(id, &u, sizeof u);
  return MPMHIP_OK;
}

int mpmhip_comm_init(mpmhip_ctx *c, const uint8_t id[MPMHIP_COMM_ID_BYTES], int32_t rank, int32_t world) {
  if (!c || !id) return MPMHIP_EINVAL;
  if (world < 1 || world > tplan::MAX_WORLD || rank < 0 || rank >= world) return fail(c, MPMHIP_EINVAL, "rank %d of %d (at most %d ranks)", rank, world, tplan::MAX_WORLD);
  if (c->tn.comm) return fail(c, MPMHIP_EINVAL, "this ctx already has a communicator");
  RcclApi *R = rccl_api();
  if (!R->handle) return fail(c, MPMHIP_EHIP, "librccl could not be loaded: %s", R->error.c_str());
  HIPCHK(c, hipSetDevice(c->device));
  ncclUniqueId u;
  memcpy(&u, id, sizeof u);
  ncclComm_t comm = nullptr;
  NCCLCHK(c, R->CommInitRank(&comm, world, u, rank));
  c->tn.comm = comm;
  c->tn.comm_rank = rank; c->tn.comm_world = world;
  return MPMHIP_OK;
}

int mpmhip_comm_destroy(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  if (!c->tn.comm) return MPMHIP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  NCCLCHK(c, rccl_api()->CommDestroy((ncclComm_t)c->tn.comm));
  c->tn.comm = nullptr;
  return MPMHIP_OK;
}

int mpmhip_comm_selftest(mpmhip_ctx *c) {
  if (!c) return MPMHIP_EINVAL;
  auto &N = c->tn;
  if (!N.comm) return fail(c, MPMHIP_EINVAL, "mpmhip_comm_init first");
  RcclApi *R = rccl_api();
  HIPCHK(c, hipSetDevice(c->device));
  const int world = N.comm_world, me = N.comm_rank, n = 1024;
  DevBuf<uint32_t> d;
  HIPCHK(c, d.alloc((size_t)n * (world + 3)));
  std::vector<uint32_t> h((size_t)n * (world + 3));
  for (int i = 0; i < n; i++) h[i] = (uint32_t)(me * 1000003 + i);
  hipError_t e = hipMemcpy(d, h.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(c, MPMHIP_EHIP, "selftest upload: %s", hipGetErrorString(e));
  uint32_t *gathered = d + n, *ring = d + (size_t)n * (world + 1), *ring_out = ring + n;
  ncclResult_t r = R->AllGather(d, gathered, n, ncclUint32, (ncclComm_t)N.comm, c->stream);
  const int next = (me + 1) % world, prev = (me + world - 1) % world;
  if (r == ncclSuccess) r = R->GroupStart();
  if (r == ncclSuccess) r = R->Send(d, n, ncclUint32, next, (ncclComm_t)N.comm, c->stream);
  if (r == ncclSuccess) r = R->Recv(ring, n, ncclUint32, prev, (ncclComm_t)N.comm, c->stream);
  if (r == ncclSuccess) r = R->GroupEnd();
  // all-reduce (sum) of the first 8 words as uint32: word i becomes sum over ranks of (rank * 1000003 + i), into ring_out
  if (r == ncclSuccess) r = R->AllReduce(d, ring_out, 8, ncclUint32, ncclSum, (ncclComm_t)N.comm, c->stream);
  if (r != ncclSuccess) return fail(c, MPMHIP_EHIP, "selftest: %s", R->GetErrorString(r));
  e = hipMemcpyAsync(h.data(), d, sizeof(uint32_t) * h.size(), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, MPMHIP_EHIP, "selftest read-back: %s", hipGetErrorString(e));
  for (int s = 0; s < world; s++)
    for (int i = 0; i < n; i++)
      if (h[(size_t)n * (1 + s) + i] != (uint32_t)(s * 1000003 + i)) return fail(c, MPMHIP_EHIP, "selftest: all-gather delivered wrong data (rank %d, word %d)", s, i);
  for (int i = 0; i < n; i++)
    if (h[(size_t)n * (world + 1) + i] != (uint32_t)(prev * 1000003 + i)) return fail(c, MPMHIP_EHIP, "selftest: send / receive delivered wrong data (word %d)", i);
  for (int i = 0; i < 8; i++) {
    uint32_t want = 0;
    for (int s = 0; s < world; s++) want += (uint32_t)(s * 1000003 + i);
    if (h[(size_t)n * (world + 2) + i] != want) return fail(c, MPMHIP_EHIP, "selftest: all-reduce delivered wrong data (word %d)", i);
  }
  return MPMHIP_OK;
}

int mpmhip_tiled_setup(mpmhip_ctx *c, const mpmhip_tiled_config *cfg, const int32_t *cuts_x, const int32_t *cuts_y, const int32_t *cuts_z) {
  if (!c || !cfg || !cuts_x || !cuts_y || !cuts_z) return MPMHIP_EINVAL;
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "tiled_setup inside a substep");
  if (cfg->wire != MPMHIP_WIRE_RCCL && cfg->wire != MPMHIP_WIRE_IPC && cfg->wire != MPMHIP_WIRE_LOCAL && cfg->wire != MPMHIP_WIRE_LOCAL_RCCL)
    return fail(c, MPMHIP_EINVAL, "unknown wire %d", cfg->wire);
  const bool loop_rccl = cfg->wire == MPMHIP_WIRE_LOCAL_RCCL;
  if (loop_rccl && (!c->tn.comm || c->tn.comm_world != 1))
    return fail(c, MPMHIP_EINVAL, "MPMHIP_WIRE_LOCAL_RCCL: every ctx of the job needs its own ONE-rank communicator (mpmhip_comm_init(ctx, id, 0, 1))");
  if (cfg->world != cfg->dims[0] * cfg->dims[1] * cfg->dims[2] || cfg->world > tplan::MAX_WORLD) return fail(c, MPMHIP_EINVAL, "world %d does not match dims (at most %d ranks)", cfg->world, tplan::MAX_WORLD);
  if (cfg->migrate_interval < 0 || cfg->migrate_interval > cfg->margin) return fail(c, MPMHIP_EINVAL, "migrate_interval must be in [0, margin]");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int rc = mpmhip_set_partition(c, cfg->rank, cfg->dims, cuts_x, cuts_y, cuts_z, cfg->margin);
  if (rc) return rc;
  void *keep_comm = c->tn.comm;
  const int keep_rank = c->tn.comm_rank, keep_world = c->tn.comm_world;
  c->tn.comm = nullptr;
  tn_release(c, cfg->wire == MPMHIP_WIRE_IPC);
  auto &N = c->tn;
  const size_t kept_bytes = N.arena ? N.lay.total : 0;  // (an IPC job set up again: its arena is taken over below if the layout holds)
  N.comm = keep_comm; N.comm_rank = keep_rank; N.comm_world = keep_world;
  N.loop_rccl = loop_rccl;
  if (N.comm && !loop_rccl && (N.comm_world != cfg->world || N.comm_rank != cfg->rank)) return fail(c, MPMHIP_EINVAL, "the communicator is rank %d of %d, the partition rank %d of %d", N.comm_rank, N.comm_world, cfg->rank, cfg->world);
  N.world = cfg->world;
  N.wire = loop_rccl ? MPMHIP_WIRE_LOCAL : cfg->wire;  // (everything but the halo boxes travels as on the local wire)
  for (int a = 0; a < 3; a++) {
    N.clip_lo[a] = std::max(0, cfg->clip_lo[a]);
    N.clip_hi[a] = std::min(c->P.res[a] + 1, cfg->clip_hi[a]);
    if (N.clip_lo[a] >= N.clip_hi[a]) return fail(c, MPMHIP_EINVAL, "empty clip box on axis %d", a);
  }
  N.migrate_interval = cfg->migrate_interval > 0 ? cfg->migrate_interval : cfg->margin;
  N.adaptive_cap = cfg->migrate_interval > 0 ? 0 : (cfg->migrate_cap > 0 ? cfg->migrate_cap : 64);
  N.k = 0; N.next_migration = N.migrate_interval;
  N.occ.assign((size_t)N.world * 6, 0);
  N.occ_valid = false; N.initial_scan = false;
  N.timeout_ticks = 100000000ull * (unsigned long long)std::max(1, getenv("MPMHIP_TILE_WAIT_S") ? atoi(getenv("MPMHIP_TILE_WAIT_S")) : 20);
  // the arena, sized for the worst-case halo volume over all ranks (tiled_plan.h: Arena; every rank lays its arena out alike)
  uint64_t halo_cap = 0;
  if (const char *refused = tplan::worst_halo_cap(tn_part(c), &halo_cap)) return fail(c, MPMHIP_EINVAL, "%s", refused);
  // (a ctx that holds bodies: the impulse rows of all ranks, both exchanges, behind the nodes of each receive buffer — tiled_plan.h.
  // Every rank of the job must hold the same bodies: the ranks' arenas are then laid out alike)
  N.rows = rigid_active(c);
  if (N.rows) halo_cap += tplan::rows_extra_cap(N.world);
  N.lay = tplan::Arena(halo_cap, cfg->inbox_records > 0 ? (uint64_t)cfg->inbox_records : std::max<uint64_t>(65536, (uint64_t)c->cap / 8));
  if (N.arena && (kept_bytes != N.lay.total || N.peers.size() != (size_t)N.world)) tn_drop_arena(N);
  std::vector<mpmhip_ctx::TiledNative::Peer> mapped;  // (the kept mappings of the peers' arenas)
  mapped.swap(N.peers);
  hipError_t e = hipSuccess;
  if (N.arena) {
    // the kept arena: zeroed below like a fresh one (every rank has synchronised its stream and passed the caller's barrier, so no
    // peer writes into it until the job is connected again)
  } else if (N.wire == MPMHIP_WIRE_IPC) {
    // written by kernels of other devices while kernels of this one poll and read it: fine-grained (coherent at system
    // scope while kernels run); MPMHIP_TILE_COARSE=1 allocates ordinary device memory instead (single-device tests)
    const bool coarse = getenv("MPMHIP_TILE_COARSE") && atoi(getenv("MPMHIP_TILE_COARSE")) != 0;
    e = coarse ? hipMalloc((void **)&N.arena, N.lay.total) : hipExtMallocWithFlags((void **)&N.arena, N.lay.total, hipDeviceMallocFinegrained);
  } else {
    e = hipMalloc((void **)&N.arena, N.lay.total);
  }
  if (e != hipSuccess) return fail(c, MPMHIP_ENOMEM, "halo arena of %zu bytes: %s", N.lay.total, hipGetErrorString(e));
  HIPCHK(c, hipMemset(N.arena, 0, N.lay.total));
  mpmhip_ctx::TiledNative::Peer self;
  tn_carve(self, N.arena, N.lay);
  N.flags = self.flags; N.table[0] = self.table[0]; N.table[1] = self.table[1];
  N.recv[0] = self.recv[0]; N.recv[1] = self.recv[1]; N.inbox = self.inbox;
  N.peers.assign((size_t)N.world, mpmhip_ctx::TiledNative::Peer());
  N.peers[cfg->rank] = self;
  for (size_t p = 0; p < mapped.size(); p++)  // (mpmhip_tiled_ipc_connect keeps a mapping whose peer hands over the same handle)
    if ((int)p != cfg->rank && mapped[p].ipc_base) {
      N.peers[p].ipc_base = mapped[p].ipc_base;
      memcpy(N.peers[p].handle, mapped[p].handle, sizeof mapped[p].handle);
    }
  if (!tn_peer_wire(N)) HIPCHK(c, N.send.alloc((size_t)N.lay.halo_cap));
  if (N.rows) HIPCHK(c, N.d_row_stage.alloc((size_t)tplan::IMP_ROW_FLOATS));
  HIPCHK(c, N.row.alloc((size_t)tplan::ROW));
  HIPCHK(c, hipMemset(N.row, 0, sizeof(uint32_t) * tplan::ROW));
  for (int k = 0; k < 2; k++) HIPCHK(c, N.d_boxes[k].alloc((size_t)MPMHIP_MAX_HALO_BOXES));
  HIPCHK(c, N.d_halo_idx.alloc((size_t)MPMHIP_MAX_HALO_BOXES));
  HIPCHK(c, N.d_all_idx.alloc((size_t)tplan::MAX_WORLD));
  HIPCHK(c, N.d_red.alloc((size_t)tplan::RED_N * (tplan::MAX_WORLD + 1)));
  HIPCHK(c, N.d_done.alloc((size_t)tplan::MAX_WORLD + 1));
  HIPCHK(c, hipMemset(N.d_done, 0, sizeof(uint32_t) * (tplan::MAX_WORLD + 1)));
  N.all_ranks.resize((size_t)N.world);
  for (int r = 0; r < N.world; r++) N.all_ranks[r] = r;
  HIPCHK(c, hipMemcpy(N.d_all_idx, N.all_ranks.data(), sizeof(int) * N.world, hipMemcpyHostToDevice));
  if (N.wire == MPMHIP_WIRE_RCCL || N.loop_rccl) {
    HIPCHK(c, hipStreamCreateWithFlags(&N.side, hipStreamNonBlocking));
    HIPCHK(c, hipEventCreateWithFlags(&N.ev_a, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&N.ev_b, hipEventDisableTiming));
  }
  N.on = true;
  N.connected = N.world == 1;
  c->overlap = cfg->overlap != 0;
  return tn_apply_plan(c);
}

int mpmhip_tiled_ipc_handle(mpmhip_ctx *c, uint8_t handle[MPMHIP_IPC_HANDLE_BYTES]) {
  if (!c || !handle) return MPMHIP_EINVAL;
  if (!c->tn.on || c->tn.wire != MPMHIP_WIRE_IPC) return fail(c, MPMHIP_EINVAL, "ipc_handle needs mpmhip_tiled_setup with MPMHIP_WIRE_IPC");
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->tn.handle_valid) {  // (once per arena: a kept arena hands out the handle its peers have opened)
    hipIpcMemHandle_t h;
    static_assert(sizeof h == MPMHIP_IPC_HANDLE_BYTES, "hipIpcMemHandle_t size");
    HIPCHK(c, hipIpcGetMemHandle(&h, c->tn.arena));
    memcpy(c->tn.handle, &h, sizeof h);
    c->tn.handle_valid = true;
  }
  memcpy(handle, c->tn.handle, MPMHIP_IPC_HANDLE_BYTES);
  return MPMHIP_OK;
}

int mpmhip_tiled_ipc_connect(mpmhip_ctx *c, const uint8_t *handles) {
  if (!c) return MPMHIP_EINVAL;
  auto &N = c->tn;
  if (!N.on || N.wire != MPMHIP_WIRE_IPC) return fail(c, MPMHIP_EINVAL, "ipc_connect needs mpmhip_tiled_setup with MPMHIP_WIRE_IPC");
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<uint8_t> gathered;
  if (!handles) {  // through the ctx's communicator
    if (!N.comm) return fail(c, MPMHIP_EINVAL, "ipc_connect(NULL) needs mpmhip_comm_init");
    uint8_t mine[MPMHIP_IPC_HANDLE_BYTES];
    int rc = mpmhip_tiled_ipc_handle(c, mine);
    if (rc) return rc;
    DevBuf<uint8_t> d;
    HIPCHK(c, d.alloc((size_t)MPMHIP_IPC_HANDLE_BYTES * (N.world + 1)));
    HIPCHK(c, hipMemcpy(d, mine, sizeof mine, hipMemcpyHostToDevice));
    const ncclResult_t r = rccl_api()->AllGather(d, d + MPMHIP_IPC_HANDLE_BYTES, MPMHIP_IPC_HANDLE_BYTES, ncclUint8, (ncclComm_t)N.comm, c->stream);
    if (r != ncclSuccess) return fail(c, MPMHIP_EHIP, "all-gather of the IPC handles: %s", rccl_api()->GetErrorString(r));
    gathered.resize((size_t)MPMHIP_IPC_HANDLE_BYTES * N.world);
    HIPCHK(c, hipMemcpyAsync(gathered.data(), d + MPMHIP_IPC_HANDLE_BYTES, gathered.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    handles = gathered.data();
  }
  for (int p = 0; p < N.world; p++) {
    if (p == c->T.rank) continue;
    auto &P = N.peers[p];
    const uint8_t *hp = handles + (size_t)p * MPMHIP_IPC_HANDLE_BYTES;
    if (P.ipc_base && memcmp(P.handle, hp, sizeof P.handle) == 0) {  // the peer kept its arena: so does this mapping
      tn_carve(P, static_cast<char *>(P.ipc_base), N.lay);
      continue;
    }
    if (P.ipc_base) { (void)hipIpcCloseMemHandle(P.ipc_base); P.ipc_base = nullptr; }
    hipIpcMemHandle_t h;
    memcpy(&h, hp, sizeof h);
    memcpy(P.handle, hp, sizeof P.handle);
    void *base = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&base, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) return fail(c, MPMHIP_EHIP, "hipIpcOpenMemHandle of rank %d's arena: %s", p, hipGetErrorString(e));
    P.ipc_base = base;
    tn_carve(P, static_cast<char *>(base), N.lay);
  }
  N.connected = true;
  return tn_apply_plan(c);
}

int mpmhip_tiled_connect_local(mpmhip_ctx *const *ctxs, int32_t n) {
  if (!ctxs || n < 1) return MPMHIP_EINVAL;
  for (int r = 0; r < n; r++) {
    mpmhip_ctx *c = ctxs[r];
    if (!c) return MPMHIP_EINVAL;
    if (!c->tn.on || c->tn.wire != MPMHIP_WIRE_LOCAL || c->tn.world != n || c->T.rank != r)
      return fail(c, MPMHIP_EINVAL, "connect_local: ctx %d must be set up as rank %d of %d with MPMHIP_WIRE_LOCAL", r, r, n);
    if (c->device != ctxs[0]->device) return fail(c, MPMHIP_EINVAL, "connect_local: all ctx must live on one device");
    if (c->tn.rows != ctxs[0]->tn.rows) return fail(c, MPMHIP_EINVAL, "connect_local: rank %d and rank 0 do not both hold rigid bodies: every rank of a job holds all bodies", r);
    if (c->tn.lay.halo_cap != ctxs[0]->tn.lay.halo_cap) return fail(c, MPMHIP_EINVAL, "connect_local: the ranks' arenas are laid out differently (not the same partition?)");
  }
  for (int r = 0; r < n; r++) {
    mpmhip_ctx *c = ctxs[r];
    if (c->tn.loop_rccl != ctxs[0]->tn.loop_rccl) return fail(c, MPMHIP_EINVAL, "connect_local: the ranks were set up with different wires");
    for (int p = 0; p < n; p++)
      if (p != r) c->tn.peers[p] = ctxs[p]->tn.peers[p];  // (a rank's own entry describes its arena)
    c->tn.local_ctx.assign(ctxs, ctxs + n);
    c->tn.connected = true;
    int rc = tn_apply_plan(c);
    if (rc) return rc;
  }
  return MPMHIP_OK;
}

// 0 begin (+ start of the exchange), 1 interior, 2 wait + end, 3 (a job with bodies) the rigid G2P's rows summed + the bodies' advection
static int tn_substep_parts(mpmhip_ctx *c, int part) {
  int rc;
  if (part == 3) return substep_finish_rows(c);
  if (part == 0) {
    if ((rc = mpmhip_substep_begin(c))) return rc;
    return tn_exchange_start(c);
  }
  if (part == 1) return mpmhip_substep_interior(c);
  if ((rc = tn_exchange_wait(c))) return rc;
  return mpmhip_substep_end(c);
}

int64_t mpmhip_tiled_advance(mpmhip_ctx *c, int64_t n) {
  if (!c || n < 0) return MPMHIP_EINVAL;
  int rc = tn_check_ready(c, "tiled_advance");
  if (rc) return rc;
  auto &N = c->tn;
  if (N.wire == MPMHIP_WIRE_LOCAL && N.world > 1) return fail(c, MPMHIP_EINVAL, "ranks of a local job advance together: mpmhip_tiled_advance_group");
  HIPCHK(c, hipSetDevice(c->device));
  if (n > 0 && !N.occ_valid && N.world > 1) {
    // in front of a job's first substep: one scan + table exchange (no particle is outside its brick yet) — every rank learns every
    // rank's bounds and the halo boxes shrink from the set-up's global clip box to the ranks' own occupancy (tn_mig_c)
    N.initial_scan = true;
    rc = tn_mig_a(c);
    if (!rc) rc = tn_mig_b(c);
    if (!rc) rc = tn_mig_c(c);
    N.initial_scan = false;
    if (rc) return rc;
  }
  for (int64_t i = 0; i < n; i++) {
    for (int part = 0; part < 4; part++)
      if ((rc = tn_substep_parts(c, part))) { c->in_substep = false; c->cur_ev = nullptr; c->rows_substep = false; return rc; }
    N.k++;
    if (N.k >= N.next_migration && N.world > 1) {
      if ((rc = tn_mig_a(c)) || (rc = tn_mig_b(c)) || (rc = tn_mig_c(c))) return rc;
    }
  }
  return n;
}

int64_t mpmhip_tiled_advance_group(mpmhip_ctx *const *ctxs, int32_t n_ctx, int64_t n) {
  if (!ctxs || n_ctx < 1 || n < 0) return MPMHIP_EINVAL;
  for (int r = 0; r < n_ctx; r++) {
    if (!ctxs[r]) return MPMHIP_EINVAL;
    int rc = tn_check_ready(ctxs[r], "tiled_advance_group");
    if (rc) return rc;
    if (ctxs[r]->tn.wire != MPMHIP_WIRE_LOCAL || ctxs[r]->tn.world != n_ctx || ctxs[r]->T.rank != r)
      return fail(ctxs[r], MPMHIP_EINVAL, "advance_group: ctx %d is not rank %d of a local job of %d", r, r, n_ctx);
    if (ctxs[r]->tn.loop_rccl && ctxs[r]->stream != ctxs[0]->stream)
      return fail(ctxs[r], MPMHIP_EINVAL, "MPMHIP_WIRE_LOCAL_RCCL: the ranks of the job must share one stream (mpmhip_set_stream)");
  }
  // ranks that share ONE stream publish their halo epochs with one launch behind the last rank's pack (k_epoch_signal_group)
  bool one_stream = n_ctx > 1 && n_ctx <= MPMHIP_MAX_HALO_BOXES;
  for (int r = 1; r < n_ctx; r++) one_stream = one_stream && ctxs[r]->stream == ctxs[0]->stream && ctxs[r]->device == ctxs[0]->device;
  bool scan0 = false;
  for (int r = 0; r < n_ctx; r++) scan0 = scan0 || !ctxs[r]->tn.occ_valid;
  if (n > 0 && scan0 && n_ctx > 1) {  // (the planning scan in front of the job's first substep: see mpmhip_tiled_advance)
    int rc = MPMHIP_OK;
    for (int r = 0; r < n_ctx; r++) ctxs[r]->tn.initial_scan = true;
    for (int ph = 0; ph < 3 && !rc; ph++)
      for (int r = 0; r < n_ctx && !rc; r++) {
        mpmhip_ctx *c = ctxs[r];
        if (hipSetDevice(c->device) != hipSuccess) { rc = fail(c, MPMHIP_EHIP, "hipSetDevice failed"); break; }
        rc = ph == 0 ? tn_mig_a(c) : (ph == 1 ? tn_mig_b(c) : tn_mig_c(c));
      }
    for (int r = 0; r < n_ctx; r++) ctxs[r]->tn.initial_scan = false;
    if (rc) return rc;
  }
  for (int64_t i = 0; i < n; i++) {
    // begin of every rank (sort, [boundary] P2G, pack: the peers' boxes are written), then interior + end rank by rank
    for (int r = 0; r < n_ctx; r++) {
      ctxs[r]->tn.defer_signal = one_stream && !ctxs[r]->tn.loop_rccl;  // (only inside this loop: energy / reductions signal per rank)
      ctxs[r]->tn.signal_deferred = false;
      int rc = tn_substep_parts(ctxs[r], 0);
      ctxs[r]->tn.defer_signal = false;
      if (rc) { ctxs[r]->in_substep = false; ctxs[r]->cur_ev = nullptr; ctxs[r]->rows_substep = false; return rc; }
    }
    {
      SignalGroup G;
      memset(&G, 0, sizeof G);
      bool any = false;
      for (int r = 0; r < n_ctx; r++) {
        auto &N = ctxs[r]->tn;
        if (!N.signal_deferred) continue;
        N.signal_deferred = false;
        G.boxes[r] = ctxs[r]->d_boxes_cur; G.n[r] = (int)N.plan.boxes.size(); G.epoch[r] = N.epoch;
        any = true;
      }
      if (any) {
        hipLaunchKernelGGL(k_epoch_signal_group, dim3(n_ctx), dim3(64), 0, ctxs[0]->stream, G);
        if (int rc = launch_check(ctxs[0], "epoch_signal_group")) return rc;
      }
    }
    for (int r = 0; r < n_ctx; r++)
      for (int part = 1; part < 3; part++) {
        ctxs[r]->tn.defer_finish = true;  // (a job with bodies: every rank's G2P — its row out — is enqueued before the first rank sums them)
        int rc = tn_substep_parts(ctxs[r], part);
        ctxs[r]->tn.defer_finish = false;
        if (rc) { ctxs[r]->in_substep = false; ctxs[r]->cur_ev = nullptr; ctxs[r]->rows_substep = false; return rc; }
      }
    for (int r = 0; r < n_ctx; r++)
      if (int rc = tn_substep_parts(ctxs[r], 3)) { ctxs[r]->rows_substep = false; return rc; }
    bool due = false;
    for (int r = 0; r < n_ctx; r++) { ctxs[r]->tn.k++; due = due || ctxs[r]->tn.k >= ctxs[r]->tn.next_migration; }
    if (due && n_ctx > 1) {
      for (int ph = 0; ph < 3; ph++)
        for (int r = 0; r < n_ctx; r++) {
          mpmhip_ctx *c = ctxs[r];
          HIPCHK(c, hipSetDevice(c->device));
          int rc = ph == 0 ? tn_mig_a(c) : (ph == 1 ? tn_mig_b(c) : tn_mig_c(c));
          if (rc) return rc;
        }
    }
  }
  return n;
}

int mpmhip_tiled_reduce(mpmhip_ctx *c, double *values, int32_t n, int32_t op) {
  if (!c || !values) return MPMHIP_EINVAL;
  int rc = tn_check_ready(c, "tiled_reduce");
  if (rc) return rc;
  if (c->tn.wire == MPMHIP_WIRE_LOCAL && c->tn.world > 1) return fail(c, MPMHIP_EINVAL, "ranks of a local job reduce together: mpmhip_tiled_reduce_group");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = tn_reduce_put(c, values, n, op))) return rc;
  return tn_reduce_finish(c, values, n, op);
}

static int tn_check_group(mpmhip_ctx *const *ctxs, int32_t n_ctx, const char *who) {
  if (!ctxs || n_ctx < 1) return MPMHIP_EINVAL;
  for (int r = 0; r < n_ctx; r++) {
    if (!ctxs[r]) return MPMHIP_EINVAL;
    int rc = tn_check_ready(ctxs[r], who);
    if (rc) return rc;
    if (ctxs[r]->tn.wire != MPMHIP_WIRE_LOCAL || ctxs[r]->tn.world != n_ctx || ctxs[r]->T.rank != r)
      return fail(ctxs[r], MPMHIP_EINVAL, "%s: ctx %d is not rank %d of a local job of %d", who, r, r, n_ctx);
  }
  return MPMHIP_OK;
}

int mpmhip_tiled_reduce_group(mpmhip_ctx *const *ctxs, int32_t n_ctx, double *values, int32_t n, int32_t op) {
  int rc = tn_check_group(ctxs, n_ctx, "tiled_reduce_group");
  if (rc || !values) return rc ? rc : MPMHIP_EINVAL;
  for (int r = 0; r < n_ctx; r++) {  // every rank's row on its way, then every rank reads the table
    HIPCHK(ctxs[r], hipSetDevice(ctxs[r]->device));
    if ((rc = tn_reduce_put(ctxs[r], values + (size_t)r * n, n, op))) return rc;
  }
  for (int r = 0; r < n_ctx; r++)
    if ((rc = tn_reduce_finish(ctxs[r], values + (size_t)r * n, n, op))) return rc;
  return MPMHIP_OK;
}

int mpmhip_calculate_energy_group(mpmhip_ctx *const *ctxs, int32_t n_ctx, double *kinetic, double *potential) {
  int rc = tn_check_group(ctxs, n_ctx, "calculate_energy_group");
  if (rc || !kinetic || !potential) return rc ? rc : MPMHIP_EINVAL;
  std::vector<double> e((size_t)n_ctx * 3);
  for (int r = 0; r < n_ctx; r++) {
    mpmhip_ctx *c = ctxs[r];
    HIPCHK(c, hipSetDevice(c->device));
    if (c->in_substep) return fail(c, MPMHIP_EINVAL, "calculate_energy inside a substep");
    if (c->tn.rows) return fail(c, MPMHIP_EINVAL, "calculate_energy of a tiled job with rigid bodies is not supported (its rasterization hands the bodies impulses)");
    if ((rc = energy_begin(c)) || (rc = tn_exchange_start(c))) return rc;
  }
  for (int r = 0; r < n_ctx; r++)
    if ((rc = tn_exchange_wait(ctxs[r])) || (rc = energy_end(ctxs[r], &e[(size_t)r * 3]))) return rc;
  if ((rc = mpmhip_tiled_reduce_group(ctxs, n_ctx, e.data(), 3, MPMHIP_REDUCE_SUM))) return rc;
  *kinetic = e[0];
  *potential = e[1];
  if (e[2] != 0.0)
    return fail(ctxs[0], MPMHIP_ENOTIMPL, "%.0f particles are of a type without potential_energy() (reference: TC_NOT_IMPLEMENTED); "
                "kinetic energy is valid", e[2]);
  return MPMHIP_OK;
}

// {live particles, active blocks, sticky error word (OR), particles migrated out so far} of the whole job
static int tn_totals_local(mpmhip_ctx *c, double v[8]) {
  Counters h;
  HIPCHK(c, hipSetDevice(c->device));
  // (the error word is read as it is: read_counters would turn a set bit into this rank's failure before the others have seen it)
  Counters *pin = reinterpret_cast<Counters *>(c->h_pinned.get());
  HIPCHK(c, hipMemcpyAsync(pin, c->cnt, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  h = *pin;
  v[0] = (double)(c->n_slots - (int64_t)h.n_dead);  // (= mpmhip_num_particles)
  v[1] = (double)h.n_active; v[2] = (double)c->tn.migrated_out;
  for (int b = 0; b < 5; b++) v[3 + b] = (double)((h.error >> b) & 1u);
  return MPMHIP_OK;
}
static void tn_totals_out(const double v[8], int64_t out[4]) {
  out[0] = (int64_t)v[0]; out[1] = (int64_t)v[1]; out[3] = (int64_t)v[2];
  int64_t err = 0;
  for (int b = 0; b < 5; b++) if (v[3 + b] > 0.0) err |= 1ll << b;
  out[2] = err;
}
int mpmhip_tiled_totals(mpmhip_ctx *c, int64_t out[4]) {
  if (!c || !out) return MPMHIP_EINVAL;
  int rc = tn_check_ready(c, "tiled_totals");
  if (rc) return rc;
  if (c->tn.wire == MPMHIP_WIRE_LOCAL && c->tn.world > 1) return fail(c, MPMHIP_EINVAL, "ranks of a local job: mpmhip_tiled_totals_group");
  double v[8];
  if ((rc = tn_totals_local(c, v)) || (rc = tn_reduce_put(c, v, 8, MPMHIP_REDUCE_SUM)) || (rc = tn_reduce_finish(c, v, 8, MPMHIP_REDUCE_SUM))) return rc;
  tn_totals_out(v, out);
  return MPMHIP_OK;
}
int mpmhip_tiled_totals_group(mpmhip_ctx *const *ctxs, int32_t n_ctx, int64_t out[4]) {
  int rc = tn_check_group(ctxs, n_ctx, "tiled_totals_group");
  if (rc || !out) return rc ? rc : MPMHIP_EINVAL;
  std::vector<double> v((size_t)n_ctx * 8);
  for (int r = 0; r < n_ctx; r++)
    if ((rc = tn_totals_local(ctxs[r], &v[(size_t)r * 8]))) return rc;
  if ((rc = mpmhip_tiled_reduce_group(ctxs, n_ctx, v.data(), 8, MPMHIP_REDUCE_SUM))) return rc;
  tn_totals_out(v.data(), out);
  return MPMHIP_OK;
}

int mpmhip_live_histogram(mpmhip_ctx *c, int64_t *hist_x, int64_t *hist_y, int64_t *hist_z, int64_t *total, int32_t cell_bounds[6]) {
  if (!c) return MPMHIP_EINVAL;
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "live_histogram inside a substep");
  HIPCHK(c, hipSetDevice(c->device));
  const int *res = c->P.res;
  const size_t bins = (size_t)res[0] + res[1] + res[2], words = bins + 1 + 3;  // rows | total | the six bounds as three 64-bit words
  auto &d = c->d_live_hist;
  if (!d) HIPCHK(c, d.alloc(words));
  std::vector<unsigned long long> h(words, 0ull);
  int init[6] = {1 << 30, 1 << 30, 1 << 30, -1, -1, -1};
  memcpy(&h[bins + 1], init, sizeof init);
  HIPCHK(c, hipMemcpyAsync(d, h.data(), sizeof(unsigned long long) * words, hipMemcpyHostToDevice, c->stream));
  if (c->n_slots > 0) {
    // few workgroups, two per CU: each flushes at most `bins` 64-bit atomics (12 KB at res = 512, as many as it has occupied bins),
    // and at 8 M slots reads 1 MB of records: the flush stays a hundredth of the particle traffic
    const size_t lds = sizeof(int32_t) * bins;
    const int grid = std::max(1, std::min(particle_grid(c->n_slots), 2 * std::max(1, (int)c->n_cus)));
    int *bounds = reinterpret_cast<int *>(d.get() + bins + 1);
    if (lds <= 65536 - 256)
      hipLaunchKernelGGL(k_live_histogram<true>, dim3(grid), dim3(256), lds, c->stream, c->P, (const float4 *)c->rg.get(), d.get(), bounds);
    else
      hipLaunchKernelGGL(k_live_histogram<false>, dim3(grid), dim3(256), 0, c->stream, c->P, (const float4 *)c->rg.get(), d.get(), bounds);
    if (int rc = launch_check(c, "live_histogram")) return rc;
  }
  HIPCHK(c, hipMemcpyAsync(h.data(), d, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int64_t *out[3] = {hist_x, hist_y, hist_z};
  size_t at = 0;
  for (int a = 0; a < 3; at += (size_t)res[a], a++)
    if (out[a]) for (int i = 0; i < res[a]; i++) out[a][i] = (int64_t)h[at + (size_t)i];
  const int64_t n = (int64_t)h[bins];
  if (total) *total = n;
  if (cell_bounds) {
    int b[6];
    memcpy(b, &h[bins + 1], sizeof b);
    for (int k = 0; k < 6; k++) cell_bounds[k] = n ? b[k] : 0;
  }
  return MPMHIP_OK;
}

int mpmhip_balanced_cuts(int32_t res, int32_t parts, const int64_t *hist, int32_t *cuts) {
  if (!hist || !cuts) return MPMHIP_EINVAL;
  if (parts < 1 || parts > MPMHIP_MAX_PARTS || res < parts) return fail(nullptr, MPMHIP_EINVAL, "balanced_cuts: 1 <= parts <= min(%d, res)", MPMHIP_MAX_PARTS);
  for (int i = 0; i < res; i++)
    if (hist[i] < 0) return fail(nullptr, MPMHIP_EINVAL, "balanced_cuts: a negative count");
  int out[MPMHIP_MAX_PARTS + 1];
  tplan::balanced_cuts(res, parts, hist, out);
  for (int k = 0; k <= parts; k++) cuts[k] = out[k];
  return MPMHIP_OK;
}

int mpmhip_tiled_redistribute(mpmhip_ctx *c, int64_t info[4]) {
  if (!c) return MPMHIP_EINVAL;
  if (info) for (int k = 0; k < 4; k++) info[k] = 0;
  int rc = tn_check_ready(c, "tiled_redistribute");
  if (rc) return rc;
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "tiled_redistribute inside a substep");
  if (c->tn.wire == MPMHIP_WIRE_LOCAL && c->tn.world > 1) return fail(c, MPMHIP_EINVAL, "ranks of a local job are redistributed together: mpmhip_tiled_redistribute_group");
  if (c->tn.rows) return fail(c, MPMHIP_EINVAL, "tiled_redistribute: a job with rigid bodies is not re-cut (a follow-up)");
  if (c->tn.world == 1) return MPMHIP_OK;
  mpmhip_ctx *one[1] = {c};
  return tn_redistribute(one, 1, info);
}
int mpmhip_tiled_redistribute_group(mpmhip_ctx *const *ctxs, int32_t n_ctx, int64_t *info) {
  int rc = tn_check_group(ctxs, n_ctx, "tiled_redistribute_group");
  if (rc) return rc;
  if (info) for (int k = 0; k < 4 * n_ctx; k++) info[k] = 0;
  for (int r = 0; r < n_ctx; r++)
    if (ctxs[r]->in_substep) return fail(ctxs[r], MPMHIP_EINVAL, "tiled_redistribute inside a substep");
  for (int r = 0; r < n_ctx; r++)
    if (ctxs[r]->tn.rows) return fail(ctxs[r], MPMHIP_EINVAL, "tiled_redistribute: a job with rigid bodies is not re-cut (a follow-up)");
  if (n_ctx == 1) return MPMHIP_OK;
  return tn_redistribute(ctxs, n_ctx, info);
}

int mpmhip_tiled_state(mpmhip_ctx *c, int64_t out[8]) {
  if (!c || !out) return MPMHIP_EINVAL;
  const auto &N = c->tn;
  out[0] = N.k; out[1] = N.next_migration; out[2] = N.migrated_out; out[3] = N.migrations; out[4] = N.replans;
  out[5] = (int64_t)N.plan.boxes.size(); out[6] = (int64_t)N.plan.total; out[7] = N.on ? (N.loop_rccl ? (int)MPMHIP_WIRE_LOCAL_RCCL : N.wire) : 0;
  return MPMHIP_OK;
}

int32_t mpmhip_tiled_plan(mpmhip_ctx *c, int32_t capacity, mpmhip_halo_box *out) {
  if (!c) return MPMHIP_EINVAL;
  const auto &N = c->tn;
  if (!N.on) return fail(c, MPMHIP_EINVAL, "tiled_plan needs mpmhip_tiled_setup first");
  const int32_t n = (int32_t)N.plan.boxes.size();
  if (!out || capacity < n) return n;
  const bool peer_wire = tn_peer_wire(N);
  for (int32_t i = 0; i < n; i++) {
    const auto &b = N.plan.boxes[i];
    for (int a = 0; a < 3; a++) { out[i].lo[a] = b.lo[a]; out[i].hi[a] = b.hi[a]; }
    out[i].peer = b.peer; out[i].reserved = (int32_t)b.peer_off;
    out[i].send = peer_wire ? nullptr : (void *)(N.send + b.off);
    out[i].recv = N.recv[0] + b.off;
  }
  return n;
}

}  // extern "C"
