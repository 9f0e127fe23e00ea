// taichi_mpm_amd/csrc/snapshot_blob.h — the three whole-state snapshot formats as data: header structs, record geometry, ONE layout
// function and ONE check function per format.  Part of libmpmhip; pure C++ (no HIP header: tests/test_snapshot_blob_cpu.py builds
// it with g++ and runs tests/cpp/snapshot_blob_host.cpp under the sanitizers).  snapshot_api.h does the copies; the section
// tables are in DESIGN.md ("Snapshot layouts").
//
// A layout function turns counts into {offset, length} of every section, in 64 bits, each count bounded by what is left of the
// blob BEFORE it is multiplied.  A check function reads host bytes only (memcpy, never a cast of a blob pointer), performs every
// test a loader needs before it may touch its context, and hands back the parsed headers with the checked layout: the loader
// copies from that and from nothing else.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "async_sched.h"  // AsyncSched::limits_are_sane
#include "group_params.h"

namespace snap {

using mpm::GroupParams;

// ------------------------------------------------------------------------------------------------ headers
struct SnapHeader {
  char magic[8];  // "MPMHIP01"
  uint32_t abi, n_groups;
  int64_t n_slots, substeps;
  int32_t next_pid, b_stale, store_b, res[3];
  float t, request_t, dx, dt;
  uint32_t n_dead, pad;
};
// scenes with rigid bodies append the bodies' records (pose, velocities, mass properties) and the joints: meshes, boundary
// particles and scripts come from the scene again (the script adds the same bodies before it loads), like the level set
struct SnapRigid {
  char magic[8];  // "MPMRIGID"
  uint32_t n_bodies, n_joints, sizeof_body, sizeof_joint;
};
// ... and, behind the joints, the settings of the rigid-rigid collision pass (a blob that ends before it keeps the ctx's own)
struct SnapRigidCollide {
  char magic[8];  // "MPMRRCOL"
  int32_t on, iterations, position_iterations;
  float penalty;
};
struct SnapAsync {
  char magic[8];  // "MPMASYNC"
  uint32_t abi, n_groups;
  int32_t res[3], nb[3];
  float dx, unit_delta_t;
  int64_t nblk, containers, current_t_int, min_delta_t_int, max_delta_t_int, update_counter, step_counter;
  int32_t next_pid, pad;
  float request_t, current_t;
};
struct Snap2D {
  char magic[8];  // "MPM2DSNP"
  uint32_t abi, n_groups;
  int32_t res[2], next_pid, n_bodies, n_joints, has_async;
  int64_t n;
  float dx, base_dt, t, request_t;
  uint32_t n_dead, n_ranked;
  // asynchronous stepper (has_async)
  int32_t nb[2];
  float unit_delta_t, a_request_t, a_current_t, pad;
  int64_t nblk, containers, current_t_int, min_delta_t_int, max_delta_t_int, update_counter, step_counter;
};
static_assert(sizeof(SnapHeader) == 80 && sizeof(SnapRigid) == 24 && sizeof(SnapRigidCollide) == 24, "3D snapshot headers");
static_assert(sizeof(SnapAsync) == 120 && sizeof(Snap2D) == 152, "async / 2D snapshot headers");

// ------------------------------------------------------------------------------------------------ record geometry
// copies of the device-side sizes and offsets (mpmhip.hip pins every one to the real type with static_assert / offsetof)
constexpr uint64_t GROUP_BYTES = sizeof(GroupParams);
constexpr uint64_t RECG_BYTES = 64, RECP_BYTES = 64, BROW_BYTES = 48;  // RecG, RecP, one row of BW floats of apic_b
constexpr uint64_t RECG_GID = 52, RECG_PID = 56;                        // group id and creation id inside a RecG
constexpr uint64_t REC2_BYTES = 64, REC2_GID = 52, REC2_ID = 56;        // the 2D container record {x2 v2, F4, apic_b4, aux gid id -}
constexpr uint64_t TAG_BYTES = 4, ID_BYTES = 4;                         // a container's block tag; the id word of a 3D container
constexpr uint64_t CONTAINER3_BYTES = TAG_BYTES + ID_BYTES + RECG_BYTES + 64;  // tag, id, g (a RecG image), w
constexpr uint64_t CONTAINER2_BYTES = TAG_BYTES + REC2_BYTES;
constexpr uint64_t W3_BYTES = 64;                                       // the second record of a 3D container {v3 -, apic_b9 ...}
constexpr uint64_t BODY3_BYTES = 188, JOINT3_BYTES = 168, JOINT3_OBJ0 = 4, JOINT3_OBJ1 = 8;  // RigidBodyDev, JointDev
constexpr uint32_t MAX_JOINTS3 = 32;
constexpr uint64_t BODY2_BYTES = 68, JOINTS2_BYTES = 260;               // mpm2d::Rigid2, mpm2d::Joints2 {n, Joint2 j[MAX_JOINTS2]}
constexpr uint64_t JOINTS2_N = 0, JOINTS2_FIRST = 4, JOINT2_BYTES = 16, JOINT2_OBJ0 = 0, JOINT2_OBJ1 = 4;
constexpr int32_t MAX_JOINTS2 = 16;
constexpr uint64_t RANK_BYTES = 4, COLOUR_BYTES = 4;                    // rank of a ranked boundary particle; a particle's colour word
constexpr uint64_t TABLE_WORD = 8;                                      // one entry of a block table (int64)
constexpr int N_TABLES = 6;                                             // continuous, strength, cfl, particle_t, backup_t, local_min
constexpr uint32_t TAG_FREE = 0xFFFFFFFFu, TAG_BACKUP = 0x80000000u;    // AS_FREE, AS_BACKUP (k_async.h)
// the particle arrays of the 2D object, in blob order
enum { P2_X, P2_V, P2_F, P2_B, P2_AUX, P2_GID, P2_PID, P2_ARRAYS };
constexpr uint64_t P2_BYTES[P2_ARRAYS] = {8, 8, 16, 16, 4, 4, 4};

// ------------------------------------------------------------------------------------------------ sections
struct Sec { uint64_t off = 0, len = 0; };
constexpr uint64_t NO_LIMIT = 1ull << 62;  // saving: the counts are the ctx's own

// hands out consecutive sections of a blob of `limit` bytes; a count that does not fit what is left sets `ok` to false for good
struct Cursor {
  uint64_t limit, at = 0;
  bool ok = true;
  explicit Cursor(uint64_t limit_) : limit(limit_) {}
  Sec take(uint64_t count, uint64_t each) {
    Sec s;
    s.off = at;
    if (!ok || count > (limit - at) / each) { ok = false; return s; }
    s.len = count * each;
    at += s.len;
    return s;
  }
};

struct Verdict {
  int rc = MPMHIP_OK;
  std::string msg;
  bool ok() const { return rc == MPMHIP_OK; }
};
inline Verdict refuse(int rc, const char *msg) { Verdict v; v.rc = rc; v.msg = msg; return v; }
template <class... A>
inline Verdict refuse(int rc, const char *fmt, A... a) {
  char buf[256];
  snprintf(buf, sizeof buf, fmt, a...);
  return refuse(rc, buf);
}
inline bool known_material(const unsigned char *group) {
  GroupParams g;
  memcpy(&g, group, sizeof g);
  return g.type >= MPMHIP_VISCO && g.type <= MPMHIP_ELASTIC;
}
template <class T>
inline T read_at(const unsigned char *blob, uint64_t off) {
  T v;
  memcpy(&v, blob + off, sizeof v);
  return v;
}

// what the context contributes to a check (each format reads its own part)
struct Facts {
  int32_t res[3] = {0, 0, 0};
  float dx = 0, dt = 0;
  int64_t capacity = 0;      // 3D: particle slots allocated
  int64_t groups_cap = 0;
  int64_t n_bodies = 0;      // entries of the scene's body table (the background body 0 counts), 0 = no rigid bodies
  int32_t nb[3] = {0, 0, 0};  // scheduler blocks per axis
  int64_t nblk = 0;
  float unit_delta_t = 0;
  bool resident = false;     // an asynchronous stepper is resident
  uint64_t n_boundary = 0;   // 2D: boundary particles of the scene's bodies
};

// ------------------------------------------------------------------------------------------------ 3D, synchronous ("MPMHIP01")
struct Counts3D {
  uint64_t n_groups = 0, n_slots = 0;
  bool rigid = false, collide = false;
  uint64_t n_bodies = 0, n_joints = 0;
};
struct Layout3D {
  Sec header, groups, rg, rp, rb;           // always
  Sec rigid, bodies, joints, collide;       // length 0 where absent
  uint64_t base = 0, total = 0;             // end of rb; end of the last section
};
inline bool layout3d(const Counts3D &n, uint64_t limit, Layout3D &L) {
  Cursor c(limit);
  L = Layout3D();
  L.header = c.take(1, sizeof(SnapHeader));
  L.groups = c.take(n.n_groups, GROUP_BYTES);
  L.rg = c.take(n.n_slots, RECG_BYTES);
  L.rp = c.take(n.n_slots, RECP_BYTES);
  L.rb = c.take(n.n_slots, BROW_BYTES);
  L.base = c.at;
  if (n.rigid) {
    L.rigid = c.take(1, sizeof(SnapRigid));
    L.bodies = c.take(n.n_bodies, BODY3_BYTES);
    L.joints = c.take(n.n_joints, JOINT3_BYTES);
    if (n.collide) L.collide = c.take(1, sizeof(SnapRigidCollide));
  }
  L.total = c.at;
  return c.ok;
}
struct Blob3D {
  SnapHeader h;
  SnapRigid r;
  SnapRigidCollide k;
  bool has_rigid = false, has_collide = false;
  Layout3D L;
};
// an optional tail at `off`: there in full, not there (the blob ends, or goes on with bytes that are not its magic: trailing bytes
// are nobody's business), or cut short (what is left begins like the tail but does not hold all of it)
enum Tail { TAIL_ABSENT, TAIL_PRESENT, TAIL_CUT };
inline Tail tail_at(const unsigned char *blob, uint64_t size, uint64_t off, uint64_t section_bytes, const char *magic) {
  const uint64_t left = size - off;  // (off <= size: the sections before it fit)
  if (left == 0 || memcmp(blob + off, magic, left < 8 ? left : 8) != 0) return TAIL_ABSENT;
  return left >= section_bytes ? TAIL_PRESENT : TAIL_CUT;
}
inline Verdict check3d(const void *src, uint64_t size, const Facts &f, Blob3D &B) {
  const unsigned char *blob = static_cast<const unsigned char *>(src);
  B = Blob3D();
  SnapHeader &h = B.h;
  if (size < sizeof h) return refuse(MPMHIP_EINVAL, "snapshot is truncated");
  memcpy(&h, blob, sizeof h);
  if (memcmp(h.magic, "MPMHIP01", 8) != 0 || h.abi != MPMHIP_ABI_VERSION) return refuse(MPMHIP_EINVAL, "not a libmpmhip snapshot of this ABI version");
  for (int k = 0; k < 3; k++)
    if (h.res[k] != f.res[k]) return refuse(MPMHIP_EINVAL, "snapshot is of a %dx%dx%d grid", h.res[0], h.res[1], h.res[2]);
  if (h.dx != f.dx) return refuse(MPMHIP_EINVAL, "snapshot has delta_x = %g, the ctx %g", h.dx, f.dx);
  // the stored P2G affine matrices carry the factor -4 inv_dx dt of the saving ctx (and apic_b is recovered with it)
  if (h.dt != f.dt) return refuse(MPMHIP_EINVAL, "snapshot has base_delta_t = %g, the ctx %g", h.dt, f.dt);
  if (h.n_slots < 0 || h.n_slots > f.capacity)
    return refuse(MPMHIP_ECAPACITY, "snapshot holds %lld particle slots, capacity is %lld", (long long)h.n_slots, (long long)f.capacity);
  if ((int64_t)h.n_groups > f.groups_cap) return refuse(MPMHIP_ECAPACITY, "snapshot holds %u groups", h.n_groups);
  Counts3D n;
  n.n_groups = h.n_groups; n.n_slots = (uint64_t)h.n_slots;
  if (!layout3d(n, size, B.L)) return refuse(MPMHIP_EINVAL, "snapshot is truncated");
  // the rigid section: the scene must have added the same bodies (meshes, scripts) before it loads
  const bool rigid_here = f.n_bodies > 0;
  const Tail rigid = tail_at(blob, size, B.L.base, sizeof(SnapRigid), "MPMRIGID");
  if (rigid == TAIL_CUT) return refuse(MPMHIP_EINVAL, "snapshot is truncated");
  B.has_rigid = rigid == TAIL_PRESENT;
  if (B.has_rigid) {
    memcpy(&B.r, blob + B.L.base, sizeof B.r);
    n.rigid = true; n.n_bodies = B.r.n_bodies; n.n_joints = B.r.n_joints;
    if (B.r.sizeof_body != BODY3_BYTES || B.r.sizeof_joint != JOINT3_BYTES || B.r.n_joints > MAX_JOINTS3 || !layout3d(n, size, B.L))
      return refuse(MPMHIP_EINVAL, "snapshot: the rigid-body section is damaged or of another build");
    if (!rigid_here || (uint64_t)f.n_bodies != B.r.n_bodies)
      return refuse(MPMHIP_EINVAL, "snapshot holds %u rigid bodies: add the scene's bodies (same meshes, same order) before loading", B.r.n_bodies - 1);
    const Tail collide = tail_at(blob, size, B.L.total, sizeof(SnapRigidCollide), "MPMRRCOL");
    if (collide == TAIL_CUT) return refuse(MPMHIP_EINVAL, "snapshot is truncated");
    B.has_collide = collide == TAIL_PRESENT;
    if (B.has_collide) {
      n.collide = true;
      layout3d(n, size, B.L);  // (fits: tail_at has looked at these bytes)
      memcpy(&B.k, blob + B.L.collide.off, sizeof B.k);
    }
  } else if (rigid_here) {
    return refuse(MPMHIP_EINVAL, "snapshot holds no rigid bodies, this simulation has %d", (int)f.n_bodies - 1);
  }
  for (uint64_t i = 0; i < n.n_slots; i++) {  // (a deleted slot, pid < 0, keeps whatever it held)
    const uint64_t rec = B.L.rg.off + RECG_BYTES * i;
    const uint32_t gid = read_at<uint32_t>(blob, rec + RECG_GID);
    if (read_at<int32_t>(blob, rec + RECG_PID) >= 0 && gid >= h.n_groups)
      return refuse(MPMHIP_EINVAL, "snapshot record %zu refers to group %u of %u", (size_t)i, gid, h.n_groups);
  }
  // (live creation ids are NOT held against next_pid: a rank of a tiled run keeps the global ids of the particles that migrated
  // to it, which may lie above the ids it handed out itself)
  if (h.next_pid < 0) return refuse(MPMHIP_EINVAL, "snapshot header inconsistent with this ctx (next id %d)", h.next_pid);
  for (uint64_t g = 0; g < n.n_groups; g++)
    if (!known_material(blob + B.L.groups.off + GROUP_BYTES * g))
      return refuse(MPMHIP_EINVAL, "snapshot holds an unknown material id %d", read_at<GroupParams>(blob, B.L.groups.off + GROUP_BYTES * g).type);
  for (uint64_t j = 0; j < n.n_joints; j++) {  // the joints index the body table on the device (body 0 is the background)
    const uint64_t at = B.L.joints.off + JOINT3_BYTES * j;
    const int32_t o0 = read_at<int32_t>(blob, at + JOINT3_OBJ0), o1 = read_at<int32_t>(blob, at + JOINT3_OBJ1);
    if (o0 < 0 || o0 >= (int64_t)n.n_bodies || o1 < 0 || o1 >= (int64_t)n.n_bodies)
      return refuse(MPMHIP_EINVAL, "snapshot joint names a body outside the scene's table");
  }
  return Verdict();
}

// ------------------------------------------------------------------------------------------------ the container part
// tags, then lane after lane — 3D {id, g, w}, 2D {rec} — shared by the asynchronous 3D format and the asynchronous part of the 2D one
struct LayoutStore {
  Sec tables[N_TABLES];
  Sec tags, lane[3];
  int n_lanes = 0;
};
inline void layout_store(Cursor &c, int dim, uint64_t nblk, uint64_t containers, LayoutStore &S) {
  S = LayoutStore();
  for (Sec &t : S.tables) t = c.take(nblk, TABLE_WORD);
  S.tags = c.take(containers, TAG_BYTES);
  if (dim == 3) {
    S.n_lanes = 3;
    S.lane[0] = c.take(containers, ID_BYTES); S.lane[1] = c.take(containers, RECG_BYTES); S.lane[2] = c.take(containers, W3_BYTES);
  } else {
    S.n_lanes = 1;
    S.lane[0] = c.take(containers, REC2_BYTES);
  }
}
// ------------------------------------------------------------------------------------------------ 3D, asynchronous ("MPMASYNC")
struct LayoutAsync {
  Sec header, groups;
  LayoutStore store;  // lanes: ids, g, w
  uint64_t total = 0;
};
inline bool layout_async(uint64_t n_groups, uint64_t nblk, uint64_t containers, uint64_t limit, LayoutAsync &L) {
  Cursor c(limit);
  L.header = c.take(1, sizeof(SnapAsync));
  L.groups = c.take(n_groups, GROUP_BYTES);
  layout_store(c, 3, nblk, containers, L.store);
  L.total = c.at;
  return c.ok;
}
struct BlobAsync {
  SnapAsync h;
  LayoutAsync L;
};
inline Verdict check_async(const void *src, uint64_t size, const Facts &f, BlobAsync &B) {
  const unsigned char *blob = static_cast<const unsigned char *>(src);
  B = BlobAsync();
  SnapAsync &h = B.h;
  if (size < sizeof h) return refuse(MPMHIP_EINVAL, "snapshot size mismatch");
  memcpy(&h, blob, sizeof h);
  if (memcmp(h.magic, "MPMASYNC", 8) != 0 || h.abi != MPMHIP_ABI_VERSION) return refuse(MPMHIP_EINVAL, "not an asynchronous-stepper snapshot of this ABI version");
  for (int k = 0; k < 3; k++)
    if (h.res[k] != f.res[k] || h.nb[k] != f.nb[k]) return refuse(MPMHIP_EINVAL, "snapshot is of a %dx%dx%d grid", h.res[0], h.res[1], h.res[2]);
  if (h.dx != f.dx || h.unit_delta_t != f.unit_delta_t) return refuse(MPMHIP_EINVAL, "snapshot has delta_x = %g, unit_delta_t = %g", h.dx, h.unit_delta_t);
  if ((int64_t)h.n_groups > f.groups_cap || h.nblk != f.nblk || h.containers < 0) return refuse(MPMHIP_EINVAL, "snapshot header inconsistent with this ctx");
  if (!layout_async(h.n_groups, (uint64_t)h.nblk, (uint64_t)h.containers, size, B.L) || B.L.total != size) return refuse(MPMHIP_EINVAL, "snapshot size mismatch");
  // the container arrays index the block table (tag), the block order and the per-id bids (id) on the device: a truncated or
  // foreign blob must not get that far
  if (h.next_pid < 0) return refuse(MPMHIP_EINVAL, "snapshot header inconsistent with this ctx (next id %d)", h.next_pid);
  // the scheduler's limits (first of the six block tables): powers of two in [1, 2^31], or update_dt_limits cannot use them
  const LayoutStore &S = B.L.store;
  if (!mpm::AsyncSched::limits_are_sane(reinterpret_cast<const char *>(blob) + S.tables[0].off, (size_t)h.nblk))
    return refuse(MPMHIP_EINVAL, "snapshot block table holds a time-step limit that is not a power of two in [1, 2^31]");
  for (uint64_t i = 0; i < (uint64_t)h.containers; i++) {
    const uint32_t tag = read_at<uint32_t>(blob, S.tags.off + TAG_BYTES * i);
    if (tag == TAG_FREE) continue;
    const int32_t id = read_at<int32_t>(blob, S.lane[0].off + ID_BYTES * i);
    const uint32_t gid = read_at<uint32_t>(blob, S.lane[1].off + RECG_BYTES * i + RECG_GID);
    if (gid >= h.n_groups) return refuse(MPMHIP_EINVAL, "snapshot container %zu names group %u of %d", (size_t)i, gid, (int)h.n_groups);
    if ((int64_t)(tag & ~TAG_BACKUP) >= h.nblk) return refuse(MPMHIP_EINVAL, "snapshot container %zu names block %u of %lld", (size_t)i, tag & ~TAG_BACKUP, (long long)h.nblk);
    if (id < 0 || id >= h.next_pid) return refuse(MPMHIP_EINVAL, "snapshot container %zu has id %d outside [0, %d)", (size_t)i, id, h.next_pid);
  }
  for (uint64_t g = 0; g < h.n_groups; g++)
    if (!known_material(blob + B.L.groups.off + GROUP_BYTES * g))
      return refuse(MPMHIP_EINVAL, "snapshot holds an unknown material id %d", read_at<GroupParams>(blob, B.L.groups.off + GROUP_BYTES * g).type);
  return Verdict();
}

// ------------------------------------------------------------------------------------------------ 2D ("MPM2DSNP")
struct Counts2D {
  uint64_t n_groups = 0, n = 0;
  uint64_t n_bodies = 0, n_ranked = 0;  // n_bodies > 0: bodies, the joint table, ranks and colours follow the particles
  bool has_async = false;
  uint64_t nblk = 0, containers = 0;
};
struct Layout2D {
  Sec header, groups, arr[P2_ARRAYS];
  Sec bodies, joints, ranks, colours;  // length 0 without rigid bodies
  LayoutStore store;                   // lane: rec; all empty without a stepper
  uint64_t total = 0;
};
inline bool layout2d(const Counts2D &n, uint64_t limit, Layout2D &L) {
  Cursor c(limit);
  L = Layout2D();
  L.header = c.take(1, sizeof(Snap2D));
  L.groups = c.take(n.n_groups, GROUP_BYTES);
  for (int a = 0; a < P2_ARRAYS; a++) L.arr[a] = c.take(n.n, P2_BYTES[a]);
  if (n.n_bodies) {
    L.bodies = c.take(n.n_bodies, BODY2_BYTES);
    L.joints = c.take(1, JOINTS2_BYTES);
    L.ranks = c.take(n.n_ranked, RANK_BYTES);
    L.colours = c.take(n.n, COLOUR_BYTES);  // MPMParticle::states, the sticky history of which side of a body a particle is on
  }
  if (n.has_async) layout_store(c, 2, n.nblk, n.containers, L.store);
  L.total = c.at;
  return c.ok;
}
struct Blob2D {
  Snap2D h;
  Layout2D L;
};
inline Verdict check2d(const void *src, uint64_t size, const Facts &f, Blob2D &B) {
  const unsigned char *blob = static_cast<const unsigned char *>(src);
  B = Blob2D();
  Snap2D &h = B.h;
  if (size < sizeof h) return refuse(MPMHIP_EINVAL, "snapshot size mismatch");
  memcpy(&h, blob, sizeof h);
  if (memcmp(h.magic, "MPM2DSNP", 8) != 0 || h.abi != MPMHIP_ABI_VERSION) return refuse(MPMHIP_EINVAL, "not a 2D snapshot of this ABI version");
  if (h.res[0] != f.res[0] || h.res[1] != f.res[1] || h.dx != f.dx) return refuse(MPMHIP_EINVAL, "snapshot is of another grid");
  if (h.n < 0 || h.next_pid < 0 || h.n_groups > (uint32_t)MPMHIP_MAX_GROUPS || h.n_joints < 0 || h.n_joints > MAX_JOINTS2 || h.containers < 0 || h.nblk < 0)
    return refuse(MPMHIP_EINVAL, "snapshot header inconsistent");
  if (h.n_bodies != f.n_bodies) return refuse(MPMHIP_EINVAL, "snapshot has another number of rigid bodies than the scene: add the scene's bodies before loading");
  if ((h.has_async != 0) != f.resident) return refuse(MPMHIP_EINVAL, "snapshot and simulation differ in being asynchronous steppers");
  if (h.has_async && (h.nb[0] != f.nb[0] || h.nb[1] != f.nb[1] || h.nblk != f.nblk || h.unit_delta_t != f.unit_delta_t))
    return refuse(MPMHIP_EINVAL, "snapshot is of another block table / unit_delta_t");
  if (h.n_bodies && h.n_ranked > f.n_boundary) return refuse(MPMHIP_EINVAL, "snapshot holds more boundary particles than the scene's bodies have");
  Counts2D n;
  n.n_groups = h.n_groups; n.n = (uint64_t)h.n; n.n_bodies = (uint64_t)h.n_bodies; n.n_ranked = h.n_ranked;
  n.has_async = h.has_async != 0; n.nblk = (uint64_t)h.nblk; n.containers = (uint64_t)h.containers;
  if (!layout2d(n, size, B.L) || B.L.total != size) return refuse(MPMHIP_EINVAL, "snapshot size mismatch");
  const Layout2D &L = B.L;
  // ---- everything that indexes device tables
  for (uint64_t g = 0; g < n.n_groups; g++)
    if (!known_material(blob + L.groups.off + GROUP_BYTES * g)) return refuse(MPMHIP_EINVAL, "snapshot holds an unknown material id");
  for (uint64_t i = 0; i < n.n; i++) {  // (a deleted particle has id < 0)
    const int32_t g = read_at<int32_t>(blob, L.arr[P2_GID].off + P2_BYTES[P2_GID] * i), id = read_at<int32_t>(blob, L.arr[P2_PID].off + P2_BYTES[P2_PID] * i);
    if (g < 0 || (uint32_t)g >= h.n_groups || id >= h.next_pid) return refuse(MPMHIP_EINVAL, "snapshot particle names an unknown group or id");
  }
  if (n.n_bodies) {  // the joints index the body table on the device (k2_articulate)
    const int32_t nj = read_at<int32_t>(blob, L.joints.off + JOINTS2_N);
    if (nj < 0 || nj > MAX_JOINTS2) return refuse(MPMHIP_EINVAL, "snapshot joint table inconsistent");
    for (int32_t j = 0; j < nj; j++) {
      const uint64_t at = L.joints.off + JOINTS2_FIRST + JOINT2_BYTES * (uint64_t)j;
      const int32_t o0 = read_at<int32_t>(blob, at + JOINT2_OBJ0), o1 = read_at<int32_t>(blob, at + JOINT2_OBJ1);
      if (o0 < 0 || o0 >= h.n_bodies || o1 < 0 || o1 >= h.n_bodies) return refuse(MPMHIP_EINVAL, "snapshot joint names a body outside the scene's table");
    }
  }
  if (n.has_async) {
    const LayoutStore &S = L.store;
    if (!mpm::AsyncSched::limits_are_sane(reinterpret_cast<const char *>(blob) + S.tables[0].off, (size_t)n.nblk))
      return refuse(MPMHIP_EINVAL, "snapshot block table holds a time-step limit that is not a power of two in [1, 2^31]");
    for (uint64_t i = 0; i < n.containers; i++) {
      const uint32_t tag = read_at<uint32_t>(blob, S.tags.off + TAG_BYTES * i);
      if (tag == TAG_FREE) continue;
      if ((int64_t)(tag & ~TAG_BACKUP) >= h.nblk) return refuse(MPMHIP_EINVAL, "snapshot container names an unknown block");
      const uint64_t rec = S.lane[0].off + REC2_BYTES * i;
      const int32_t g = read_at<int32_t>(blob, rec + REC2_GID), id = read_at<int32_t>(blob, rec + REC2_ID);
      if (g < 0 || (uint32_t)g >= h.n_groups || id < 0 || id >= h.next_pid) return refuse(MPMHIP_EINVAL, "snapshot container names an unknown group or id");
    }
  }
  return Verdict();
}

// ------------------------------------------------------------------------------------------------ a 3D blob loaded brick by brick
// mpmhip_snapshot_load_brick / mpmhip_snapshot_histogram (snapshot_job_api.h): check3d with two differences.  The blob's slot count
// is not held against the ctx's capacity — a rank keeps the records of its own brick, counted on the device — but against 2^31 - 1,
// what the kernels index with 32 bits; and a blob with a rigid section is refused whatever f.n_bodies says (a tiled ctx has no
// rigid bodies).  Everything else is check3d's own verdict.
constexpr int64_t BRICK_MAX_SLOTS = 0x7fffffffll;
inline Verdict check3d_brick(const void *src, uint64_t size, const Facts &f, Blob3D &B) {
  Facts g = f;
  g.capacity = BRICK_MAX_SLOTS;
  g.n_bodies = 0;
  const Verdict v = check3d(src, size, g, B);
  if (!v.ok() && B.has_rigid) return refuse(MPMHIP_EINVAL, "snapshot holds %u rigid bodies: a tiled job loads no rigid-body snapshot", B.r.n_bodies ? B.r.n_bodies - 1 : 0u);
  return v;
}

}  // namespace snap
