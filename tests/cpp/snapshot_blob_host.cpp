// tests/cpp/snapshot_blob_host.cpp — taichi_mpm_amd/csrc/snapshot_blob.h on the host, header only: the layout and the check function
// of the three snapshot formats on the smallest blobs that have every section.  Blobs live in heap buffers of exactly their size,
// so that AddressSanitizer sees any read behind one.  The offsets of the first scenario are written out by hand from the formulas
// the three formats had before the header existed; nothing there is computed from the header's constants.  Every scenario returns
// 0 or the line of the first check that failed; tests/test_snapshot_blob_cpu.py runs them through ctypes, and main() runs them all
// as a program of its own (built with -fsanitize=address,undefined).
#include "../../taichi_mpm_amd/csrc/snapshot_blob.h"

#include <cstdio>
#include <cstdlib>
#include <memory>

#define CHECK(cond) do { if (!(cond)) return __LINE__; } while (0)

using namespace snap;

namespace {
struct Bytes {  // a heap buffer of exactly n bytes
  std::unique_ptr<unsigned char[]> p;
  uint64_t n = 0;
  explicit Bytes(uint64_t n_) : p(new unsigned char[n_ ? n_ : 1]), n(n_) { memset(p.get(), 0, n_ ? n_ : 1); }
  Bytes(const Bytes &o, uint64_t len) : p(new unsigned char[len ? len : 1]), n(len) { memcpy(p.get(), o.p.get(), len < o.n ? len : o.n); }
  template <class T> void put(uint64_t off, const T &v) { memcpy(p.get() + off, &v, sizeof v); }
  template <class T> Bytes with(uint64_t off, const T &v) const { Bytes b(*this, n); b.put(off, v); return b; }
};
void put_groups(Bytes &b, Sec s) {
  GroupParams g;
  memset(&g, 0, sizeof g);
  g.p[0] = 1.0f; g.p[1] = 1.0f;
  g.type = MPMHIP_SAND; b.put(s.off, g);
  g.type = MPMHIP_ELASTIC; b.put(s.off + sizeof g, g);
}
void put_tables(Bytes &b, const LayoutStore &S, int nblk) {
  for (int t = 0; t < N_TABLES; t++)
    for (int k = 0; k < nblk; k++) b.put<int64_t>(S.tables[t].off + 8 * k, t == 0 ? (int64_t)1 << k : 1);
}

// ---- 3D: 2 groups, 3 slots of which one dead, 2 bodies (the background and one), 1 joint, the collision tail
Facts facts3d() {
  Facts f;
  f.res[0] = 16; f.res[1] = 16; f.res[2] = 32; f.dx = 1.0f / 16; f.dt = 1e-4f; f.capacity = 8; f.groups_cap = 64; f.n_bodies = 2;
  return f;
}
Facts facts3d_no_bodies() { Facts f = facts3d(); f.n_bodies = 0; return f; }
Bytes blob3d(Layout3D &L) {
  Counts3D n;
  n.n_groups = 2; n.n_slots = 3; n.rigid = n.collide = true; n.n_bodies = 2; n.n_joints = 1;
  layout3d(n, NO_LIMIT, L);
  Bytes b(L.total);
  SnapHeader h;
  memset(&h, 0, sizeof h);
  memcpy(h.magic, "MPMHIP01", 8);
  h.abi = MPMHIP_ABI_VERSION; h.n_groups = 2; h.n_slots = 3; h.substeps = 7; h.next_pid = 5; h.store_b = 1;
  h.res[0] = 16; h.res[1] = 16; h.res[2] = 32; h.dx = 1.0f / 16; h.dt = 1e-4f; h.n_dead = 1;
  b.put(L.header.off, h);
  put_groups(b, L.groups);
  const uint32_t gid[3] = {0, 77, 1};  // (the dead slot keeps a stale group id: nobody looks at it)
  const int32_t pid[3] = {0, -1, 4};
  for (int i = 0; i < 3; i++) { b.put(L.rg.off + 64 * i + 52, gid[i]); b.put(L.rg.off + 64 * i + 56, pid[i]); }
  SnapRigid r;
  memcpy(r.magic, "MPMRIGID", 8);
  r.n_bodies = 2; r.n_joints = 1; r.sizeof_body = 188; r.sizeof_joint = 168;
  b.put(L.rigid.off, r);
  b.put<int32_t>(L.joints.off + 4, 1); b.put<int32_t>(L.joints.off + 8, 0);  // obj0 = the body, obj1 = the background
  SnapRigidCollide k;
  memcpy(k.magic, "MPMRRCOL", 8);
  k.on = 1; k.iterations = 3; k.position_iterations = 1; k.penalty = 2e3f;
  b.put(L.collide.off, k);
  return b;
}

// ---- asynchronous 3D: 2 groups, 4 blocks, 5 containers of which one free and one backup
Facts facts_async() {
  Facts f;
  f.res[0] = 4; f.res[1] = 4; f.res[2] = 4; f.nb[0] = 2; f.nb[1] = 2; f.nb[2] = 1; f.dx = 0.25f; f.unit_delta_t = 2e-6f; f.groups_cap = 64; f.nblk = 4;
  return f;
}
Bytes blob_async(LayoutAsync &L) {
  layout_async(2, 4, 5, NO_LIMIT, L);
  Bytes b(L.total);
  SnapAsync h;
  memset(&h, 0, sizeof h);
  memcpy(h.magic, "MPMASYNC", 8);
  h.abi = MPMHIP_ABI_VERSION; h.n_groups = 2;
  for (int k = 0; k < 3; k++) { h.res[k] = 4; h.nb[k] = k < 2 ? 2 : 1; }
  h.dx = 0.25f; h.unit_delta_t = 2e-6f; h.nblk = 4; h.containers = 5; h.current_t_int = 8; h.min_delta_t_int = 1; h.max_delta_t_int = 8; h.next_pid = 4;
  b.put(L.header.off, h);
  put_groups(b, L.groups);
  put_tables(b, L.store, 4);
  const uint32_t tag[5] = {0, 3, 0xFFFFFFFFu, 0x80000000u | 2u, 1};
  const int32_t id[5] = {0, 1, -9, 1, 3};
  const uint32_t gid[5] = {0, 1, 99, 1, 0};  // (the free container keeps stale words)
  for (int i = 0; i < 5; i++) {
    b.put(L.store.tags.off + 4 * i, tag[i]); b.put(L.store.lane[0].off + 4 * i, id[i]); b.put(L.store.lane[1].off + 64 * i + 52, gid[i]);
  }
  return b;
}

// ---- 2D: 2 groups, 3 particles, 1 body, 1 joint, 2 ranked boundary particles, the stepper's part with 4 blocks and 3 containers
Facts facts2d() {
  Facts f;
  f.res[0] = 32; f.res[1] = 32; f.dx = 1.0f / 32; f.n_bodies = 1; f.resident = true; f.nb[0] = 2; f.nb[1] = 2; f.nblk = 4; f.unit_delta_t = 2e-6f;
  f.n_boundary = 6;
  return f;
}
Bytes blob2d(Layout2D &L) {
  Counts2D n;
  n.n_groups = 2; n.n = 3; n.n_bodies = 1; n.n_ranked = 2; n.has_async = true; n.nblk = 4; n.containers = 3;
  layout2d(n, NO_LIMIT, L);
  Bytes b(L.total);
  Snap2D h;
  memset(&h, 0, sizeof h);
  memcpy(h.magic, "MPM2DSNP", 8);
  h.abi = MPMHIP_ABI_VERSION; h.n_groups = 2; h.res[0] = 32; h.res[1] = 32; h.next_pid = 9; h.n_bodies = 1; h.n_joints = 1; h.has_async = 1;
  h.n = 3; h.dx = 1.0f / 32; h.base_dt = 1e-4f; h.n_dead = 1; h.n_ranked = 2; h.nb[0] = 2; h.nb[1] = 2; h.unit_delta_t = 2e-6f;
  h.nblk = 4; h.containers = 3; h.min_delta_t_int = 1; h.max_delta_t_int = 8;
  b.put(L.header.off, h);
  put_groups(b, L.groups);
  const int32_t gid[3] = {1, 0, 0}, pid[3] = {8, -1, 2};
  for (int i = 0; i < 3; i++) { b.put(L.arr[P2_GID].off + 4 * i, gid[i]); b.put(L.arr[P2_PID].off + 4 * i, pid[i]); }
  b.put<int32_t>(L.joints.off, 1);  // one joint, body 0 to body 0
  put_tables(b, L.store, 4);
  const uint32_t tag[3] = {2, 0x80000000u | 3u, 0xFFFFFFFFu};
  const int32_t cg[3] = {0, 1, -4}, cid[3] = {5, 5, 1000};
  for (int i = 0; i < 3; i++) {
    b.put(L.store.tags.off + 4 * i, tag[i]); b.put(L.store.lane[0].off + 64 * i + 52, cg[i]); b.put(L.store.lane[0].off + 64 * i + 56, cid[i]);
  }
  return b;
}

Verdict run3d(const Bytes &b, const Facts &f) { Blob3D B; return check3d(b.p.get(), b.n, f, B); }
Verdict run_async(const Bytes &b, const Facts &f) { BlobAsync B; return check_async(b.p.get(), b.n, f, B); }
Verdict run2d(const Bytes &b, const Facts &f) { Blob2D B; return check2d(b.p.get(), b.n, f, B); }
bool refused(const Verdict &v, const char *text, int rc = MPMHIP_EINVAL) { return v.rc == rc && v.msg.find(text) != std::string::npos; }
bool sec(Sec s, uint64_t off, uint64_t len) { return s.off == off && s.len == len; }
}  // namespace

extern "C" {
// every section of the three blobs at the place the formats always had it
int sb_offsets() {
  Layout3D A;
  blob3d(A);
  // 80 | 2 x 80 | 3 x 64 | 3 x 64 | 3 x 48 | 24 | 2 x 188 | 1 x 168 | 24
  CHECK(sec(A.header, 0, 80) && sec(A.groups, 80, 160) && sec(A.rg, 240, 192) && sec(A.rp, 432, 192) && sec(A.rb, 624, 144));
  CHECK(A.base == 768 && sec(A.rigid, 768, 24) && sec(A.bodies, 792, 376) && sec(A.joints, 1168, 168) && sec(A.collide, 1336, 24) && A.total == 1360);
  LayoutAsync B;
  blob_async(B);
  // 120 | 2 x 80 | 6 x 4 x 8 | 5 x 4 | 5 x 4 | 5 x 64 | 5 x 64  (= 120 + 160 + 192 + 5 x 136)
  CHECK(sec(B.header, 0, 120) && sec(B.groups, 120, 160));
  for (int t = 0; t < 6; t++) CHECK(sec(B.store.tables[t], 280 + 32 * t, 32));
  CHECK(sec(B.store.tags, 472, 20) && B.store.n_lanes == 3 && sec(B.store.lane[0], 492, 20) && sec(B.store.lane[1], 512, 320) && sec(B.store.lane[2], 832, 320));
  CHECK(B.total == 1152);
  Layout2D C;
  blob2d(C);
  // 152 | 2 x 80 | 3 x (8 + 8 + 16 + 16 + 4 + 4 + 4) | 68 | 260 | 2 x 4 | 3 x 4 | 6 x 4 x 8 | 3 x 4 | 3 x 64
  CHECK(sec(C.header, 0, 152) && sec(C.groups, 152, 160) && sec(C.arr[0], 312, 24) && sec(C.arr[1], 336, 24) && sec(C.arr[2], 360, 48) && sec(C.arr[3], 408, 48));
  CHECK(sec(C.arr[4], 456, 12) && sec(C.arr[5], 468, 12) && sec(C.arr[6], 480, 12));
  CHECK(sec(C.bodies, 492, 68) && sec(C.joints, 560, 260) && sec(C.ranks, 820, 8) && sec(C.colours, 828, 12));
  for (int t = 0; t < 6; t++) CHECK(sec(C.store.tables[t], 840 + 32 * t, 32));
  CHECK(sec(C.store.tags, 1032, 12) && C.store.n_lanes == 1 && sec(C.store.lane[0], 1044, 192) && C.total == 1236);
  // without the optional parts: a 3D blob of no bodies, a synchronous 2D blob of no bodies
  Counts3D n3;
  n3.n_groups = 1; n3.n_slots = 2;
  CHECK(layout3d(n3, NO_LIMIT, A) && A.total == 80 + 80 + 2 * 176 && A.base == A.total && A.rigid.len == 0 && A.collide.len == 0);
  Counts2D n2;
  n2.n_groups = 1; n2.n = 2;
  CHECK(layout2d(n2, NO_LIMIT, C) && C.total == 152 + 80 + 2 * 60 && C.bodies.len == 0 && C.joints.len == 0 && C.store.tags.len == 0);
  return 0;
}

// the three blobs pass, and so do the 3D variants a loader has always taken
int sb_accept() {
  Layout3D A;
  const Bytes a = blob3d(A);
  Blob3D R;
  CHECK(check3d(a.p.get(), a.n, facts3d(), R).ok());
  CHECK(R.has_rigid && R.has_collide && R.L.total == 1360 && R.L.joints.off == 1168 && R.r.n_joints == 1 && R.k.iterations == 3 && R.h.n_slots == 3);
  CHECK(check3d(Bytes(a, 1336).p.get(), 1336, facts3d(), R).ok() && R.has_rigid && !R.has_collide && R.L.total == 1336);  // no MPMRRCOL tail
  CHECK(check3d(Bytes(a, 768).p.get(), 768, facts3d_no_bodies(), R).ok() && !R.has_rigid && R.L.total == 768);            // no rigid section
  Bytes trailing(a, 1365);                                                                                                    // bytes behind the last section
  memset(trailing.p.get() + 1360, 0xEE, 5);
  CHECK(check3d(trailing.p.get(), trailing.n, facts3d(), R).ok() && R.L.total == 1360);
  Bytes trailing2(a, 1341);  // ... behind the joints, where no tail begins
  memset(trailing2.p.get() + 1336, 0xEE, 5);
  CHECK(check3d(trailing2.p.get(), trailing2.n, facts3d(), R).ok() && !R.has_collide);
  LayoutAsync B;
  const Bytes b = blob_async(B);
  CHECK(run_async(b, facts_async()).ok());
  Layout2D C;
  const Bytes c = blob2d(C);
  CHECK(run2d(c, facts2d()).ok());
  return 0;
}

// every shorter blob is refused — but for the two lengths of the 3D format that end exactly before an optional tail
int sb_truncation() {
  Layout3D A;
  const Bytes a = blob3d(A);
  for (uint64_t len = 0; len < a.n; len++) {
    const Bytes cut(a, len);
    const bool with_bodies = run3d(cut, facts3d()).ok(), without = run3d(cut, facts3d_no_bodies()).ok();
    CHECK(with_bodies == (len == 1336) && without == (len == 768));
  }
  LayoutAsync B;
  const Bytes b = blob_async(B);
  for (uint64_t len = 0; len < b.n; len++) CHECK(refused(run_async(Bytes(b, len), facts_async()), "size mismatch"));
  Layout2D C;
  const Bytes c = blob2d(C);
  for (uint64_t len = 0; len < c.n; len++) CHECK(refused(run2d(Bytes(c, len), facts2d()), "size mismatch"));
  Bytes longer(c, c.n + 1);
  CHECK(refused(run2d(longer, facts2d()), "size mismatch"));
  return 0;
}

int sb_corrupt_3d() {
  Layout3D L;
  const Bytes a = blob3d(L);
  const Facts f = facts3d();
  CHECK(refused(run3d(a.with<char>(3, 'X'), f), "not a libmpmhip snapshot"));
  CHECK(refused(run3d(a.with<uint32_t>(8, 2), f), "not a libmpmhip snapshot"));
  CHECK(refused(run3d(a.with<int32_t>(48, 17), f), "snapshot is of a 16x17x32 grid"));
  CHECK(refused(run3d(a.with<float>(64, 0.5f), f), "delta_x"));
  CHECK(refused(run3d(a.with<float>(68, 2e-4f), f), "base_delta_t"));
  CHECK(refused(run3d(a.with<int64_t>(16, -1), f), "particle slots", MPMHIP_ECAPACITY));
  CHECK(refused(run3d(a.with<int64_t>(16, (int64_t)1 << 61), f), "particle slots", MPMHIP_ECAPACITY));
  Facts roomy = f;
  roomy.capacity = INT64_MAX;  // (were the capacity no bound: the layout refuses what the blob cannot hold, before multiplying)
  CHECK(refused(run3d(a.with<int64_t>(16, (int64_t)1 << 61), roomy), "truncated"));
  CHECK(refused(run3d(a.with<int64_t>(16, 8), roomy), "truncated"));
  CHECK(refused(run3d(a.with<uint32_t>(12, 0xFFFFFFFFu), f), "snapshot holds 4294967295 groups", MPMHIP_ECAPACITY));
  roomy.groups_cap = INT64_MAX;
  CHECK(refused(run3d(a.with<uint32_t>(12, 0xFFFFFFFFu), roomy), "truncated"));
  CHECK(refused(run3d(a.with<uint32_t>(L.rg.off + 52, 2), f), "snapshot record 0 refers to group 2 of 2"));
  CHECK(run3d(a.with<uint32_t>(L.rg.off + 64 + 52, 5000), f).ok());  // (the dead slot)
  CHECK(refused(run3d(a.with<int32_t>(32, -1), f), "next id -1"));
  CHECK(run3d(a.with<int32_t>(L.rg.off + 56, 1000), f).ok());  // (a live id above next_pid: ranks of a tiled run hold migrated ones)
  CHECK(refused(run3d(a.with<int32_t>(L.groups.off + 80 + 64, 99), f), "unknown material id 99"));
  CHECK(refused(run3d(a.with<int32_t>(L.groups.off + 64, 0), f), "unknown material id 0"));
  CHECK(refused(run3d(a.with<int32_t>(L.joints.off + 4, 2), f), "joint names a body"));
  CHECK(refused(run3d(a.with<int32_t>(L.joints.off + 8, -1), f), "joint names a body"));
  CHECK(refused(run3d(a.with<int32_t>(L.joints.off + 8, 1000), f), "joint names a body"));
  CHECK(refused(run3d(a.with<uint32_t>(L.rigid.off + 8, 3), f), "rigid-body section is damaged"));    // a body more than the blob holds
  CHECK(refused(run3d(a.with<uint32_t>(L.rigid.off + 8, 0xFFFFFFFFu), f), "rigid-body section is damaged"));
  CHECK(refused(run3d(a.with<uint32_t>(L.rigid.off + 12, 33), f), "rigid-body section is damaged"));  // more joints than MAX_JOINTS
  CHECK(refused(run3d(a.with<uint32_t>(L.rigid.off + 16, 192), f), "rigid-body section is damaged"));
  Facts three = f;
  three.n_bodies = 3;
  CHECK(refused(run3d(a, three), "snapshot holds 1 rigid bodies"));
  CHECK(refused(run3d(a, facts3d_no_bodies()), "snapshot holds 1 rigid bodies"));
  CHECK(refused(run3d(Bytes(a, 768), f), "snapshot holds no rigid bodies, this simulation has 1"));
  return 0;
}

int sb_corrupt_async() {
  LayoutAsync L;
  const Bytes b = blob_async(L);
  const Facts f = facts_async();
  const LayoutStore &S = L.store;
  CHECK(refused(run_async(b.with<char>(0, 'X'), f), "not an asynchronous-stepper snapshot"));
  CHECK(refused(run_async(b.with<uint32_t>(8, 4), f), "not an asynchronous-stepper snapshot"));
  CHECK(refused(run_async(b.with<int32_t>(16, 8), f), "snapshot is of a 8x4x4 grid"));
  CHECK(refused(run_async(b.with<int32_t>(28, 3), f), "grid"));  // nb[0]
  CHECK(refused(run_async(b.with<float>(40, 0.5f), f), "delta_x"));
  CHECK(refused(run_async(b.with<float>(44, 1e-6f), f), "unit_delta_t"));
  CHECK(refused(run_async(b.with<int64_t>(56, -1), f), "header inconsistent"));
  CHECK(refused(run_async(b.with<int64_t>(56, (int64_t)1 << 62), f), "size mismatch"));
  CHECK(refused(run_async(b.with<int64_t>(56, 6), f), "size mismatch"));
  CHECK(refused(run_async(b.with<int64_t>(48, 5), f), "header inconsistent"));  // nblk
  CHECK(refused(run_async(b.with<uint32_t>(12, 0xFFFFFFFFu), f), "header inconsistent"));
  CHECK(refused(run_async(b.with<uint32_t>(12, 3), f), "size mismatch"));
  CHECK(refused(run_async(b.with<int32_t>(104, -2), f), "next id -2"));
  CHECK(refused(run_async(b.with<int64_t>(S.tables[0].off + 8, 3), f), "not a power of two"));
  CHECK(refused(run_async(b.with<int64_t>(S.tables[0].off, 0), f), "not a power of two"));
  CHECK(refused(run_async(b.with<int64_t>(S.tables[0].off + 24, (int64_t)1 << 32), f), "not a power of two"));
  CHECK(refused(run_async(b.with<uint32_t>(S.lane[1].off + 64 + 52, 2), f), "snapshot container 1 names group 2 of 2"));
  CHECK(refused(run_async(b.with<uint32_t>(S.tags.off, 4), f), "snapshot container 0 names block 4 of 4"));
  CHECK(refused(run_async(b.with<uint32_t>(S.tags.off + 12, 0x80000000u | 4u), f), "snapshot container 3 names block 4 of 4"));
  CHECK(refused(run_async(b.with<uint32_t>(S.tags.off, 0x7FFFFFF0u), f), "snapshot container"));
  CHECK(refused(run_async(b.with<int32_t>(S.lane[0].off + 16, 4), f), "snapshot container 4 has id 4 outside [0, 4)"));
  CHECK(refused(run_async(b.with<int32_t>(S.lane[0].off, -5), f), "snapshot container 0 has id -5"));
  CHECK(refused(run_async(b.with<int32_t>(L.groups.off + 64, 99), f), "unknown material id 99"));
  return 0;
}

int sb_corrupt_2d() {
  Layout2D L;
  const Bytes c = blob2d(L);
  const Facts f = facts2d();
  const LayoutStore &S = L.store;
  CHECK(refused(run2d(c.with<char>(7, 'X'), f), "not a 2D snapshot"));
  CHECK(refused(run2d(c.with<uint32_t>(8, 0), f), "not a 2D snapshot"));
  CHECK(refused(run2d(c.with<int32_t>(20, 64), f), "another grid"));
  CHECK(refused(run2d(c.with<float>(48, 0.5f), f), "another grid"));
  CHECK(refused(run2d(c.with<int64_t>(40, -3), f), "header inconsistent"));
  CHECK(refused(run2d(c.with<int32_t>(24, -1), f), "header inconsistent"));  // next_pid
  CHECK(refused(run2d(c.with<uint32_t>(12, 0xFFFFFFFFu), f), "header inconsistent"));
  CHECK(refused(run2d(c.with<int32_t>(32, 17), f), "header inconsistent"));  // n_joints
  CHECK(refused(run2d(c.with<int64_t>(104, -1), f), "header inconsistent"));  // containers
  CHECK(refused(run2d(c.with<int32_t>(28, 2), f), "another number of rigid bodies"));
  CHECK(refused(run2d(c.with<int32_t>(28, 0), f), "another number of rigid bodies"));
  CHECK(refused(run2d(c.with<int32_t>(36, 0), f), "differ in being asynchronous"));
  Facts sync = f;
  sync.resident = false;
  CHECK(refused(run2d(c, sync), "differ in being asynchronous"));
  CHECK(refused(run2d(c.with<int32_t>(72, 3), f), "another block table"));  // nb[0]
  CHECK(refused(run2d(c.with<float>(80, 1e-6f), f), "another block table"));
  CHECK(refused(run2d(c.with<int64_t>(96, 5), f), "another block table"));  // nblk
  CHECK(refused(run2d(c.with<uint32_t>(68, 7), f), "more boundary particles"));
  CHECK(refused(run2d(c.with<int64_t>(40, (int64_t)1 << 61), f), "size mismatch"));
  CHECK(refused(run2d(c.with<int64_t>(104, (int64_t)1 << 62), f), "size mismatch"));
  CHECK(refused(run2d(c.with<int64_t>(40, 4), f), "size mismatch"));
  CHECK(refused(run2d(c.with<uint32_t>(68, 3), f), "size mismatch"));  // n_ranked
  CHECK(refused(run2d(c.with<int32_t>(L.groups.off + 64, 9), f), "unknown material id"));
  CHECK(refused(run2d(c.with<int32_t>(L.arr[P2_GID].off, 2), f), "particle names an unknown group or id"));
  CHECK(refused(run2d(c.with<int32_t>(L.arr[P2_GID].off + 4, -1), f), "particle names an unknown group or id"));
  CHECK(refused(run2d(c.with<int32_t>(L.arr[P2_PID].off, 9), f), "particle names an unknown group or id"));
  CHECK(refused(run2d(c.with<int32_t>(L.joints.off, 17), f), "joint table inconsistent"));
  CHECK(refused(run2d(c.with<int32_t>(L.joints.off, -1), f), "joint table inconsistent"));
  CHECK(refused(run2d(c.with<int32_t>(L.joints.off + 4, 1), f), "joint names a body"));
  CHECK(refused(run2d(c.with<int32_t>(L.joints.off + 8, -1), f), "joint names a body"));
  CHECK(run2d(c.with<int32_t>(L.joints.off + 4 + 16, 1000), f).ok());  // (behind the joints in use)
  CHECK(refused(run2d(c.with<int64_t>(S.tables[0].off + 16, 6), f), "not a power of two"));
  CHECK(refused(run2d(c.with<uint32_t>(S.tags.off, 4), f), "container names an unknown block"));
  CHECK(refused(run2d(c.with<int32_t>(S.lane[0].off + 52, 2), f), "container names an unknown group or id"));
  CHECK(refused(run2d(c.with<int32_t>(S.lane[0].off + 64 + 56, 9), f), "container names an unknown group or id"));
  CHECK(refused(run2d(c.with<int32_t>(S.lane[0].off + 56, -1), f), "container names an unknown group or id"));
  return 0;
}

// every byte of every header at 0x00, 0x7F and 0xFF: accepted or refused, never a read outside the blob (the sanitized build's part)
int sb_sweep() {
  const unsigned char values[3] = {0x00, 0x7F, 0xFF};
  int accepted = 0;
  Layout3D A;
  const Bytes a = blob3d(A);
  const uint64_t heads3[3][2] = {{A.header.off, A.header.len}, {A.rigid.off, A.rigid.len}, {A.collide.off, A.collide.len}};
  for (const auto &hd : heads3)
    for (uint64_t i = 0; i < hd[1]; i++)
      for (unsigned char v : values) {
        accepted += run3d(a.with(hd[0] + i, v), facts3d()).ok();
        accepted += run3d(a.with(hd[0] + i, v), facts3d_no_bodies()).ok();
      }
  LayoutAsync B;
  const Bytes b = blob_async(B);
  for (uint64_t i = 0; i < B.header.len; i++)
    for (unsigned char v : values) accepted += run_async(b.with(i, v), facts_async()).ok();
  Layout2D C;
  const Bytes c = blob2d(C);
  Facts roomy = facts2d();
  roomy.n_boundary = ~0ull;
  for (uint64_t i = 0; i < C.header.len; i++)
    for (unsigned char v : values) {
      accepted += run2d(c.with(i, v), facts2d()).ok();
      accepted += run2d(c.with(i, v), roomy).ok();
    }
  CHECK(accepted > 0);  // (clocks, counters and padding may hold anything)
  return 0;
}

// the check of one format on a blob from outside (the fixtures saved by a GPU run): "" or the refusal.  kind: 0 the synchronous 3D
// format, 1 the asynchronous one, 2 the 2D one
const char *sb_check(int kind, const void *blob, uint64_t size, const Facts *f) {
  static std::string msg;
  Blob3D a;
  BlobAsync b;
  Blob2D c;
  msg = (kind == 0 ? check3d(blob, size, *f, a) : kind == 1 ? check_async(blob, size, *f, b) : check2d(blob, size, *f, c)).msg;
  return msg.c_str();
}
}

int main() {
  int (*const all[])() = {sb_offsets, sb_accept, sb_truncation, sb_corrupt_3d, sb_corrupt_async, sb_corrupt_2d, sb_sweep};
  const char *const names[] = {"sb_offsets", "sb_accept", "sb_truncation", "sb_corrupt_3d", "sb_corrupt_async", "sb_corrupt_2d", "sb_sweep"};
  int failed = 0;
  for (size_t i = 0; i < sizeof all / sizeof all[0]; i++)
    if (const int line = all[i]()) {
      std::printf("%s: check at line %d failed\n", names[i], line);
      failed = 1;
    }
  if (!failed) std::printf("snapshot_blob: %zu scenarios ok\n", sizeof all / sizeof all[0]);
  return failed;
}
