// tests/cpp/snapshot_job_host.cpp — snap::check3d_brick (taichi_mpm_amd/csrc/snapshot_blob.h) on the host, header only: the check a
// rank of a tiled job runs before it loads its brick of a blob (mpmhip_snapshot_load_brick).  It is check3d with the slot count held
// against 2^31 - 1 in the place of the ctx's capacity, and a rigid section refused whatever the ctx holds.  Blobs live in heap buffers
// of exactly their size, so that AddressSanitizer sees any read behind one.  Every scenario returns 0 or the line of the first check
// that failed; main() runs them all (tests/test_snapshot_job_cpu.py builds this with -fsanitize=address,undefined and runs it).
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
  Bytes(const Bytes &o, uint64_t len) : p(new unsigned char[len ? len : 1]), n(len) {
    memset(p.get(), 0, len ? len : 1);
    memcpy(p.get(), o.p.get(), len < o.n ? len : o.n);
  }
  template <class T> void put(uint64_t off, const T &v) { memcpy(p.get() + off, &v, sizeof v); }
  template <class T> Bytes with(uint64_t off, const T &v) const { Bytes b(*this, n); b.put(off, v); return b; }
};
Facts facts(int64_t capacity) {
  Facts f;
  f.res[0] = 16; f.res[1] = 16; f.res[2] = 32; f.dx = 1.0f / 16; f.dt = 1e-4f; f.capacity = capacity; f.groups_cap = 64;
  return f;
}
// 2 groups, 5 slots of which one dead; with `rigid` the section of two bodies and one joint behind them
Bytes blob(bool rigid, Layout3D &L) {
  Counts3D n;
  n.n_groups = 2; n.n_slots = 5; n.rigid = n.collide = rigid; n.n_bodies = 2; n.n_joints = 1;
  layout3d(n, NO_LIMIT, L);
  Bytes b(L.total);
  SnapHeader h;
  memset(&h, 0, sizeof h);
  memcpy(h.magic, "MPMHIP01", 8);
  h.abi = MPMHIP_ABI_VERSION; h.n_groups = 2; h.n_slots = 5; h.substeps = 7; h.next_pid = 9; h.store_b = 1;
  h.res[0] = 16; h.res[1] = 16; h.res[2] = 32; h.dx = 1.0f / 16; h.dt = 1e-4f; h.n_dead = 1;
  b.put(L.header.off, h);
  GroupParams g;
  memset(&g, 0, sizeof g);
  g.p[0] = 1.0f;
  g.type = MPMHIP_SAND; b.put(L.groups.off, g);
  g.type = MPMHIP_ELASTIC; b.put(L.groups.off + sizeof g, g);
  const uint32_t gid[5] = {0, 77, 1, 1, 0};  // (the dead slot keeps a stale group id)
  const int32_t pid[5] = {8, -1, 4, 0, 2};
  for (int i = 0; i < 5; i++) { b.put(L.rg.off + 64 * i + RECG_GID, gid[i]); b.put(L.rg.off + 64 * i + RECG_PID, pid[i]); }
  if (rigid) {
    SnapRigid r;
    memcpy(r.magic, "MPMRIGID", 8);
    r.n_bodies = 2; r.n_joints = 1; r.sizeof_body = (uint32_t)BODY3_BYTES; r.sizeof_joint = (uint32_t)JOINT3_BYTES;
    b.put(L.rigid.off, r);
    b.put<int32_t>(L.joints.off + JOINT3_OBJ0, 1);
    SnapRigidCollide k;
    memset(&k, 0, sizeof k);
    memcpy(k.magic, "MPMRRCOL", 8);
    b.put(L.collide.off, k);
  }
  return b;
}
}  // namespace

extern "C" {

// a blob of more slots than the ctx holds: check3d refuses for capacity, check3d_brick accepts with the same layout
int sj_capacity_is_not_the_blobs() {
  Layout3D L;
  const Bytes b = blob(false, L);
  Blob3D A, B;
  CHECK(check3d(b.p.get(), b.n, facts(2), A).rc == MPMHIP_ECAPACITY);
  const Verdict v = check3d_brick(b.p.get(), b.n, facts(2), B);
  CHECK(v.ok());
  CHECK(B.h.n_slots == 5 && B.h.n_dead == 1 && B.h.next_pid == 9 && !B.has_rigid);
  CHECK(B.L.rg.off == L.rg.off && B.L.rp.off == L.rp.off && B.L.rb.off == L.rb.off && B.L.rb.len == 5 * BROW_BYTES && B.L.total == L.total);
  CHECK(check3d(b.p.get(), b.n, facts(5), A).ok() && A.L.total == B.L.total);  // ... and where check3d accepts, both agree
  CHECK(check3d_brick(b.p.get(), b.n, facts(0), B).ok());
  return 0;
}
// a rigid section is refused, with or without bodies in the ctx
int sj_rigid_is_refused() {
  Layout3D L;
  const Bytes b = blob(true, L);
  for (int bodies = 0; bodies <= 2; bodies += 2) {
    Facts f = facts(8);
    f.n_bodies = bodies;
    Blob3D B;
    const Verdict v = check3d_brick(b.p.get(), b.n, f, B);
    CHECK(v.rc == MPMHIP_EINVAL && v.msg.find("rigid") != std::string::npos);
  }
  Facts f = facts(8);
  f.n_bodies = 2;
  Blob3D A;
  CHECK(check3d(b.p.get(), b.n, f, A).ok());  // (check3d itself keeps accepting it on a ctx with the bodies)
  return 0;
}
// every shorter length is refused, and no length leads to a read behind the buffer (AddressSanitizer)
int sj_truncation() {
  Layout3D L;
  const Bytes b = blob(false, L);
  for (uint64_t len = 0; len < b.n; len++) {
    const Bytes cut(b, len);
    Blob3D B;
    const Verdict v = check3d_brick(cut.p.get(), cut.n, facts(8), B);
    CHECK(v.rc == MPMHIP_EINVAL && v.msg.find("truncated") != std::string::npos);
  }
  return 0;
}
// what check3d refuses, check3d_brick refuses with the same code
int sj_the_rest_is_check3d() {
  Layout3D L;
  const Bytes b = blob(false, L);
  Blob3D B;
  Facts f = facts(8);
  f.res[2] = 16;
  CHECK(check3d_brick(b.p.get(), b.n, f, B).rc == MPMHIP_EINVAL);
  f = facts(8); f.dx = 1.0f / 32;
  CHECK(check3d_brick(b.p.get(), b.n, f, B).rc == MPMHIP_EINVAL);
  f = facts(8); f.dt = 2e-4f;
  CHECK(check3d_brick(b.p.get(), b.n, f, B).rc == MPMHIP_EINVAL);
  f = facts(8); f.groups_cap = 1;
  CHECK(check3d_brick(b.p.get(), b.n, f, B).rc == MPMHIP_ECAPACITY);
  f = facts(8);
  CHECK(check3d_brick(b.with<uint32_t>(8, MPMHIP_ABI_VERSION + 1).p.get(), b.n, f, B).rc == MPMHIP_EINVAL);
  CHECK(check3d_brick(b.with<int64_t>(16, -1).p.get(), b.n, f, B).rc == MPMHIP_ECAPACITY);
  CHECK(check3d_brick(b.with<int64_t>(16, BRICK_MAX_SLOTS + 1).p.get(), b.n, f, B).rc == MPMHIP_ECAPACITY);
  CHECK(check3d_brick(b.with<int64_t>(16, BRICK_MAX_SLOTS).p.get(), b.n, f, B).rc == MPMHIP_EINVAL);  // (fits 32 bits, not the blob)
  CHECK(check3d_brick(b.with<int64_t>(16, 6).p.get(), b.n, f, B).rc == MPMHIP_EINVAL);
  CHECK(check3d_brick(b.with<int32_t>(32, -1).p.get(), b.n, f, B).rc == MPMHIP_EINVAL);  // next_pid
  CHECK(check3d_brick(b.with<uint32_t>(L.rg.off + 64 * 2 + RECG_GID, 2).p.get(), b.n, f, B).rc == MPMHIP_EINVAL);  // a live slot's group
  CHECK(check3d_brick(b.with<uint32_t>(L.rg.off + 64 * 1 + RECG_GID, 99).p.get(), b.n, f, B).ok());                 // a dead slot's
  CHECK(check3d_brick(b.with<int32_t>(L.groups.off + 64, 99).p.get(), b.n, f, B).rc == MPMHIP_EINVAL);              // an unknown material
  return 0;
}

}  // extern "C"

int main() {
  struct { const char *name; int (*fn)(); } all[] = {{"sj_capacity_is_not_the_blobs", sj_capacity_is_not_the_blobs}, {"sj_rigid_is_refused", sj_rigid_is_refused},
                                                     {"sj_truncation", sj_truncation}, {"sj_the_rest_is_check3d", sj_the_rest_is_check3d}};
  int bad = 0;
  for (auto &s : all) {
    const int line = s.fn();
    if (line) { printf("%s failed at line %d\n", s.name, line); bad++; }
  }
  if (!bad) printf("scenarios ok\n");
  return bad ? 1 : 0;
}
