// tests/cpp/region_program_host.cpp — taichi_mpm_amd/csrc/region_program.h on the host, header only: the check every entry point
// that takes a region expression runs before anything is uploaded or launched.  Descriptions live in heap buffers of exactly their
// size, so that AddressSanitizer sees any read outside one; the phi pointers point at one float (the check may ask that an array is
// there, never read it).  Every scenario returns 0 or the line of the first check that failed; tests/test_region_program_cpu.py runs
// them through ctypes, and main() runs them all as a program of its own (built with -fsanitize=address,undefined).
#include "../../taichi_mpm_amd/csrc/region_program.h"

#include <cstdio>
#include <cstring>
#include <memory>

#define CHECK(cond) do { if (!(cond)) return __LINE__; } while (0)

namespace {

float g_one_sample = 0.0f;

struct Desc {  // a heap copy of exactly sizeof(mpmhip_region_desc) bytes
  std::unique_ptr<unsigned char[]> p;
  Desc() : p(new unsigned char[sizeof(mpmhip_region_desc)]) { memset(p.get(), 0, sizeof(mpmhip_region_desc)); }
  Desc(const Desc &o) : p(new unsigned char[sizeof(mpmhip_region_desc)]) { memcpy(p.get(), o.p.get(), sizeof(mpmhip_region_desc)); }
  mpmhip_region_desc *operator->() { return reinterpret_cast<mpmhip_region_desc *>(p.get()); }
  const mpmhip_region_desc *get() const { return reinterpret_cast<const mpmhip_region_desc *>(p.get()); }
};

void push(Desc &d, int leaf) { d->ops[d->n_ops].op = MPMHIP_REGION_PUSH; d->ops[d->n_ops++].leaf = leaf; }
void op(Desc &d, int code) { d->ops[d->n_ops++].op = code; }
mpmhip_region_leaf &ball(Desc &d, float r) {
  mpmhip_region_leaf &L = d->leaves[d->n_leaves++];
  L.kind = 0; L.shape.type = 1;
  L.shape.p[0] = L.shape.p[1] = L.shape.p[2] = 0.5f; L.shape.p[3] = r;
  return L;
}
int field(Desc &d, int res) {
  mpmhip_region_field &F = d->fields[d->n_fields];
  for (int k = 0; k < 3; k++) { F.res[k] = res; F.origin[k] = 0.25f; }
  F.spacing = 1.0f / 128;
  F.phi = &g_one_sample;
  return d->n_fields++;
}
mpmhip_region_leaf &sampled(Desc &d, int f) {
  mpmhip_region_leaf &L = d->leaves[d->n_leaves++];
  L.kind = 1; L.field = f;
  return L;
}
void place(mpmhip_region_leaf &L, float deg, float scale) {
  const float a = deg * 3.14159265358979f / 180.0f, c = std::cos(a), s = std::sin(a);
  const float R[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
  L.placed = 1;
  for (int k = 0; k < 9; k++) L.rot[k] = R[k];
  L.scale = scale;
  L.translate[0] = 0.7f; L.translate[1] = 0.56f; L.translate[2] = 0.47f;
  L.pivot[0] = L.pivot[1] = L.pivot[2] = 0.5f;
}

// the programs of the GPU tests
Desc prog_a() {  // sampled ball minus sampled ball on one lattice
  Desc d;
  const int f0 = field(d, 60), f1 = field(d, 60);
  sampled(d, f0); sampled(d, f1);
  push(d, 0); push(d, 1); op(d, MPMHIP_REGION_NEG); op(d, MPMHIP_REGION_INTERSECT);
  return d;
}
Desc prog_b() {  // one array, two leaves: plain, and placed
  Desc d;
  const int f = field(d, 60);
  sampled(d, f);
  place(sampled(d, f), 30.0f, 0.75f);
  push(d, 0); push(d, 1); op(d, MPMHIP_REGION_UNION);
  return d;
}
Desc prog_c() {  // (ball - ball) & half space
  Desc d;
  ball(d, 12.0f / 64); ball(d, 8.0f / 64);
  mpmhip_region_leaf &cut = d->leaves[d->n_leaves++];
  cut.shape.type = 0; cut.shape.p[1] = 1.0f; cut.shape.p[3] = -0.53125f;
  push(d, 0); push(d, 1); op(d, MPMHIP_REGION_NEG); op(d, MPMHIP_REGION_INTERSECT); push(d, 2); op(d, MPMHIP_REGION_INTERSECT);
  return d;
}
Desc prog_band() {  // the shell 0 < phi < 3 of a plane, in a box, with a placed ball's complement
  Desc d;
  mpmhip_region_leaf &g = d->leaves[d->n_leaves++];
  g.shape.type = 0; g.shape.p[1] = 1.0f; g.shape.p[3] = -0.3f;
  g.banded = 1; g.lo = 0.0f; g.hi = 3.0f;
  mpmhip_region_leaf &b = d->leaves[d->n_leaves++];
  b.shape.type = 2;
  for (int k = 0; k < 3; k++) { b.shape.p[k] = 0.25f; b.shape.p[3 + k] = 0.75f; }
  place(ball(d, 4.0f / 64), 45.0f, 1.5f);
  push(d, 0); push(d, 1); op(d, MPMHIP_REGION_INTERSECT); push(d, 2); op(d, MPMHIP_REGION_NEG); op(d, MPMHIP_REGION_INTERSECT);
  return d;
}
Desc prog_balanced8() {  // depth 4: ((0|1)&(2|3)) | ((4|5)&(6|7))
  Desc d;
  for (int i = 0; i < 8; i++) ball(d, (4.0f + i) / 64);
  for (int h = 0; h < 2; h++) {
    for (int q = 0; q < 2; q++) { push(d, 4 * h + 2 * q); push(d, 4 * h + 2 * q + 1); op(d, MPMHIP_REGION_UNION); }
    op(d, MPMHIP_REGION_INTERSECT);
  }
  op(d, MPMHIP_REGION_UNION);
  return d;
}

template <int D>
bool ok(const Desc &d, std::string *why = nullptr) {
  std::string w;
  const bool r = region_program::check<D>(d.get(), w);
  if (why) *why = w;
  return r;
}
template <int D>
bool refused(const Desc &d, const char *what) {
  std::string w;
  return !region_program::check<D>(d.get(), w) && w.find(what) != std::string::npos;
}

}  // namespace

extern "C" {

int rp_accept() {
  std::string why;
  CHECK(ok<3>(prog_a(), &why) && why.empty());
  CHECK(ok<3>(prog_b()) && ok<3>(prog_c()) && ok<3>(prog_band()) && ok<3>(prog_balanced8()));
  CHECK(ok<2>(prog_a()) && ok<2>(prog_b()) && ok<2>(prog_c()) && ok<2>(prog_band()) && ok<2>(prog_balanced8()));
  size_t counts[MPMHIP_REGION_MAX_FIELDS] = {};
  const Desc a = prog_a();
  CHECK(region_program::check<3>(a.get(), why, counts) && counts[0] == 216000 && counts[1] == 216000);
  CHECK(region_program::check<2>(a.get(), why, counts) && counts[0] == 3600);
  Desc full = prog_balanced8();  // the limits themselves pass: 24 operations with complements that cancel nothing
  while (full->n_ops < MPMHIP_REGION_MAX_OPS) op(full, MPMHIP_REGION_NEG);
  CHECK(ok<3>(full));
  return 0;
}

int rp_refuse_program() {
  std::string why;
  CHECK(!region_program::check<3>(nullptr, why) && why.find("description is required") != std::string::npos);
  { Desc d = prog_c(); d->n_ops = 0; CHECK(refused<3>(d, "the program is empty")); }
  { Desc d = prog_c(); d->n_ops = -3; CHECK(refused<3>(d, "the program is empty")); }
  { Desc d = prog_c(); d->n_ops = 25; CHECK(refused<3>(d, "at most 24 operations")); }
  { Desc d = prog_c(); d->n_leaves = 9; CHECK(refused<3>(d, "n_leaves = 9")); }
  { Desc d = prog_c(); d->n_leaves = 0; CHECK(refused<3>(d, "n_leaves = 0")); }
  { Desc d = prog_a(); d->n_fields = 5; CHECK(refused<3>(d, "n_fields = 5")); }
  { Desc d = prog_c(); d->ops[1].leaf = 3; CHECK(refused<3>(d, "operation 1: leaf index 3 out of range")); }
  { Desc d = prog_c(); d->ops[0].leaf = -1; CHECK(refused<3>(d, "operation 0: leaf index -1 out of range")); }
  { Desc d = prog_a(); d->leaves[1].field = 2; CHECK(refused<3>(d, "leaf 1: field index 2 out of range")); }
  { Desc d = prog_a(); d->leaves[0].field = -1; CHECK(refused<3>(d, "leaf 0: field index -1 out of range")); }
  { Desc d = prog_c(); d->ops[0].op = MPMHIP_REGION_UNION; CHECK(refused<3>(d, "operation 0: stack underflow")); }
  { Desc d = prog_c(); d->ops[0].op = MPMHIP_REGION_NEG; CHECK(refused<3>(d, "operation 0: stack underflow")); }
  { Desc d = prog_c(); d->ops[1].op = MPMHIP_REGION_INTERSECT; CHECK(refused<3>(d, "operation 1: stack underflow")); }
  { Desc d = prog_c(); d->n_ops = 0; for (int i = 0; i < 5; i++) push(d, 0); for (int i = 0; i < 4; i++) op(d, MPMHIP_REGION_UNION);
    CHECK(refused<3>(d, "operation 4: stack depth above 4")); }
  { Desc d = prog_c(); d->n_ops--; CHECK(refused<3>(d, "leaves 2 values on the stack")); }
  { Desc d = prog_c(); d->ops[2].op = 4; CHECK(refused<3>(d, "operation 2: unknown opcode 4")); }
  { Desc d = prog_c(); d->leaves[0].kind = 2; CHECK(refused<3>(d, "leaf 0: unknown kind 2")); }
  { Desc d = prog_c(); d->leaves[2].shape.type = 3; CHECK(refused<3>(d, "leaf 2: unknown shape type 3")); }
  return 0;
}

int rp_refuse_leaves() {
  const float nan = std::nanf(""), inf = HUGE_VALF;
  { Desc d = prog_b(); d->leaves[1].rot[4] = nan; CHECK(refused<3>(d, "leaf 1: the rotation is not finite")); }
  { Desc d = prog_b(); d->leaves[1].rot[8] = inf; CHECK(refused<3>(d, "the rotation is not finite")); }
  { Desc d = prog_b(); d->leaves[1].rot[0] = 1.0f; CHECK(refused<3>(d, "the rotation is not orthonormal")); }
  { Desc d = prog_b(); for (int k = 0; k < 9; k++) d->leaves[1].rot[k] *= 1.01f; CHECK(refused<3>(d, "the rotation is not orthonormal")); }
  { Desc d = prog_b(); memset(d->leaves[1].rot, 0, sizeof d->leaves[1].rot); CHECK(refused<3>(d, "the rotation is not orthonormal")); }
  { Desc d = prog_b(); for (int k = 0; k < 3; k++) d->leaves[1].rot[6 + k] = -d->leaves[1].rot[6 + k];  // orthonormal, det = -1
    CHECK(refused<3>(d, "leaf 1: the rotation is a reflection") && ok<2>(d)); }
  { Desc d = prog_b(); d->leaves[1].rot[0] = inf; CHECK(refused<2>(d, "the rotation is not finite")); }  // (D = 2: the angle)
  { Desc d = prog_b(); d->leaves[1].rot[4] = nan; CHECK(ok<2>(d)); }  // (D = 2 reads rot[0] alone)
  { Desc d = prog_b(); d->leaves[1].scale = 0.0f; CHECK(refused<3>(d, "scale must be a finite number > 0")); }
  { Desc d = prog_b(); d->leaves[1].scale = -1.0f; CHECK(refused<3>(d, "scale must be")); }
  { Desc d = prog_b(); d->leaves[1].scale = inf; CHECK(refused<3>(d, "scale must be")); }
  { Desc d = prog_b(); d->leaves[1].scale = nan; CHECK(refused<2>(d, "scale must be")); }
  { Desc d = prog_b(); d->leaves[1].translate[1] = nan; CHECK(refused<3>(d, "translate and pivot must be finite")); }
  { Desc d = prog_b(); d->leaves[1].pivot[2] = inf; CHECK(refused<3>(d, "translate and pivot must be finite") && ok<2>(d)); }
  { Desc d = prog_b(); d->leaves[0].scale = -1.0f; d->leaves[0].rot[0] = nan; CHECK(ok<3>(d)); }  // (not placed: not read)
  // shape leaves: what the level set's own check refuses, on the axes D reads, and non-finite parameters
  { Desc d = prog_c(); d->leaves[1].shape.p[3] = 0.0f; CHECK(refused<3>(d, "leaf 1: sphere radius must be > 0") && refused<2>(d, "sphere radius")); }
  { Desc d = prog_c(); d->leaves[0].shape.p[3] = nan; CHECK(refused<3>(d, "leaf 0: the shape's parameters must be finite")); }
  { Desc d = prog_c(); d->leaves[0].shape.p[2] = inf; CHECK(refused<3>(d, "parameters must be finite") && ok<2>(d)); }  // (z is not read in the plane)
  { Desc d = prog_c(); d->leaves[2].shape.p[3] = nan; CHECK(refused<2>(d, "leaf 2: the shape's parameters must be finite")); }
  { Desc d = prog_band(); d->leaves[1].shape.p[4] = 0.25f; CHECK(refused<3>(d, "leaf 1: cuboid needs lo < hi") && refused<2>(d, "cuboid needs")); }
  { Desc d = prog_band(); d->leaves[1].shape.p[5] = 0.0f; CHECK(refused<3>(d, "cuboid needs lo < hi") && ok<2>(d)); }
  { Desc d = prog_band(); d->leaves[1].shape.p[0] = nan; CHECK(refused<2>(d, "parameters must be finite")); }
  { Desc d = prog_band(); d->leaves[0].hi = 0.0f; CHECK(refused<3>(d, "leaf 0: a band needs lo < hi")); }
  { Desc d = prog_band(); d->leaves[0].lo = 4.0f; CHECK(refused<3>(d, "a band needs lo < hi")); }
  { Desc d = prog_band(); d->leaves[0].lo = nan; CHECK(refused<3>(d, "a band needs lo < hi")); }
  { Desc d = prog_band(); d->leaves[0].hi = nan; CHECK(refused<2>(d, "a band needs lo < hi")); }
  { Desc d = prog_band(); d->leaves[0].lo = -inf; d->leaves[0].hi = inf; CHECK(ok<3>(d)); }
  { Desc d = prog_band(); d->leaves[1].lo = 1.0f; d->leaves[1].hi = 0.0f; CHECK(ok<3>(d)); }  // (not banded: not read)
  return 0;
}

int rp_refuse_fields() {
  const float nan = std::nanf("");
  { Desc d = prog_a(); d->fields[1].res[2] = 1; CHECK(refused<3>(d, "field 1: res[2] = 1, at least 2 samples per axis are needed") && ok<2>(d)); }
  { Desc d = prog_a(); d->fields[0].res[0] = -5; CHECK(refused<2>(d, "field 0: res[0] = -5")); }
  { Desc d = prog_a(); d->fields[0].origin[1] = nan; CHECK(refused<3>(d, "field 0: origin[1] is not finite")); }
  { Desc d = prog_a(); d->fields[0].spacing = 0.0f; CHECK(refused<3>(d, "field 0: spacing must be a finite number > 0")); }
  { Desc d = prog_a(); d->fields[0].spacing = nan; CHECK(refused<3>(d, "spacing must be")); }
  { Desc d = prog_a(); for (int k = 0; k < 3; k++) d->fields[1].res[k] = 2000; CHECK(refused<3>(d, "field 1: more than 2^31 samples") && ok<2>(d)); }
  { Desc d = prog_a(); d->fields[1].phi = nullptr; CHECK(refused<3>(d, "field 1: its phi array is missing")); }
  { Desc d = prog_a(); d->n_fields = 1; CHECK(refused<3>(d, "leaf 1: field index 1 out of range (1 fields)")); }
  return 0;
}

// every byte of a valid description at 0x00 / 0x7F / 0xFF: accept or refuse with a reason, never a read outside the description
// (the sanitizer build is what would see one) and never an empty reason
int rp_sweep() {
  const Desc base[] = {prog_a(), prog_b(), prog_c(), prog_band(), prog_balanced8()};
  const unsigned char vals[3] = {0x00, 0x7F, 0xFF};
  long accepted = 0, refused_n = 0;
  for (const Desc &b : base)
    for (size_t at = 0; at < sizeof(mpmhip_region_desc); at++) {
      // the phi pointers are not data the check may follow: a spoilt pointer stays unread, so they are swept too
      for (unsigned char v : vals) {
        Desc d(b);
        d.p[at] = v;
        std::string why3, why2;
        const bool r3 = region_program::check<3>(d.get(), why3), r2 = region_program::check<2>(d.get(), why2);
        CHECK(r3 == why3.empty() && r2 == why2.empty());
        (r3 ? accepted : refused_n)++;
      }
    }
  CHECK(accepted > 0 && refused_n > 0);
  return 0;
}

}  // extern "C"

int main() {
  int (*const all[])() = {rp_accept, rp_refuse_program, rp_refuse_leaves, rp_refuse_fields, rp_sweep};
  const char *const names[] = {"rp_accept", "rp_refuse_program", "rp_refuse_leaves", "rp_refuse_fields", "rp_sweep"};
  int failed = 0;
  for (size_t i = 0; i < sizeof all / sizeof all[0]; i++)
    if (const int line = all[i]()) {
      std::printf("%s: check at line %d failed\n", names[i], line);
      failed = 1;
    }
  if (!failed) std::printf("region_program: %zu scenarios ok\n", sizeof all / sizeof all[0]);
  return failed;
}
