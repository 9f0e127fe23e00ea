// taichi_mpm_amd/csrc/region_program.h — what every entry point that takes a region expression demands of it (host only: no HIP
// header, no ctx; rules: include/mpmhip.h, "Region expressions").  Its callers are the two seeding entries and the two ctx-free
// entries of region_api.h; each puts its own name in front of the reason.  The check reads the description and nothing behind its
// pointers: a phi array is only asked to be there.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/mpmhip.h"
#include "sdf_lattice.h"

namespace region_program {

constexpr float ORTHO_TOL = 1e-4f;  // per entry of R^T R - I

inline bool finite3(const float *v, int n) {
  for (int k = 0; k < n; k++)
    if (!std::isfinite(v[k])) return false;
  return true;
}

// the number of samples of field f's lattice in *counts (when given); false: the description is refused and `why` says what is
// wrong with it.  D = 2 or 3.
template <int D>
bool check(const mpmhip_region_desc *r, std::string &why, size_t *counts = nullptr) {
  if (!r) { why = "the region description is required"; return false; }
  if (r->n_ops <= 0) { why = "the program is empty"; return false; }
  if (r->n_ops > MPMHIP_REGION_MAX_OPS) { why = "n_ops = " + std::to_string(r->n_ops) + ", at most " + std::to_string(MPMHIP_REGION_MAX_OPS) + " operations"; return false; }
  if (r->n_leaves <= 0 || r->n_leaves > MPMHIP_REGION_MAX_LEAVES) { why = "n_leaves = " + std::to_string(r->n_leaves) + " outside [1, " + std::to_string(MPMHIP_REGION_MAX_LEAVES) + "]"; return false; }
  if (r->n_fields < 0 || r->n_fields > MPMHIP_REGION_MAX_FIELDS) { why = "n_fields = " + std::to_string(r->n_fields) + " outside [0, " + std::to_string(MPMHIP_REGION_MAX_FIELDS) + "]"; return false; }
  for (int f = 0; f < r->n_fields; f++) {
    const mpmhip_region_field &F = r->fields[f];
    const std::string who = "field " + std::to_string(f) + ": ";
    std::string reason;
    const size_t count = sdf_lattice::check<D>(F.res, F.origin, F.spacing, reason);
    if (!count) { why = who + reason; return false; }
    if (!F.phi) { why = who + "its phi array is missing"; return false; }
    if (counts) counts[f] = count;
  }
  for (int i = 0; i < r->n_leaves; i++) {
    const mpmhip_region_leaf &L = r->leaves[i];
    const std::string who = "leaf " + std::to_string(i) + ": ";
    if (L.kind == 0) {  // what check_shapes asks of a shape of the level set, on the parameters D axes read, and finite ones
      const mpmhip_shape &S = L.shape;
      if (S.type < 0 || S.type > 2) { why = who + "unknown shape type " + std::to_string(S.type); return false; }
      if (S.type == 2) {
        if (!finite3(S.p, D) || !finite3(S.p + 3, D)) { why = who + "the shape's parameters must be finite"; return false; }
        for (int k = 0; k < D; k++)
          if (!(S.p[k] < S.p[3 + k])) { why = who + "cuboid needs lo < hi"; return false; }
      } else {
        if (!finite3(S.p, D) || !std::isfinite(S.p[3])) { why = who + "the shape's parameters must be finite"; return false; }
        if (S.type == 1 && !(S.p[3] > 0.0f)) { why = who + "sphere radius must be > 0"; return false; }
      }
    } else if (L.kind == 1) {
      if (L.field < 0 || L.field >= r->n_fields) { why = who + "field index " + std::to_string(L.field) + " out of range (" + std::to_string(r->n_fields) + " fields)"; return false; }
    } else {
      why = who + "unknown kind " + std::to_string(L.kind);
      return false;
    }
    if (L.placed) {
      if (D == 3) {
        if (!finite3(L.rot, 9)) { why = who + "the rotation is not finite"; return false; }
        for (int a = 0; a < 3; a++)
          for (int b = 0; b < 3; b++) {
            float s = 0.0f;
            for (int k = 0; k < 3; k++) s += L.rot[3 * k + a] * L.rot[3 * k + b];
            if (!(std::fabs(s - (a == b ? 1.0f : 0.0f)) <= ORTHO_TOL)) { why = who + "the rotation is not orthonormal"; return false; }
          }
        const float *R = L.rot;
        const float det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        if (!(det > 0.0f)) { why = who + "the rotation is a reflection (determinant < 0)"; return false; }
      } else if (!std::isfinite(L.rot[0])) {
        why = who + "the rotation is not finite";
        return false;
      }
      if (!(L.scale > 0.0f) || !std::isfinite(L.scale)) { why = who + "scale must be a finite number > 0"; return false; }
      if (!finite3(L.translate, D) || !finite3(L.pivot, D)) { why = who + "translate and pivot must be finite"; return false; }
    }
    if (L.banded && !(L.lo < L.hi)) { why = who + "a band needs lo < hi"; return false; }  // (false for a NaN in either edge)
  }
  int depth = 0;
  for (int i = 0; i < r->n_ops; i++) {
    const mpmhip_region_op &o = r->ops[i];
    const std::string who = "operation " + std::to_string(i) + ": ";
    if (o.op == MPMHIP_REGION_PUSH) {
      if (o.leaf < 0 || o.leaf >= r->n_leaves) { why = who + "leaf index " + std::to_string(o.leaf) + " out of range (" + std::to_string(r->n_leaves) + " leaves)"; return false; }
      if (++depth > MPMHIP_REGION_MAX_DEPTH) { why = who + "stack depth above " + std::to_string(MPMHIP_REGION_MAX_DEPTH); return false; }
    } else if (o.op == MPMHIP_REGION_UNION || o.op == MPMHIP_REGION_INTERSECT) {
      if (depth < 2) { why = who + "stack underflow"; return false; }
      depth--;
    } else if (o.op == MPMHIP_REGION_NEG) {
      if (depth < 1) { why = who + "stack underflow"; return false; }
    } else {
      why = who + "unknown opcode " + std::to_string(o.op);
      return false;
    }
  }
  if (depth != 1) { why = "the program leaves " + std::to_string(depth) + " values on the stack, not one"; return false; }
  return true;
}

}  // namespace region_program
