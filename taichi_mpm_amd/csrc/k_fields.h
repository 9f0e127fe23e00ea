// taichi_mpm_amd/csrc/k_fields.h — particle fields between the records and caller-owned DEVICE arrays (mpmhip_download_dev,
// mpmhip_upload_dev: include/mpmhip.h), without a host copy.  A lane per slot everywhere, FIELDS_WG slots per workgroup.
//   slot order (the rows of mpmhip_download): an ordered stream compaction of the live slots (pid >= 0) in three launches,
//     k_fields_count     totals[w] = the live slots of workgroup w (ballot + popcount)
//     k_id_prefix_scan   (k_frame.h) their exclusive prefix, the sum behind it: the host reads that one word and judges the capacity
//                        before the third launch writes anything
//     k_fields_emit      row = prefix[w] + the live slots before the lane in its workgroup.  A lane loads its own slot's float4s — of
//                        RecG always (the id lives there), of RecP only for v, of the apic_b row only for B — so a wave's loads cover
//                        whole 64-byte records back to back.  Rows are 4, 12 or 36 bytes: a lane storing its own row scatters words
//                        at that stride, so the workgroup's rows of a 12- or 36-byte field are laid out in LDS first and leave as
//                        consecutive words (what k_g2p's transposed record store does in the other direction; measured
//                        against the lane-per-row store in DESIGN.md section 13).
//   id order (row r = the particle whose id has rank r among the live ids): k_live_id_top, k_id_mark, k_id_prefix_* of k_frame.h give
//     (bits, prefix); k_fields_emit_ranked places a slot's row by frame_rank.  The stores are scattered by nature.
//   upload: k_fields_put, the inverse — the row number as above (by the ids the slots hold BEFORE the launch, also when ids are what
//     is uploaded), a gather from the source rows, and stores into the named members of the record alone (x into RecG and RecP).
// No workgroup waits on another.  Every row number is checked against the row count before it is used, every id against `top`.
// 32-bit slot indices: a ctx holds fewer than 2^25 particles.  Compiled by k_frame.hip (fields_launch.h); host driver: fields_api.h.
// Part of libmpmhip; off the substep's path.
#pragma once
#include "k_frame.h"
#include "fields_launch.h"

namespace mpm {

// is the lane's slot live; its number among the live slots of the workgroup; their count (wave_n: FIELDS_WG / 64 words of LDS)
__device__ __forceinline__ uint32_t fields_wg_rank(bool live, uint32_t *wave_n, uint32_t &total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(live);
  if (lane == 0) wave_n[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t before = 0;
  total = 0;
#pragma unroll
  for (uint32_t w = 0; w < FIELDS_WG / 64; w++) {
    const uint32_t s = wave_n[w];
    before += w < wave ? s : 0u;
    total += s;
  }
  return before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(FIELDS_WG) void k_fields_count(uint32_t n_slots, const RecG *__restrict__ rg, uint32_t *__restrict__ totals) {
  __shared__ uint32_t wave_n[FIELDS_WG / 64];
  const uint32_t s = blockIdx.x * FIELDS_WG + threadIdx.x;
  uint32_t total;
  fields_wg_rank(s < n_slots && rg[s].pid >= 0, wave_n, total);
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// what a lane holds of its slot: RecG (x aux | F0-3 | F4-7 | F8 gid pid states), RecP's first two float4 (x v0 | v1 v2 A0 A1), the
// apic_b row (nine of twelve words used)
struct FieldRec {
  float4 g0, g1, g2, g3, p0, p1, b0, b1, b2;
};
__device__ __forceinline__ void fields_put3(float *q, float a, float b, float c) { q[0] = a; q[1] = b; q[2] = c; }
__device__ __forceinline__ void fields_put9(float *q, const float4 &a, const float4 &b, float c) {
  q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = a.w; q[4] = b.x; q[5] = b.y; q[6] = b.z; q[7] = b.w; q[8] = c;
}
// (g3 is loaded by the caller: it holds the id).  dst.p[] are kernel arguments: every branch on them is uniform.
__device__ __forceinline__ void fields_load(FieldRec &r, const FieldTable &dst, const float4 *__restrict__ rg, const float4 *__restrict__ rp,
                                            const float4 *__restrict__ rb, uint32_t s) {
  if (dst.p[MPMHIP_F_X] || dst.p[MPMHIP_F_AUX]) r.g0 = rg[(size_t)s * 4];
  if (dst.p[MPMHIP_F_F]) { r.g1 = rg[(size_t)s * 4 + 1]; r.g2 = rg[(size_t)s * 4 + 2]; }
  if (dst.p[MPMHIP_F_V]) { r.p0 = rp[(size_t)s * 4]; r.p1 = rp[(size_t)s * 4 + 1]; }
  if (dst.p[MPMHIP_F_B]) { r.b0 = rb[(size_t)s * 3]; r.b1 = rb[(size_t)s * 3 + 1]; r.b2 = rb[(size_t)s * 3 + 2]; }
}
// the one-word fields of a live lane to row j; the integer fields travel as the bit patterns the float4 loads brought
__device__ __forceinline__ void fields_words(const FieldRec &r, const FieldTable &dst, uint32_t j) {
  if (dst.p[MPMHIP_F_AUX]) static_cast<float *>(dst.p[MPMHIP_F_AUX])[j] = r.g0.w;
  if (dst.p[MPMHIP_F_GID]) static_cast<float *>(dst.p[MPMHIP_F_GID])[j] = r.g3.y;
  if (dst.p[MPMHIP_F_ID]) static_cast<float *>(dst.p[MPMHIP_F_ID])[j] = r.g3.z;
  if (dst.p[MPMHIP_F_STATES]) static_cast<float *>(dst.p[MPMHIP_F_STATES])[j] = r.g3.w;
}

// the workgroup's rows of one field of W words, `total` of them from row `base` on: the live lane with number d writes its row through
// `put` into LDS at d, then all lanes copy total * W consecutive words out.  Uniform: dst.
template <int W, class Put>
__device__ __forceinline__ void fields_rows(float *__restrict__ dst, float *lds, bool live, uint32_t d, uint32_t base, uint32_t total, Put put) {
  if (!dst) return;
  __syncthreads();  // (the field before this one has left the LDS)
  if (live) put(lds + d * W);
  __syncthreads();
  float *out = dst + (size_t)base * W;
  for (uint32_t i = threadIdx.x; i < total * W; i += FIELDS_WG) out[i] = lds[i];
}

__global__ __launch_bounds__(FIELDS_WG) void k_fields_emit(uint32_t n_slots, const float4 *__restrict__ rg, const float4 *__restrict__ rp,
                                                           const float4 *__restrict__ rb, const uint32_t *__restrict__ offs, uint32_t n_rows,
                                                           FieldTable dst) {
  __shared__ uint32_t wave_n[FIELDS_WG / 64];
  __shared__ float lds[FIELDS_WG * 9];
  const uint32_t s = blockIdx.x * FIELDS_WG + threadIdx.x;
  FieldRec r;
  r.g3 = make_float4(0.0f, 0.0f, __int_as_float(-1), 0.0f);
  if (s < n_slots) r.g3 = rg[(size_t)s * 4 + 3];
  const bool live = __float_as_int(r.g3.z) >= 0;
  uint32_t total;
  const uint32_t d = fields_wg_rank(live, wave_n, total);
  const uint32_t base = offs[blockIdx.x];
  // (the host sized the destinations by the scan's sum: a row at or beyond n_rows says the records changed between the launches)
  total = base >= n_rows ? 0u : min(total, n_rows - base);
  if (live) fields_load(r, dst, rg, rp, rb, s);
  if (live && d < total) fields_words(r, dst, base + d);
  fields_rows<3>(static_cast<float *>(dst.p[MPMHIP_F_X]), lds, live, d, base, total, [&](float *q) { fields_put3(q, r.g0.x, r.g0.y, r.g0.z); });
  fields_rows<3>(static_cast<float *>(dst.p[MPMHIP_F_V]), lds, live, d, base, total, [&](float *q) { fields_put3(q, r.p0.w, r.p1.x, r.p1.y); });
  fields_rows<9>(static_cast<float *>(dst.p[MPMHIP_F_B]), lds, live, d, base, total, [&](float *q) { fields_put9(q, r.b0, r.b1, r.b2.x); });
  fields_rows<9>(static_cast<float *>(dst.p[MPMHIP_F_F]), lds, live, d, base, total, [&](float *q) { fields_put9(q, r.g1, r.g2, r.g3.x); });
}

__global__ __launch_bounds__(FIELDS_WG) void k_fields_emit_ranked(uint32_t n_slots, const float4 *__restrict__ rg, const float4 *__restrict__ rp,
                                                                  const float4 *__restrict__ rb, uint32_t top, const uint32_t *__restrict__ bits,
                                                                  const uint32_t *__restrict__ prefix, uint32_t n_rows, FieldTable dst,
                                                                  int32_t *__restrict__ err) {
  const uint32_t s = blockIdx.x * FIELDS_WG + threadIdx.x;
  if (s >= n_slots) return;
  FieldRec r;
  r.g3 = rg[(size_t)s * 4 + 3];
  const int32_t pid = __float_as_int(r.g3.z);
  if (pid < 0) return;
  if ((uint32_t)pid >= top) { atomicMax(&err[FRAME_ERR_RANGE], pid); return; }
  uint32_t j;
  if (!frame_rank(bits, prefix, (uint32_t)pid, j) || j >= n_rows) { atomicMax(&err[FRAME_ERR_ABSENT], pid); return; }
  fields_load(r, dst, rg, rp, rb, s);
  fields_words(r, dst, j);
  if (dst.p[MPMHIP_F_X]) fields_put3(static_cast<float *>(dst.p[MPMHIP_F_X]) + (size_t)j * 3, r.g0.x, r.g0.y, r.g0.z);
  if (dst.p[MPMHIP_F_V]) fields_put3(static_cast<float *>(dst.p[MPMHIP_F_V]) + (size_t)j * 3, r.p0.w, r.p1.x, r.p1.y);
  if (dst.p[MPMHIP_F_B]) fields_put9(static_cast<float *>(dst.p[MPMHIP_F_B]) + (size_t)j * 9, r.b0, r.b1, r.b2.x);
  if (dst.p[MPMHIP_F_F]) fields_put9(static_cast<float *>(dst.p[MPMHIP_F_F]) + (size_t)j * 9, r.g1, r.g2, r.g3.x);
}

// Upload.  The members a field names are stored on their own (12-, 36- and 4-byte stores into the lane's own record lines), so nothing
// else of a record is read or rewritten: the aux beside x, v[0] behind RecP.x, A behind v and the three spare words of an apic_b row
// stay what they were.  An id below 0 is stored as 0 (mpmhip_upload); small[FIELDS_W_TOP] = max(1 + the ids stored).
template <bool RANKED>
__global__ __launch_bounds__(FIELDS_WG) void k_fields_put(uint32_t n_slots, RecG *__restrict__ rg, RecP *__restrict__ rp, float *__restrict__ rb,
                                                          const uint32_t *__restrict__ offs, uint32_t top, const uint32_t *__restrict__ bits,
                                                          const uint32_t *__restrict__ prefix, uint32_t n_rows, FieldTable src,
                                                          uint32_t *__restrict__ small) {
  __shared__ uint32_t wave_n[FIELDS_WG / 64];
  const uint32_t s = blockIdx.x * FIELDS_WG + threadIdx.x;
  const int32_t pid = s < n_slots ? rg[s].pid : -1;
  bool live = pid >= 0;
  uint32_t j = 0;
  if (RANKED) {
    if (live && ((uint32_t)pid >= top || !frame_rank(bits, prefix, (uint32_t)pid, j))) j = 0xFFFFFFFFu;
  } else {
    uint32_t total;
    j = offs[blockIdx.x] + fields_wg_rank(live, wave_n, total);
  }
  if (live && j >= n_rows) {  // (the host checked n against the live count: the records changed between the launches)
    atomicMax(reinterpret_cast<int32_t *>(&small[FIELDS_W_ERR]), (int32_t)min(j, 0x7FFFFFFFu));
    live = false;
  }
  uint32_t id_top = 0;
  if (live) {
    RecG &g = rg[s];
    RecP &p = rp[s];
    if (src.p[MPMHIP_F_X]) {
      const float *q = static_cast<const float *>(src.p[MPMHIP_F_X]) + (size_t)j * 3;
      const float x0 = q[0], x1 = q[1], x2 = q[2];
      g.x[0] = x0; g.x[1] = x1; g.x[2] = x2;
      p.x[0] = x0; p.x[1] = x1; p.x[2] = x2;
    }
    if (src.p[MPMHIP_F_V]) {
      const float *q = static_cast<const float *>(src.p[MPMHIP_F_V]) + (size_t)j * 3;
      const float v0 = q[0], v1 = q[1], v2 = q[2];
      p.v[0] = v0; p.v[1] = v1; p.v[2] = v2;
    }
    if (src.p[MPMHIP_F_B]) {
      const float *q = static_cast<const float *>(src.p[MPMHIP_F_B]) + (size_t)j * 9;
      float *b = rb + (size_t)s * BW;
#pragma unroll
      for (int k = 0; k < 9; k++) b[k] = q[k];
    }
    if (src.p[MPMHIP_F_F]) {
      const float *q = static_cast<const float *>(src.p[MPMHIP_F_F]) + (size_t)j * 9;
#pragma unroll
      for (int k = 0; k < 9; k++) g.F[k] = q[k];
    }
    if (src.p[MPMHIP_F_AUX]) g.aux = static_cast<const float *>(src.p[MPMHIP_F_AUX])[j];
    if (src.p[MPMHIP_F_STATES]) g.pad = static_cast<const uint32_t *>(src.p[MPMHIP_F_STATES])[j];
    if (src.p[MPMHIP_F_ID]) {
      const int32_t id = max(static_cast<const int32_t *>(src.p[MPMHIP_F_ID])[j], 0);
      g.pid = id;
      id_top = (uint32_t)id + 1u;
    }
  }
  if (src.p[MPMHIP_F_ID]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) id_top = max(id_top, (uint32_t)__shfl_xor(id_top, o));
    if ((threadIdx.x & 63) == 0 && id_top) atomicMax(&small[FIELDS_W_TOP], id_top);
  }
}

}  // namespace mpm
