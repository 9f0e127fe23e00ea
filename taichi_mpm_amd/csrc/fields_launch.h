// taichi_mpm_amd/csrc/fields_launch.h — what the host driver of the device-pointer field calls (fields_api.h, in mpmhip.hip) sees of
// the kernels of k_fields.h: their launchers.  The kernels are compiled by k_frame.hip, outside the code object with the substep's
// kernels (frame_launch.h says why).  Host only.
#pragma once
#include "frame_launch.h"

namespace mpm {

constexpr int FIELDS_WG = 256;  // threads per workgroup of every kernel of k_fields.h = slots per workgroup: a lane per slot
static_assert(FIELDS_WG == FRAME_WG, "k_fields.h sums a workgroup's waves as k_frame.h does and scans the workgroup totals with its k_id_prefix_scan");

// the field tables of mpmhip_download_dev / mpmhip_upload_dev as the kernels take them (by value): index = MPMHIP_F_*, null = not wanted
struct FieldTable {
  void *p[8];
};

// the small words of an upload: 1 + the largest id written (0: none), the largest row number at or beyond the row count (-1: none)
enum { FIELDS_W_TOP = 0, FIELDS_W_ERR = 1, FIELDS_WORDS = 2 };

inline uint32_t fields_spans(uint32_t n_slots) { return (n_slots + FIELDS_WG - 1) / FIELDS_WG; }

// slot order, launches 1 and 2: totals[w] = live slots of workgroup w's FIELDS_WG slots, then their exclusive prefix in place with
// totals[fields_spans(n_slots)] = the live slots of the ctx (k_id_prefix_scan of k_frame.h)
void fields_launch_count(hipStream_t st, uint32_t n_slots, const RecG *rg, uint32_t *totals);
// launch 3: the wanted fields of every live slot to row offs[workgroup] + (live slots before it in the workgroup); rows of more
// than one word go through LDS and leave as consecutive words
void fields_launch_emit(hipStream_t st, uint32_t n_slots, const float4 *rg, const float4 *rp, const float4 *rb, const uint32_t *offs,
                        uint32_t n_rows, const FieldTable &dst);
// id order: row = the rank of the slot's id in (bits, prefix) of frame_launch_mark / frame_launch_prefix; err as k_bgeo_rows_ranked's
void fields_launch_emit_ranked(hipStream_t st, uint32_t n_slots, const float4 *rg, const float4 *rp, const float4 *rb, uint32_t top,
                               const uint32_t *bits, const uint32_t *prefix, uint32_t n_rows, const FieldTable &dst, int32_t *err);
// upload: the row number as above (offs: slot order; bits: id order, by the ids the slots hold before the launch), the named fields of
// row -> record
void fields_launch_put(hipStream_t st, bool ranked, uint32_t n_slots, RecG *rg, RecP *rp, float *rb, const uint32_t *offs, uint32_t top,
                       const uint32_t *bits, const uint32_t *prefix, uint32_t n_rows, const FieldTable &src, uint32_t *small);

}  // namespace mpm
