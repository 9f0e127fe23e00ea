// taichi_mpm_amd/csrc/snapshot_job_launch.h — what the host driver of a job's snapshot (snapshot_job_api.h, in mpmhip.hip) sees of the
// kernels of k_snapshot_job.h: their launchers.  The kernels are compiled by k_frame.hip, outside the code object with the substep's
// kernels (frame_launch.h says why).  Host only.
#pragma once
#include "frame_launch.h"

namespace mpm {

constexpr int SNAP_REC_F4 = 11;   // float4 of one record: RecG 4, RecP 4, the apic_b row 3
constexpr int SNAP_SPAN = 1024;   // records of a staged chunk one workgroup of k_snap_own_count / k_snap_own_emit owns, contiguous
// the small words of a load: live records, live records no rank can place, the emit's error word (-1 = none), then the six joint bounds
enum { SNAP_W_LIVE = 0, SNAP_W_LOST = 1, SNAP_W_ERR = 2, SNAP_W_BOUNDS = 3, SNAP_WORDS = 9 };

inline uint32_t snap_spans(uint32_t n) { return (n + SNAP_SPAN - 1) / SNAP_SPAN; }

// k_snap_rows_ranked over the n_slots records of one ctx, `grid` workgroups of FRAME_WG threads (arguments: the kernel's)
void snap_launch_rows(hipStream_t st, int grid, uint32_t n_slots, const float4 *rg, const float4 *rp, const float4 *rb, uint32_t top,
                      const uint32_t *bits, const uint32_t *prefix, uint32_t n_rows, float4 *out_rg, float4 *out_rp, float4 *out_rb,
                      const uint32_t *job_bits, const uint32_t *job_prefix, uint32_t *row_index, int32_t *err);
// k_snap_own_count / k_snap_own_emit over a staged chunk of n records: snap_spans(n) workgroups
void snap_launch_own_count(hipStream_t st, const Params &P, const Tiling &T, uint32_t n, const float4 *rg, uint32_t *totals, uint32_t *small);
void snap_launch_own_emit(hipStream_t st, const Params &P, const Tiling &T, uint32_t n, const float4 *rg, const float4 *rp, const float4 *rb,
                          const uint32_t *offs, uint32_t cap, float4 *out_rg, float4 *out_rp, float4 *out_rb, uint32_t *small);

}  // namespace mpm
