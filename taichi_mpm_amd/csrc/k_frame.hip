// taichi_mpm_amd/csrc/k_frame.hip — the kernels of a job's frame (k_frame.h) and of a job's snapshot (k_snapshot_job.h) with their
// launchers (frame_launch.h, snapshot_job_launch.h), the impulse rows of a job with CPIC rigid bodies (k_rigid_rows.h,
// rigid_rows_launch.h) and the device-pointer field calls (k_fields.h, fields_launch.h): the second translation unit of libmpmhip.so,
// with a code object of its own.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mpmhip.h"
#define MPM_BGEO_ROW_ONLY  // of k_bgeo.h: bgeo_row, not the one-ctx kernels
#include "k_frame.h"
#include "k_snapshot_job.h"
#include "k_rigid_rows.h"
#include "k_fields.h"

namespace mpm {

void frame_launch_top(hipStream_t st, int grid, uint32_t n_slots, const RecG *rg, uint32_t *top) {
  hipLaunchKernelGGL(k_live_id_top, dim3(grid), dim3(FRAME_WG), 0, st, n_slots, rg, top);
}
void frame_launch_mark(hipStream_t st, int grid, uint32_t n_slots, const RecG *rg, uint32_t top, uint32_t *bits, uint32_t *live, int32_t *err) {
  hipLaunchKernelGGL(k_id_mark, dim3(grid), dim3(FRAME_WG), 0, st, n_slots, rg, top, bits, live, err);
}
void frame_launch_prefix(hipStream_t st, uint32_t n_words, uint32_t n_blocks, const uint32_t *bits, uint32_t *sums, uint32_t *prefix) {
  hipLaunchKernelGGL(k_id_prefix_sums, dim3(n_blocks), dim3(FRAME_WG), 0, st, n_words, bits, sums);
  hipLaunchKernelGGL(k_id_prefix_scan, dim3(1), dim3(FRAME_WG), 0, st, n_blocks, sums);
  hipLaunchKernelGGL(k_id_prefix_add, dim3(n_blocks), dim3(FRAME_WG), 0, st, n_words, bits, (const uint32_t *)sums, prefix);
}
void frame_launch_rows(hipStream_t st, int grid, bool verbose, uint32_t n_slots, const RecG *rg, const RecP *rp, const float *rb,
                       const GroupParams *groups, const int32_t *limits, uint32_t top, const uint32_t *bits, const uint32_t *prefix,
                       uint32_t n_rows, uint32_t *rows, const uint32_t *job_bits, const uint32_t *job_prefix, uint32_t *row_index, int32_t *err) {
  auto k = verbose ? k_bgeo_rows_ranked<true> : k_bgeo_rows_ranked<false>;
  hipLaunchKernelGGL(k, dim3(grid), dim3(FRAME_WG), 0, st, n_slots, rg, rp, rb, groups, limits, top, bits, prefix, n_rows, rows, job_bits, job_prefix,
                     row_index, err);
}

void snap_launch_rows(hipStream_t st, int grid, uint32_t n_slots, const float4 *rg, const float4 *rp, const float4 *rb, uint32_t top,
                      const uint32_t *bits, const uint32_t *prefix, uint32_t n_rows, float4 *out_rg, float4 *out_rp, float4 *out_rb,
                      const uint32_t *job_bits, const uint32_t *job_prefix, uint32_t *row_index, int32_t *err) {
  hipLaunchKernelGGL(k_snap_rows_ranked, dim3(grid), dim3(FRAME_WG), 0, st, n_slots, rg, rp, rb, top, bits, prefix, n_rows, out_rg, out_rp, out_rb,
                     job_bits, job_prefix, row_index, err);
}
void snap_launch_own_count(hipStream_t st, const Params &P, const Tiling &T, uint32_t n, const float4 *rg, uint32_t *totals, uint32_t *small) {
  hipLaunchKernelGGL(k_snap_own_count, dim3(snap_spans(n)), dim3(256), 0, st, P, T, n, rg, totals, small);
}
void snap_launch_own_emit(hipStream_t st, const Params &P, const Tiling &T, uint32_t n, const float4 *rg, const float4 *rp, const float4 *rb,
                          const uint32_t *offs, uint32_t cap, float4 *out_rg, float4 *out_rp, float4 *out_rb, uint32_t *small) {
  hipLaunchKernelGGL(k_snap_own_emit, dim3(snap_spans(n)), dim3(256), 0, st, P, T, n, rg, rp, rb, offs, cap, out_rg, out_rp, out_rb, small);
}


void rows_launch_sum(hipStream_t st, int nb, const Params &P, const Counters *cnt, const uint8_t *blk_rigid, const float *rows, RigidBodyDev *rb) {
  hipLaunchKernelGGL(k_rigid_rows_sum, dim3(nb - 1), dim3(ROWS_SUM_WG), 0, st, P, cnt, blk_rigid, rows, rb);
}
void rows_launch_out(hipStream_t st, RigidBodyDev *rb, int nb, const RowPut &L, int world, float *stage, uint32_t epoch) {
  hipLaunchKernelGGL(k_rigid_row_out, dim3(1), dim3(ROW_OUT_WG), 0, st, rb, nb, L, world, stage, epoch);
}
void rows_launch_apply(hipStream_t st, RigidBodyDev *rb, int nb, const float *table, int world, const uint32_t *words, int n_wait,
                       uint32_t epoch, unsigned long long timeout_ticks, Counters *cnt) {
  hipLaunchKernelGGL(k_rigid_rows_world, dim3(1), dim3(64), 0, st, rb, nb, table, world, words, n_wait, epoch, timeout_ticks, cnt);
}

void fields_launch_count(hipStream_t st, uint32_t n_slots, const RecG *rg, uint32_t *totals) {
  const uint32_t spans = fields_spans(n_slots);
  hipLaunchKernelGGL(k_fields_count, dim3(spans), dim3(FIELDS_WG), 0, st, n_slots, rg, totals);
  hipLaunchKernelGGL(k_id_prefix_scan, dim3(1), dim3(FRAME_WG), 0, st, spans, totals);
}
void fields_launch_emit(hipStream_t st, uint32_t n_slots, const float4 *rg, const float4 *rp, const float4 *rb, const uint32_t *offs,
                        uint32_t n_rows, const FieldTable &dst) {
  hipLaunchKernelGGL(k_fields_emit, dim3(fields_spans(n_slots)), dim3(FIELDS_WG), 0, st, n_slots, rg, rp, rb, offs, n_rows, dst);
}
void fields_launch_emit_ranked(hipStream_t st, uint32_t n_slots, const float4 *rg, const float4 *rp, const float4 *rb, uint32_t top,
                               const uint32_t *bits, const uint32_t *prefix, uint32_t n_rows, const FieldTable &dst, int32_t *err) {
  hipLaunchKernelGGL(k_fields_emit_ranked, dim3(fields_spans(n_slots)), dim3(FIELDS_WG), 0, st, n_slots, rg, rp, rb, top, bits, prefix, n_rows, dst, err);
}
void fields_launch_put(hipStream_t st, bool ranked, uint32_t n_slots, RecG *rg, RecP *rp, float *rb, const uint32_t *offs, uint32_t top,
                       const uint32_t *bits, const uint32_t *prefix, uint32_t n_rows, const FieldTable &src, uint32_t *small) {
  auto k = ranked ? k_fields_put<true> : k_fields_put<false>;
  hipLaunchKernelGGL(k, dim3(fields_spans(n_slots)), dim3(FIELDS_WG), 0, st, n_slots, rg, rp, rb, offs, top, bits, prefix, n_rows, src, small);
}

}  // namespace mpm
