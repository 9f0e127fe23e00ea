// taichi_mpm_amd/csrc/frame_launch.h — what the host driver of a job's frame (frame_job_api.h, in mpmhip.hip) sees of the kernels of
// k_frame.h: their launchers.  The kernels are compiled in a translation unit of their own (k_frame.hip), so that the code object
// with the substep's kernels is, byte for byte, the one it was before these kernels existed.  Host only.
#pragma once
#include "mpm_common.h"

namespace mpm {

constexpr int FRAME_WG = 256;  // threads per workgroup of every kernel of k_frame.h, and words per workgroup of the prefix

// the error words of a frame (int32, -1 = none; the largest offending id otherwise)
enum { FRAME_ERR_TWICE = 0, FRAME_ERR_RANGE = 1, FRAME_ERR_ABSENT = 2, FRAME_ERR_WORDS = 3 };

// each launches its kernel on `st` with `grid` workgroups of FRAME_WG threads (arguments: the kernel's, k_frame.h)
void frame_launch_top(hipStream_t st, int grid, uint32_t n_slots, const RecG *rg, uint32_t *top);
void frame_launch_mark(hipStream_t st, int grid, uint32_t n_slots, const RecG *rg, uint32_t top, uint32_t *bits, uint32_t *live, int32_t *err);
// the three launches of k_id_prefix: sums[n_blocks + 1], prefix[n_words]; n_blocks = ceil(n_words / FRAME_WG)
void frame_launch_prefix(hipStream_t st, uint32_t n_words, uint32_t n_blocks, const uint32_t *bits, uint32_t *sums, uint32_t *prefix);
void frame_launch_rows(hipStream_t st, int grid, bool verbose, uint32_t n_slots, const RecG *rg, const RecP *rp, const float *rb,
                       const GroupParams *groups, const int32_t *limits, uint32_t top, const uint32_t *bits, const uint32_t *prefix,
                       uint32_t n_rows, uint32_t *rows, const uint32_t *job_bits, const uint32_t *job_prefix, uint32_t *row_index, int32_t *err);

}  // namespace mpm
