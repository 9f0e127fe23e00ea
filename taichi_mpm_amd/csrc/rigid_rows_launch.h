// taichi_mpm_amd/csrc/rigid_rows_launch.h — what the substep driver of a tiled job with CPIC rigid bodies (mpmhip.hip, tiled_api.h)
// sees of the kernels of k_rigid_rows.h: their launchers.  The kernels are compiled in the second translation unit (k_frame.hip), so
// that the code object with the substep's kernels keeps its symbol table.  Host only.
#pragma once
#include "mpm_common.h"
#include "rigid_records.h"

namespace mpm {

static_assert(tplan::IMP_ROW_FLOATS == MAX_RIGID * 6, "a rank's impulse row: impulse and torque of every body");

// where a rank's row goes: its place in every rank's table of the exchange and parity in flight, and its epoch word on that rank's
// flag page.  Null: nothing travels there by a peer write (the RCCL wires carry the staged row instead).
struct RowPut {
  float *dst[MPMHIP_MAX_HALO_BOXES];
  uint32_t *flag[MPMHIP_MAX_HALO_BOXES];
};

// deterministic mode: the fixed-order sums over the flagged blocks' rows of d_imp_rows -> tmp_imp / tmp_trq of the bodies 1 .. nb - 1
void rows_launch_sum(hipStream_t st, int nb, const Params &P, const Counters *cnt, const uint8_t *blk_rigid, const float *rows, RigidBodyDev *rb);
// tmp_imp / tmp_trq of all bodies -> the rank's row (moved and cleared): to `stage` (if not null), to L.dst[p] of the ranks p < world,
// then `epoch` to L.flag[p]
void rows_launch_out(hipStream_t st, RigidBodyDev *rb, int nb, const RowPut &L, int world, float *stage, uint32_t epoch);
// [wait until words[0 .. n_wait) have reached `epoch`, bounded by timeout_ticks: error bit 16], then the rows table[r], r < world, added
// in rank order and applied to the bodies 1 .. nb - 1
void rows_launch_apply(hipStream_t st, RigidBodyDev *rb, int nb, const float *table, int world, const uint32_t *words, int n_wait,
                       uint32_t epoch, unsigned long long timeout_ticks, Counters *cnt);

}  // namespace mpm
