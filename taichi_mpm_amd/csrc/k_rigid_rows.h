// taichi_mpm_amd/csrc/k_rigid_rows.h — CPIC rigid bodies on a tiled job: a rank's impulse row out, all ranks' rows summed in rank
// order and applied.  Compiled in k_frame.hip (the second code object of libmpmhip.so); launchers: rigid_rows_launch.h.
//
// Every rank of a job holds ALL bodies, and their records are byte-identical on all ranks at every substep boundary.  What couples
// the ranks is tmp_imp / tmp_trq of each body: a rank's colour-aware transfer kernels (k_p2g_rigid, k_g2p_rigid) collect there what
// the rank's own particles hand the bodies.  On one ctx k_rigid_apply_tmp (k_rigid_rows_apply in the deterministic mode) turns the
// sums into velocities.  On a job
//   k_rigid_rows_sum     (deterministic mode only) k_rigid_rows_apply's fixed-order sum over the flagged blocks' rows of d_imp_rows,
//                        written to tmp_imp / tmp_trq instead of applied
//   k_rigid_row_out      moves tmp_imp / tmp_trq of all bodies into the rank's ROW (IMP_ROW floats, tiled_plan.h) and clears them;
//                        the row goes to its place in every rank's table by peer writes, and the exchange's epoch behind it
//   k_rigid_rows_world   waits for the epochs of all ranks (the bounded wait of the halo boxes: error bit 16 after timeout_ticks),
//                        adds the rows r = 0 .. world - 1 in that order and applies the sum with k_rigid_apply_tmp's arithmetic
// Every rank adds the same rows in the same order: the replicas stay one, whatever the order the rows arrived in.
#pragma once
#include "rigid_rows_launch.h"

namespace mpm {

constexpr int ROWS_SUM_WG = 1024;

__global__ __launch_bounds__(ROWS_SUM_WG) void k_rigid_rows_sum(Params P, const Counters *__restrict__ cnt, const uint8_t *__restrict__ blk_rigid,
                                                                const float *__restrict__ rows, RigidBodyDev *rb) {
  __shared__ float red[6][ROWS_SUM_WG];
  const int b = blockIdx.x + 1, t = threadIdx.x;
  const uint32_t na = min(cnt->n_active, P.max_blocks);
  float s[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (uint32_t a = t; a < na; a += ROWS_SUM_WG) {  // thread t: the rows a = t, t + 1024, ... in turn
    const bool flagged = blk_rigid[a] != 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const float r = rows[(size_t)a * tplan::IMP_ROW_FLOATS + b * 6 + k];
      s[k] += flagged ? r : 0.0f;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; k++) red[k][t] = s[k];
  __syncthreads();
  for (int h = ROWS_SUM_WG / 2; h > 0; h >>= 1) {  // a fixed tree over the threads
    if (t < h) {
#pragma unroll
      for (int k = 0; k < 6; k++) red[k][t] += red[k][t + h];
    }
    __syncthreads();
  }
  if (t < 6) {  // (nothing else adds to them in this mode)
    if (t < 3) rb[b].tmp_imp[t] = red[t][0];
    else rb[b].tmp_trq[t - 3] = red[t][0];
  }
}

constexpr int ROW_OUT_WG = 128;  // >= IMP_ROW floats, >= MAX_WORLD flags
static_assert(ROW_OUT_WG >= tplan::IMP_ROW_FLOATS && ROW_OUT_WG >= tplan::MAX_WORLD, "one thread per float of a row, one per rank");

__global__ __launch_bounds__(ROW_OUT_WG) void k_rigid_row_out(RigidBodyDev *rb, int nb, RowPut L, int world, float *stage, uint32_t epoch) {
  const int t = threadIdx.x;
  if (t < tplan::IMP_ROW_FLOATS) {
    const int b = t / 6, k = t % 6;
    float v = 0.0f;  // (body 0, the background, and the bodies the scene does not have: zeros)
    if (b >= 1 && b < nb) {
      float *p = k < 3 ? &rb[b].tmp_imp[k] : &rb[b].tmp_trq[k - 3];
      v = *p;
      *p = 0.0f;
    }
    if (stage) stage[t] = v;
    for (int p = 0; p < world; p++)
      if (L.dst[p]) L.dst[p][t] = v;
  }
  __threadfence_system();
  __syncthreads();
  if (t < world && L.flag[t]) __hip_atomic_store(L.flag[t], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(64) void k_rigid_rows_world(RigidBodyDev *rb, int nb, const float *table, int world, const uint32_t *words,
                                                         int n_wait, uint32_t epoch, unsigned long long timeout_ticks, Counters *cnt) {
  const int t = threadIdx.x;
  if (t < n_wait) {  // lane r waits until rank r has published the exchange's epoch (k_epoch_wait's loop)
    const uint32_t *w = words + t;
    const unsigned long long t0 = wall_clock64();
    while ((int32_t)(__hip_atomic_load(w, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) - epoch) < 0) {
      __builtin_amdgcn_s_sleep(16);
      if (wall_clock64() - t0 > timeout_ticks) {
        atomicOr(&cnt->error, 16u);
        break;
      }
    }
  }
  __syncthreads();
  __atomic_thread_fence(__ATOMIC_ACQUIRE);  // (system scope: the lanes that did not wait read behind the ones that did)
  const int b = t;
  if (b < 1 || b >= nb) return;
  const uint32_t *tw = reinterpret_cast<const uint32_t *>(table);
  float s[6];
#pragma unroll
  for (int k = 0; k < 6; k++) {  // rank order: ((row 0 + row 1) + row 2) + ...
    float a = 0.0f;
    for (int r = 0; r < world; r++) {
      const float v = __uint_as_float(__hip_atomic_load(tw + (size_t)r * tplan::IMP_ROW_FLOATS + b * 6 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
      a = r == 0 ? v : a + v;
    }
    s[k] = a;
  }
  RigidBodyDev &B = rb[b];  // (k_rigid_apply_tmp's arithmetic, k_rigid.h)
  float tb[3], u[3], w[3];
#pragma unroll
  for (int k = 0; k < 3; k++) B.vel[k] += s[k] * B.inv_mass;
  // world inverse inertia applied to the torque: R (I^-1 (R^T torque))
#pragma unroll
  for (int c = 0; c < 3; c++) tb[c] = B.R[c] * s[3] + B.R[3 + c] * s[4] + B.R[6 + c] * s[5];
#pragma unroll
  for (int r = 0; r < 3; r++) u[r] = B.inv_I[3 * r] * tb[0] + B.inv_I[3 * r + 1] * tb[1] + B.inv_I[3 * r + 2] * tb[2];
#pragma unroll
  for (int r = 0; r < 3; r++) w[r] = B.R[3 * r] * u[0] + B.R[3 * r + 1] * u[1] + B.R[3 * r + 2] * u[2];
#pragma unroll
  for (int k = 0; k < 3; k++) B.omega[k] += w[k];
}

}  // namespace mpm
