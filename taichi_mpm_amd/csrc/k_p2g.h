// taichi_mpm_amd/csrc/k_p2g.h — P2G (rasterize_optimized, src/transfer.cpp:467-569)
// Part of libmpmhip (see mpmhip.hip for the substep overview and the data layout).
#pragma once
#include "mpm_common.h"

namespace mpm {

// ------------------------------------------------------------------------------------------------ P2G
// rasterize_optimized / block_op_normal (src/transfer.cpp:467-569).
// Mapping: ONE WAVE PER active 4^3-cell block, ONE LANE PER CELL.  The sorted index lists the particles of each cell
// contiguously, so lane c walks its cell's particles and accumulates their node contributions in registers (the
// reference walks cells sequentially inside a block and accumulates into its scratch tile the same way,
// :474-483).  Write conflicts between particles of one cell therefore never reach memory; the wave merges its
// per-cell sums into its 6^3-node LDS tile by ordered, non-atomic float4 read-modify-writes and the tile is
// written out whole; conflicts between blocks are resolved by k_grid.  The records come through LDS
// (p2g_cell_staged).
// One particle's contribution (record q0..q3) to the 27 node sums of its cell, accumulated in registers.
__device__ __forceinline__ void p2g_particle(const Params &P, const float4 &q0, const float4 &q1, const float4 &q2,
                                             const float4 &q3, float ox, float oy, float oz, float (&acc)[27][4]) {
  const float mass = q3.w;  // the particle mass travels in the record: no dependent table lookup
  float v0 = q0.w, v1 = q1.x, v2 = q1.y;
  if (P.particle_gravity) {  // src/transfer.cpp:485-487
    v0 = fmaf(P.g[0], P.dt, v0); v1 = fmaf(P.g[1], P.dt, v1); v2 = fmaf(P.g[2], P.dt, v2);
  }
  // position relative to the base cell, in grid units: in [0.5, 1.5)^3  (:490,518)
  const float r0 = q0.x * P.idx - ox, r1 = q0.y * P.idx - oy, r2 = q0.z * P.idx - oz;
  float w0[3], w1[3], w2[3];
  bspline_weights(r0, w0); bspline_weights(r1, w1); bspline_weights(r2, w2);
  const float A00 = q1.z, A01 = q1.w, A02 = q2.x, A10 = q2.y, A11 = q2.z, A12 = q2.w, A20 = q3.x, A21 = q3.y,
              A22 = q3.z;
  const float mv0 = mass * v0, mv1 = mass * v1, mv2 = mass * v2;
  // contrib(i, j, k) = affine (r - (i, j, k)) + mass v is affine in the node offset: start from the node (0, 0, 0)
  // and step by one column of the affine matrix per node — (x, y) and (z, m) as packed fp32 pairs, the mass riding
  // along with a zero step: 2 packed adds + 2 packed multiply-adds per node instead of 9 + 4 scalar ones (256 -> 212
  // vector instructions per particle; the kernel is latency-bound, so only 0.171 -> 0.168 ms at C3, 0.206 -> 0.201 after
  // impact).  Same terms as :535-541, the offsets subtracted column by column instead of before the product.
  const f2 a0xy = {A00, A10}, a0zw = {A20, 0.0f}, a1xy = {A01, A11}, a1zw = {A21, 0.0f}, a2xy = {A02, A12},
           a2zw = {A22, 0.0f};
  f2 cixy = {fmaf(A02, r2, fmaf(A01, r1, fmaf(A00, r0, mv0))), fmaf(A12, r2, fmaf(A11, r1, fmaf(A10, r0, mv1)))};
  f2 cizw = {fmaf(A22, r2, fmaf(A21, r1, fmaf(A20, r0, mv2))), mass};
#pragma unroll
  for (int i3 = 0; i3 < 3; i3++) {
    f2 cjxy = cixy, cjzw = cizw;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const float wij = w0[i3] * w1[j];
      f2 ckxy = cjxy, ckzw = cjzw;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const int n = (i3 * 3 + j) * 3 + k;
        const f2 w = splat2(wij * w2[k]);
        f2 axy = {acc[n][0], acc[n][1]}, azw = {acc[n][2], acc[n][3]};
        axy = fma2(w, ckxy, axy); azw = fma2(w, ckzw, azw);
        acc[n][0] = axy.x; acc[n][1] = axy.y; acc[n][2] = azw.x; acc[n][3] = azw.y;
        if (k < 2) { ckxy -= a2xy; ckzw -= a2zw; }
      }
      if (j < 2) { cjxy -= a1xy; cjzw -= a1zw; }
    }
    if (i3 < 2) { cixy -= a0xy; cizw -= a0zw; }
  }
}

// Merge chains.  The merge is 27 read-modify-writes of the wave's tile that must stay in program order (two offsets of two
// lanes can name the same node): 27 x (LDS read latency + add + write) = 1.3 us of a block's ~15.  Instead every x-plane of the
// stencil merges into its OWN tile (tile + c * TN): three independent chains of nine steps whose reads, adds and writes interleave
// (measured -2..-4 us of 166 at C3); the write-out sums the three tiles.
constexpr int P2G_MC = 3;
// Merge the per-cell sums into this wave's tiles.  The tiles belong to this wavefront alone, and within one
// stencil-offset step all 64 lanes address distinct nodes (same offset, different cells), so a plain float4
// read-modify-write is race-free as long as the steps stay in program order: LDS operations of one wave
// execute in order, the wave_barrier keeps the compiler from interleaving them.  (DS float atomics cost
// ~2 LDS cycles per LANE on gfx950 even without conflicts: measured 145 cycles per ds_add_f32.)
__device__ __forceinline__ void p2g_merge(bool any, int nbase, float4 *tile, const float (&acc)[27][4]) {
#pragma unroll
  for (int s = 0; s < 9; s++) {
    float4 t[P2G_MC];
#pragma unroll
    for (int c = 0; c < P2G_MC; c++) t[c] = tile[c * TN + nbase + (c * TS + s / 3) * TS + s % 3];
    if (any) {
#pragma unroll
      for (int c = 0; c < P2G_MC; c++) {
        t[c].x += acc[c * 9 + s][0]; t[c].y += acc[c * 9 + s][1]; t[c].z += acc[c * 9 + s][2]; t[c].w += acc[c * 9 + s][3];
        tile[c * TN + nbase + (c * TS + s / 3) * TS + s % 3] = t[c];
      }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
  }
}

// Staged record loads.  The lanes walk their cells in lock step: in window w every lane takes particles 2w and 2w + 1 of its
// cell.  The wave fetches a window's 128 records (positions cell_start + 2w, + 2w + 1 of the 64 cells) TOGETHER: lane l holds
// the indices of records l and l + 64 (perm lanes), and each of 8 float4 loads takes quarter l & 3 of record 16 i + (l >> 2),
// i.e. 16 whole records per instruction — k_g2p writes the records at their sorted positions, so perm is near the identity and
// an instruction covers ~1 KiB in a few lines, where a lane loading its own records touches 64 lines per instruction (one per
// lane; profiles/p2g_staged_*: TA busy and L1 requests).  The window goes to LDS, and every lane reads its own records from
// there, each cell's particles in sorted order.
constexpr int P2G_WIN = 2;                      // particles per cell in a staged window
constexpr int P2G_STAGE = 4 * P2G_WIN * BC;     // float4 of the staging image: [quarter][slot][cell], in the wave's tile area
// image index of quarter q of the record in slot t of cell c: k = 2q + t picks a 1 KiB row, the cell XOR k inside it makes
// both the ds_write_b128 of the loads (8 lanes = one cell, k = 0..7) and the ds_read_b128 of one k (lane = cell) conflict-free
__device__ __forceinline__ int p2g_stage_at(int k, int c) { return k * BC + (c ^ k); }

struct P2GStage {
  uint32_t bA, nA, bB, nB;  // first sorted position and particle count of the cells of this lane's records l and l + 64
  uint32_t pA, pB;          // their indices (perm) in the next window to be loaded, ~0u where the cell has no such particle
  uint32_t nw;              // windows of the block: ceil(fullest cell / P2G_WIN), wave-uniform
};

__device__ __forceinline__ void p2g_stage_perm(const uint32_t *__restrict__ perm, P2GStage &s, uint32_t t0, int lane) {
  const uint32_t t = t0 + (lane & 1);
  s.pA = t < s.nA ? perm[s.bA + t] : ~0u;
  s.pB = t < s.nB ? perm[s.bB + t] : ~0u;
}

__device__ __forceinline__ void p2g_stage_load(const float4 *__restrict__ rp, const P2GStage &s, float4 (&R)[8], int lane) {
  uint32_t idx[8];  // (all shuffles first: the loads then issue back to back)
#pragma unroll
  for (int i = 0; i < 8; i++) idx[i] = (uint32_t)__shfl((int)(i < 4 ? s.pA : s.pB), (i & 3) * 16 + (lane >> 2));
#pragma unroll
  for (int i = 0; i < 8; i++) {
    if (idx[i] != ~0u) R[i] = rp[(size_t)idx[i] * 4 + (lane & 3)];
  }
}

__device__ __forceinline__ void p2g_stage_store(float4 *stage, const float4 (&R)[8], int lane) {
  __builtin_amdgcn_wave_barrier();  // (every lane's reads of the previous window are issued before the image is overwritten)
  asm volatile("" ::: "memory");
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int j = i * 16 + (lane >> 2);
    stage[p2g_stage_at((lane & 3) * 2 + (j & 1), j >> 1)] = R[i];
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

template <class AfterParticles>
__device__ __forceinline__ void p2g_cell_staged(const Params &P, const float4 *__restrict__ rp,
                                                const uint32_t *__restrict__ perm, P2GStage s, uint32_t n, float ox, float oy,
                                                float oz, int nbase, int lane, float4 *tile, AfterParticles &&after_particles) {
  static_assert(P2G_WIN == 2 && P2G_STAGE <= P2G_MC * TN, "the staging image lives in the wave's tile area");
  float acc[27][4];
#pragma unroll
  for (int n = 0; n < 27; n++) { acc[n][0] = 0.0f; acc[n][1] = 0.0f; acc[n][2] = 0.0f; acc[n][3] = 0.0f; }
  float4 *stage = tile;
  // software pipeline: while window w is computed, the records of window w + 1 and the indices of window w + 2 are in flight
  float4 R[8];
#pragma unroll
  for (int i = 0; i < 8; i++) R[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (s.nw > 0) {  // (the indices of window 0: loaded by the caller while the previous block was merged)
    p2g_stage_load(rp, s, R, lane);
    if (s.nw > 1) p2g_stage_perm(perm, s, P2G_WIN, lane);
    p2g_stage_store(stage, R, lane);
  }
  for (uint32_t w = 0; w < s.nw; w++) {  // (wave-uniform)
    if (w + 1 < s.nw) {
      p2g_stage_load(rp, s, R, lane);
      if (w + 2 < s.nw) p2g_stage_perm(perm, s, (w + 2) * P2G_WIN, lane);
    }
#pragma unroll 1
    for (int t = 0; t < P2G_WIN; t++) {  // (not unrolled: one copy of the particle's ~210 instructions)
      if (w * P2G_WIN + t < n) {
        const float4 q0 = stage[p2g_stage_at(0 + t, lane)], q1 = stage[p2g_stage_at(2 + t, lane)],
                     q2 = stage[p2g_stage_at(4 + t, lane)], q3 = stage[p2g_stage_at(6 + t, lane)];
        p2g_particle(P, q0, q1, q2, q3, ox, oy, oz, acc);
      }
    }
    if (w + 1 < s.nw) p2g_stage_store(stage, R, lane);
  }
  after_particles();  // (the caller's look-ahead loads for the next block: in flight during the merge and the write-out)
  // the image shares the tile's memory: the tile is cleared once the last window has been read
  __syncthreads();
  for (int t = lane; t < P2G_MC * TN; t += 64) tile[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  __syncthreads();
  p2g_merge(n > 0, nbase, tile, acc);
}

template <bool RIGID>  // RIGID: skip the blocks flagged in blk_rigid (k_p2g_rigid takes them)
__global__ __launch_bounds__(64, 2) void k_p2g(Params P, const float4 *__restrict__ rp, const Counters *__restrict__ cnt,
                                               const uint32_t *__restrict__ act_blk, const uint32_t *__restrict__ cell_start,
                                               const uint32_t *__restrict__ perm, const GroupParams *__restrict__ groups,
                                               float4 *__restrict__ tiles, Tiling T, int phase,
                                               const uint8_t *__restrict__ blk_rigid) {
  __shared__ float4 tile[P2G_MC][TN];  // per merge chain: (m*vx, m*vy, m*vz, m) per node of the block's 6^3 tile
  const uint32_t na = min(cnt->n_active, P.max_blocks);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;  // (wave: always 0, see load_indices)
  const int cx = lane >> 4, cy = (lane >> 2) & 3, cz = lane & 3;
  const int nbase = (cx * TS + cy) * TS + cz;
  // The start of a block is a chain of dependent loads (block key, cell table, first indices, first records).  The
  // first three links are taken one block ahead: key and cell range of the NEXT block are requested before this block's
  // particle loop, its first indices before this block's tile is merged and written out — a block then starts with
  // its record loads.
  struct Ahead { uint32_t key, c0, c1, p0, p1; P2GStage s; };
  auto load_table = [&](uint32_t a, Ahead &h) {
    h.key = 0; h.c0 = 0; h.c1 = 0;
    if (a < na) { h.key = act_blk[a]; h.c0 = cell_start[a * BC + lane]; h.c1 = cell_start[a * BC + lane + 1]; }
  };
  auto load_indices = [&](Ahead &h) {  // (all 64 lanes active: the ranges of the perm lanes' cells come by shuffles)
    // [p0, p1) = [c0, c1), written as the range of wave 0 of a split of the cell's particles: the form the kernel was tuned in.
    // Plain c0 / c1 compile to another schedule (1262 instead of 1254 instructions, profiles/kernel_diff.py).
    const uint32_t m = h.c1 - h.c0;
    h.p0 = h.c0 + m * wave;
    h.p1 = h.c0 + m * (wave + 1);
    const uint32_t n = h.p1 - h.p0;
    const int ca = lane >> 1, cb = 32 + (lane >> 1);
    h.s.bA = (uint32_t)__shfl((int)h.p0, ca); h.s.nA = (uint32_t)__shfl((int)n, ca);
    h.s.bB = (uint32_t)__shfl((int)h.p0, cb); h.s.nB = (uint32_t)__shfl((int)n, cb);
    uint32_t nmax = n;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nmax = max(nmax, (uint32_t)__shfl_xor((int)nmax, off));
    h.s.nw = (nmax + P2G_WIN - 1) / P2G_WIN;
    p2g_stage_perm(perm, h.s, 0, lane);
  };
  Ahead cur, nxt;
  load_table(blockIdx.x, cur);
  load_indices(cur);
  for (uint32_t a = blockIdx.x; a < na; a += gridDim.x) {
    load_table(a + gridDim.x, nxt);
    int bx, by, bz;
    demorton3(cur.key, bx, by, bz);
    bool mine = in_phase(T, phase, bx * BS, by * BS, bz * BS, TS);  // workgroup-uniform
    if constexpr (RIGID) { if (blk_rigid[a]) mine = false; }  // near a rigid body: k_p2g_rigid takes the block (CPIC colour test)
    if (!mine) {
      load_indices(nxt);
      cur = nxt;
      continue;
    }
    const float ox = (float)(bx * BS + cx), oy = (float)(by * BS + cy), oz = (float)(bz * BS + cz);
    auto ahead = [&]() { load_indices(nxt); };
    p2g_cell_staged(P, rp, perm, cur.s, cur.p1 - cur.p0, ox, oy, oz, nbase, lane, &tile[0][0], ahead);
    __syncthreads();
    for (int t = threadIdx.x; t < TN; t += 64) {
      float4 u = tile[0][t];
#pragma unroll
      for (int w = 1; w < P2G_MC; w++) {
        const float4 q = tile[w][t];
        u.x += q.x; u.y += q.y; u.z += q.z; u.w += q.w;
      }
      tiles[(size_t)a * TN + t] = u;
    }
    __syncthreads();
    cur = nxt;
  }
}

}  // namespace mpm
