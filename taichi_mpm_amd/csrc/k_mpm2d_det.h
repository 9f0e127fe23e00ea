// taichi_mpm_amd/csrc/k_mpm2d_det.h — the deterministic mode of MPM<2> (mpmhip2d_config.deterministic): a substep that is a
// function of the particle SET (state + creation id) and the bodies, not of slot order, launch sizes or arrival order.
// The default path (k_mpm2d.h) scatters with global float atomics; here nothing is added atomically in float:
//   k2d_count / (scan) / k2d_fill / k2d_order   cell sort: key = dense index of the base node, every cell's entries in ascending
//                                               (creation id, slot) — the tie-break keeps duplicate ids a permutation
//   k2d_stage    one lane per sorted position: the particle's P2G record (the expressions of k_p2g), written once, coalesced;
//                with bodies also the impulses of the colour test, summed per workgroup in a fixed tree into a row
//   k2d_gather   one lane per node of a 4 x 64 tile: the records of a cell row are ONE contiguous range (cells along the second
//                axis are consecutive keys), loaded as whole records through LDS in chunks; every node of the dense grid is
//                written once with a plain store, zeros included (no memset of the grid)
//   k2d_g2p      with bodies: g2p_particle over the sorted positions, the penalty impulses into per-workgroup rows
//   k2d_rows_apply   the rows added in a fixed order and applied to the bodies (in place of k2_rigid_apply_tmp)
// Part of libmpmhip (C ABI: mpmhip2d_*).
#pragma once
#include <hip/hip_runtime.h>

#include "k_mpm2d.h"

namespace mpm2d {

constexpr int DET_TI = 4, DET_TJ = 64;  // node tile of k2d_gather: one wave per node row
constexpr int DET_CH = 256;             // records per LDS chunk (48 bytes each)
constexpr int DET_ROW = MAX_RIGID2 * 3; // floats of an impulse row: (impulse x, y, torque) per body

// particle p's key, or -1; a particle that is in no cell (it can only have been uploaded there) is deleted here, as k_g2p does on
// the default path — k_p2g tests the velocity after the gravity kick, so this does too
__global__ __launch_bounds__(256) void k2d_count(Params P, int64_t n, const float *__restrict__ x, const float *__restrict__ v,
                                                 int32_t *__restrict__ pid, int32_t *__restrict__ key, uint32_t *__restrict__ off,
                                                 uint32_t *__restrict__ count, unsigned int *__restrict__ n_dead) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  int32_t k = -1;
  if (pid[p] >= 0) {
    float vv[2] = {v[2 * p], v[2 * p + 1]};
    if (P.particle_gravity) { vv[0] += P.g[0] * P.dt; vv[1] += P.g[1] * P.dt; }
    const float xx[2] = {x[2 * p], x[2 * p + 1]};
    int b[2];
    if (alive_pos(P, xx, vv, b)) {
      k = b[0] * (P.res[1] + 1) + b[1];
      off[p] = atomicAdd(&count[k], 1u);  // (arrival order: only a place to stand until k2d_order)
    } else {
      pid[p] = -1;
      atomicAdd(n_dead, 1u);
    }
  }
  key[p] = k;
}
__global__ __launch_bounds__(256) void k2d_fill(int64_t n, const int32_t *__restrict__ key, const uint32_t *__restrict__ off,
                                                const uint32_t *__restrict__ start, uint32_t *__restrict__ unordered) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || key[p] < 0) return;
  unordered[start[key[p]] + off[p]] = (uint32_t)p;
}
// rank by counting: a particle's place in its cell is the number of entries with a smaller (id, slot) — any cell size works
__global__ __launch_bounds__(256) void k2d_order(int64_t n, const int32_t *__restrict__ key, const int32_t *__restrict__ pid,
                                                 const uint32_t *__restrict__ start, const uint32_t *__restrict__ unordered,
                                                 uint32_t *__restrict__ idx) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || key[p] < 0) return;
  const uint32_t lo = start[key[p]], hi = start[key[p] + 1];
  const int32_t id = pid[p];
  uint32_t rank = 0;
  for (uint32_t e = lo; e < hi; e++) {
    const uint32_t q = unordered[e];
    const int32_t qid = pid[q];
    rank += (qid < id || (qid == id && q < (uint32_t)p)) ? 1u : 0u;
  }
  idx[lo + rank] = (uint32_t)p;
}

// one lane's column of (impulse, torque) sums per body, then the workgroup's fixed tree: cols[k][t] += cols[k][t + stride]
__device__ __forceinline__ void imp_cols_clear(float (*cols)[256], int nb) {
  for (int k = 0; k < 3 * nb; k++) cols[k][threadIdx.x] = 0.0f;
}
__device__ __forceinline__ void imp_cols_to_row(float (*cols)[256], int nb, float *__restrict__ row) {
  const int t = threadIdx.x;
  for (int st = 128; st > 0; st >>= 1) {
    __syncthreads();
    if (t < st)
      for (int k = 0; k < 3 * nb; k++) cols[k][t] += cols[k][t + st];
  }
  __syncthreads();
  if (t < 3 * nb) row[t] = cols[t][0];
}

// the staged record: 3 x float4 = (r0, r1, m v.x, m v.y) (A) (mass, colour word, b1, slot)
template <bool RIGID>
__global__ __launch_bounds__(256) void k2d_stage(Params P, const uint32_t *__restrict__ total, const uint32_t *__restrict__ idx,
                                                 const float *__restrict__ x, float *__restrict__ v, const float *__restrict__ F,
                                                 const float *__restrict__ B, const float *__restrict__ aux,
                                                 const int32_t *__restrict__ gid, const GroupParams *__restrict__ groups,
                                                 float4 *__restrict__ rec, RigidArgs2 R, int nb, float *__restrict__ rows) {
  __shared__ float cols[RIGID ? DET_ROW : 1][256];
  if (RIGID) imp_cols_clear(cols, nb);
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s < *total) {
    const size_t p = idx[s];
    float vv[2] = {v[2 * p], v[2 * p + 1]};
    if (P.particle_gravity) {
      vv[0] += P.g[0] * P.dt; vv[1] += P.g[1] * P.dt;
      v[2 * p] = vv[0]; v[2 * p + 1] = vv[1];
    }
    const float xx[2] = {x[2 * p], x[2 * p + 1]};
    int b[2];
    alive_pos(P, xx, vv, b);  // (true: k2d_count keyed it)
    const GroupParams g = groups[gid[p]];
    const float mass = g.p[0];
    const m2 Fm = {F[4 * p], F[4 * p + 1], F[4 * p + 2], F[4 * p + 3]};
    const m2 st = calculate_force(g, Fm, aux[p]);
    const float S = -4.0f * P.idx * P.dt, m4 = 4.0f * mass;
    const float r0 = xx[0] * P.idx - (float)b[0], r1 = xx[1] * P.idx - (float)b[1];
    uint32_t pstate = 0u;
    if (RIGID) pstate = R.states[p];
    rec[3 * (size_t)s + 0] = make_float4(r0, r1, mass * vv[0], mass * vv[1]);
    rec[3 * (size_t)s + 1] = make_float4(st.a * S + B[4 * p] * m4, st.b * S + B[4 * p + 1] * m4, st.c * S + B[4 * p + 2] * m4, st.d * S + B[4 * p + 3] * m4);
    rec[3 * (size_t)s + 2] = make_float4(mass, __uint_as_float(pstate), __int_as_float(b[1]), __int_as_float((int)p));
    if (RIGID) {  // the impulses of k_p2g's colour test (src/transfer.cpp:227-254), into this lane's column
      const Bnd2 bn = R.bnd[p];
      float w0[3], w1[3];
      weights(r0, w0); weights(r1, w1);
      const int ny = P.res[1] + 1;
      const float t0[3] = {r0 - 1.5f, -2.0f * (r0 - 1.0f), r0 - 0.5f}, t1[3] = {r1 - 1.5f, -2.0f * (r1 - 1.0f), r1 - 0.5f};
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
          const uint32_t word = node_word2(R, (size_t)(b[0] + i) * ny + (b[1] + j));
          if (!incompatible2(word, pstate)) continue;
          const int rid = (int)(word >> 24) - 1;
          if (rid < 0) continue;
          const Rigid2 *Bd = R.rb + rid;
          const float w = w0[i] * w1[j];
          const float gpos[2] = {(b[0] + i) * P.dx, (b[1] + j) * P.dx};
          float rv[2], pv[2] = {vv[0], vv[1]};
          velocity_at2(*Bd, gpos, rv);
          friction_project2(pv, rv, bn.n, Bd->fric[(pstate >> (2 * rid)) & 1u]);
          const float gr[2] = {t0[i] * P.idx * w1[j], w0[i] * t1[j] * P.idx};
          const float imp[2] = {mass * w * (vv[0] - pv[0]) + P.dt * (st.a * gr[0] + st.b * gr[1]),
                                mass * w * (vv[1] - pv[1]) + P.dt * (st.c * gr[0] + st.d * gr[1])};
          cols[3 * rid + 0][threadIdx.x] += imp[0];
          cols[3 * rid + 1][threadIdx.x] += imp[1];
          cols[3 * rid + 2][threadIdx.x] += (gpos[0] - Bd->pos[0]) * imp[1] - (gpos[1] - Bd->pos[1]) * imp[0];
        }
    }
  }
  if (RIGID) imp_cols_to_row(cols, nb, rows + (size_t)blockIdx.x * DET_ROW);
}

__device__ __forceinline__ float weight_of(float rel, int k) {
  float w[3];
  weights(rel, w);
  return k == 0 ? w[0] : (k == 1 ? w[1] : w[2]);
}

// gather P2G.  Node (i, j) receives from the cells (i - a, j - b), a, b in 0..2; the sum runs over the cell rows in ascending
// order, inside a row over ascending keys, inside a cell in index order — fixed by the index alone.
template <bool RIGID>
__global__ __launch_bounds__(256) void k2d_gather(Params P, const uint32_t *__restrict__ start, const float4 *__restrict__ rec,
                                                  float *__restrict__ grid, RigidArgs2 R) {
  __shared__ float4 sh[3 * DET_CH];
  const int t = threadIdx.x, nx = P.res[0] + 1, ny = P.res[1] + 1;
  const int i = blockIdx.y * DET_TI + (t >> 6), j0 = blockIdx.x * DET_TJ, j = j0 + (t & 63);
  const bool node = i < nx && j < ny;
  uint32_t word = 0u;
  if (RIGID && node) word = node_word2(R, (size_t)i * ny + j);
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
  for (int rr = 0; rr < DET_TI + 2; rr++) {
    const int r = (int)blockIdx.y * DET_TI - 2 + rr;  // the cell row (uniform over the workgroup)
    if (r < 0 || r >= nx) continue;
    const size_t rowk = (size_t)r * ny;
    const uint32_t S = start[rowk + max(j0 - 2, 0)], E = start[rowk + min(j0 + DET_TJ, ny)];  // the tile's records of this row
    const int a = i - r;
    uint32_t lo = 0u, hi = 0u;  // this node's records of this row: the cells j - 2 .. j
    if (node && a >= 0 && a <= 2) { lo = start[rowk + max(j - 2, 0)]; hi = start[rowk + j + 1]; }
    for (uint32_t c0 = S; c0 < E; c0 += DET_CH) {
      const uint32_t cn = min((uint32_t)DET_CH, E - c0);
      __syncthreads();
      for (uint32_t q = t; q < 3u * cn; q += 256u) sh[q] = rec[3 * (size_t)c0 + q];
      __syncthreads();
      const uint32_t e1 = min(hi, c0 + cn);
      for (uint32_t e = max(lo, c0); e < e1; e++) {
        const float4 q0 = sh[3 * (e - c0)], q1 = sh[3 * (e - c0) + 1], q2 = sh[3 * (e - c0) + 2];
        if (RIGID && incompatible2(word, __float_as_uint(q2.y))) continue;  // the other side of a body receives nothing
        const int b = j - __float_as_int(q2.z);
        const float d0 = q0.x - (float)a, d1 = q0.y - (float)b, w = weight_of(q0.x, a) * weight_of(q0.y, b);
        s0 += w * (q0.z + q1.x * d0 + q1.y * d1);
        s1 += w * (q0.w + q1.z * d0 + q1.w * d1);
        s2 += w * q2.x;
      }
    }
  }
  if (node) {
    float *gp = grid + 3 * ((size_t)i * ny + j);
    gp[0] = s0; gp[1] = s1; gp[2] = s2;
  }
}

// G2P of a scene with bodies: lane s works on slot idx[s] in place; the penalty impulses go into the workgroup's row
__global__ __launch_bounds__(256) void k2d_g2p(Params P, LevelSetDev LS, const uint32_t *__restrict__ total, const uint32_t *__restrict__ idx,
                                               float *__restrict__ x, float *__restrict__ v, float *__restrict__ F, float *__restrict__ B,
                                               float *__restrict__ aux, const int32_t *__restrict__ gid, int32_t *__restrict__ pid,
                                               const GroupParams *__restrict__ groups, const float *__restrict__ grid,
                                               unsigned int *__restrict__ n_dead, RigidArgs2 R, int nb, float *__restrict__ rows) {
  __shared__ float cols[DET_ROW][256];
  imp_cols_clear(cols, nb);
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s < *total) g2p_particle<true>(P, LS, (int64_t)idx[s], x, v, F, B, aux, gid, pid, groups, grid, n_dead, R, &cols[0][threadIdx.x]);
  imp_cols_to_row(cols, nb, rows + (size_t)blockIdx.x * DET_ROW);
}

// one wave per body: lane l adds the rows l, l + 64, .. in ascending order, the 64 sums meet in a fixed butterfly
__global__ __launch_bounds__(64) void k2d_rows_apply(Rigid2 *rb, const float *__restrict__ rows, const uint32_t *__restrict__ total) {
  const int b = blockIdx.x + 1, l = threadIdx.x;
  const uint32_t nrows = (*total + 255u) / 256u;
  float s[3] = {0.0f, 0.0f, 0.0f};
  for (uint32_t r = l; r < nrows; r += 64u)
#pragma unroll
    for (int c = 0; c < 3; c++) s[c] += rows[(size_t)r * DET_ROW + 3 * b + c];
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int c = 0; c < 3; c++) s[c] += __shfl_xor(s[c], o);
  if (l == 0) {
    Rigid2 &Bd = rb[b];
    Bd.vel[0] += s[0] * Bd.inv_mass; Bd.vel[1] += s[1] * Bd.inv_mass;
    Bd.omega += Bd.inv_I * s[2];
  }
}

}  // namespace mpm2d
