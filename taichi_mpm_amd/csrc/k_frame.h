// taichi_mpm_amd/csrc/k_frame.h — the frame of a whole job: the rank of every live creation id among ALL live ids, on the device.
// write_partio orders the rows by creation id (src/visualize.cpp:17-100, the sort at :39-43).  Several ctx (the ranks of a tiled
// job) each hold a part of the ids, in any slot order; the row number of id p in the job's file is the number of live ids below p:
//   k_live_id_top      top = 1 + the largest live id
//   k_id_mark          bit p of a bitmap of ceil(top / 32) words for every live id p (every ctx marks the same bitmap)
//   k_id_prefix_*      prefix[w] = popcount of the words before w (three launches: sums, the scan of the sums, the add)
//   k_bgeo_rows_ranked row of id p at  prefix[p >> 5] + popc(bits[p >> 5] & ((1 << (p & 31)) - 1))
// No workgroup waits on another inside a kernel; every index derived from an id is checked against `top` before it is used.
// Compiled by k_frame.hip, a translation unit of its own (frame_launch.h says why); host driver: frame_job_api.h.  Part of libmpmhip;
// off the hot path.
#pragma once
#include "k_bgeo.h"
#include "frame_launch.h"

namespace mpm {

// 1 + the largest pid over the live slots -> *top (atomic max; the host zeroes it)
__global__ __launch_bounds__(FRAME_WG) void k_live_id_top(uint32_t n_slots, const RecG *__restrict__ rg, uint32_t *__restrict__ top) {
  uint32_t m = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += gridDim.x * blockDim.x) {
    const int32_t pid = rg[i].pid;
    if (pid >= 0) m = max(m, (uint32_t)pid + 1u);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor(m, o));
  __shared__ uint32_t wave_m[FRAME_WG / 64];
  if ((threadIdx.x & 63) == 0) wave_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t = max(max(wave_m[0], wave_m[1]), max(wave_m[2], wave_m[3]));
    if (t) atomicMax(top, t);
  }
}

// bit pid of bits[ceil(top / 32)] for every live slot; *live += the live slots.  The old value of the OR tells whether another slot,
// of this ctx or of one that marked before, holds the id already: err[FRAME_ERR_TWICE].  An id at or beyond top is not marked:
// err[FRAME_ERR_RANGE].
__global__ __launch_bounds__(FRAME_WG) void k_id_mark(uint32_t n_slots, const RecG *__restrict__ rg, uint32_t top, uint32_t *__restrict__ bits,
                                                      uint32_t *__restrict__ live, int32_t *__restrict__ err) {
  uint32_t mine = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += gridDim.x * blockDim.x) {
    const int32_t pid = rg[i].pid;
    if (pid < 0) continue;
    mine++;
    if ((uint32_t)pid >= top) { atomicMax(&err[FRAME_ERR_RANGE], pid); continue; }
    const uint32_t bit = 1u << (pid & 31);
    if (atomicOr(&bits[(uint32_t)pid >> 5], bit) & bit) atomicMax(&err[FRAME_ERR_TWICE], pid);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(live, mine);
}

// exclusive prefix of v over the workgroup's 256 threads, total = their sum (wave_sum: 4 words of LDS, free again on return)
__device__ __forceinline__ uint32_t frame_wg_exclusive(uint32_t v, uint32_t *wave_sum, uint32_t &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < FRAME_WG / 64; w++) {
    const uint32_t s = wave_sum[w];
    before += w < wave ? s : 0u;
    total += s;
  }
  __syncthreads();
  return before + inc - v;
}

// k_id_prefix, launch 1: sums[b] = set bits of the 256 words of workgroup b
__global__ __launch_bounds__(FRAME_WG) void k_id_prefix_sums(uint32_t n_words, const uint32_t *__restrict__ bits, uint32_t *__restrict__ sums) {
  __shared__ uint32_t wave_sum[FRAME_WG / 64];
  const uint32_t i = blockIdx.x * FRAME_WG + threadIdx.x;
  uint32_t total;
  frame_wg_exclusive(i < n_words ? (uint32_t)__popc(bits[i]) : 0u, wave_sum, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// launch 2, ONE workgroup: sums[0 .. n_blocks) -> their exclusive prefix in place, sums[n_blocks] = the number of set bits
__global__ __launch_bounds__(FRAME_WG) void k_id_prefix_scan(uint32_t n_blocks, uint32_t *__restrict__ sums) {
  __shared__ uint32_t wave_sum[FRAME_WG / 64];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n_blocks; base += FRAME_WG) {  // (uniform trip count: the scan synchronises the workgroup)
    const uint32_t i = base + threadIdx.x;
    uint32_t total;
    const uint32_t e = frame_wg_exclusive(i < n_blocks ? sums[i] : 0u, wave_sum, total);
    if (i < n_blocks) sums[i] = carry + e;
    carry += total;
  }
  if (threadIdx.x == 0) sums[n_blocks] = carry;
}
// launch 3: prefix[w] = set bits of the words before w
__global__ __launch_bounds__(FRAME_WG) void k_id_prefix_add(uint32_t n_words, const uint32_t *__restrict__ bits, const uint32_t *__restrict__ sums,
                                                            uint32_t *__restrict__ prefix) {
  __shared__ uint32_t wave_sum[FRAME_WG / 64];
  const uint32_t i = blockIdx.x * FRAME_WG + threadIdx.x;
  uint32_t total;
  const uint32_t e = frame_wg_exclusive(i < n_words ? (uint32_t)__popc(bits[i]) : 0u, wave_sum, total);
  if (i < n_words) prefix[i] = sums[blockIdx.x] + e;
}

// the number of set bits of (bits, prefix) below id p; false when bit p itself is not set
__device__ __forceinline__ bool frame_rank(const uint32_t *__restrict__ bits, const uint32_t *__restrict__ prefix, uint32_t p, uint32_t &j) {
  const uint32_t w = bits[p >> 5], bit = 1u << (p & 31);
  j = prefix[p >> 5] + (uint32_t)__popc(w & (bit - 1u));
  return (w & bit) != 0u;
}

// a lane per slot, records read in slot order; the row of a live slot (bgeo_row, k_bgeo.h: the words k_bgeo_rows writes) goes to
// rows[j], j = the rank of its id in (bits, prefix), which must hold fewer than n_rows ids (the host sized `rows` by their count).
// With row_index: row_index[j] = the rank of the id in (job_bits, job_prefix) — the ctx's rows compacted in its own bitmap, each
// with its row number in the job's file; an id the job's bitmap lacks: err[FRAME_ERR_ABSENT].
template <bool VERBOSE>
__global__ __launch_bounds__(FRAME_WG) void k_bgeo_rows_ranked(uint32_t n_slots, const RecG *__restrict__ rg, const RecP *__restrict__ rp,
                                                               const float *__restrict__ rb, const GroupParams *__restrict__ groups,
                                                               const int32_t *__restrict__ limits /* [slot][3] or nullptr */,
                                                               uint32_t top, const uint32_t *__restrict__ bits,
                                                               const uint32_t *__restrict__ prefix, uint32_t n_rows, uint32_t *__restrict__ rows,
                                                               const uint32_t *__restrict__ job_bits, const uint32_t *__restrict__ job_prefix,
                                                               uint32_t *__restrict__ row_index, int32_t *__restrict__ err) {
  constexpr int W = VERBOSE ? BGEO_W_VERBOSE : BGEO_W_PLAIN;
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_slots; s += gridDim.x * blockDim.x) {
    const RecG g = rg[s];
    if (g.pid < 0) continue;
    if ((uint32_t)g.pid >= top) { atomicMax(&err[FRAME_ERR_RANGE], g.pid); continue; }
    uint32_t j;
    if (!frame_rank(bits, prefix, (uint32_t)g.pid, j) || j >= n_rows) { atomicMax(&err[FRAME_ERR_ABSENT], g.pid); continue; }
    if (row_index) {
      uint32_t jj;
      if (!frame_rank(job_bits, job_prefix, (uint32_t)g.pid, jj)) { atomicMax(&err[FRAME_ERR_ABSENT], g.pid); continue; }
      row_index[j] = jj;
    }
    const RecP p = rp[s];
    bgeo_row<VERBOSE>(s, g, p, rb, groups, limits, rows + (size_t)j * W);
  }
}

}  // namespace mpm
