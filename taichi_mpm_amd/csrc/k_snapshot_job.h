// taichi_mpm_amd/csrc/k_snapshot_job.h — the snapshot of a whole tiled job, and a snapshot loaded brick by brick.
//   k_snap_rows_ranked  saving: the records of one ctx to their ranks (k_frame.h: the number of live ids of the JOB below each id) in
//                       the three sections of an MPMHIP01 blob (snapshot_blob.h) — the job's blob holds no dead slot and is in
//                       ascending creation id, whatever the bricks
//   k_snap_own_count    loading, over a staged chunk of a blob's RecG section: per workgroup the live records of its span whose base
//                       cell lies in this rank's brick (live_base_cell + owner_rank, the re-cut's rule: k_tiling.h); for the whole
//                       chunk the live records, those no rank can place, and the joint cell bounds of the placeable ones
//   k_snap_own_emit     ... the owned records of the span to the ctx's slots offs[workgroup] + (owned records before it in the span):
//                       blob order is kept, the ctx after a load is a function of (blob, partition, rank)
// A record is 11 float4 (RecG 4, RecP 4, apic_b row 3).  No lane moves a whole record: a group of four lanes owns one, lane q moves
// float4 q of RecG, of RecP and (q < 3) of the apic_b row, so a wave's loads cover 1 KB / 1 KB / 768 B of contiguous memory and its
// stores runs of 64 / 64 / 48 bytes.  Every index derived from an id is checked against `top`, every rank against the row count,
// every slot against the capacity, before use.  No workgroup waits on another.
// Compiled by k_frame.hip (snapshot_job_launch.h); host driver: snapshot_job_api.h.  Part of libmpmhip; off the hot path.
#pragma once
#include "k_frame.h"
#define MPM_TILING_RULES_ONLY  // of k_tiling.h: part_index, live_base_cell, owner_rank, bounds_epilogue — not its kernels
#include "k_tiling.h"
#include "snapshot_job_launch.h"

namespace mpm {

// Lane group g of four = slot, lane q of the group = float4 q.  Rows: out_rg / out_rp [n_rows][4], out_rb [n_rows][3] float4.  With
// job_bits: row_index[j] = the rank of the id in (job_bits, job_prefix), as k_bgeo_rows_ranked writes it.  Errors (lane 0 of the
// group): err[FRAME_ERR_RANGE] an id at or beyond top, err[FRAME_ERR_ABSENT] an id its bitmap lacks or a rank at or beyond n_rows.
__global__ __launch_bounds__(FRAME_WG) void k_snap_rows_ranked(uint32_t n_slots, const float4 *__restrict__ rg, const float4 *__restrict__ rp,
                                                               const float4 *__restrict__ rb, uint32_t top, const uint32_t *__restrict__ bits,
                                                               const uint32_t *__restrict__ prefix, uint32_t n_rows, float4 *__restrict__ out_rg,
                                                               float4 *__restrict__ out_rp, float4 *__restrict__ out_rb,
                                                               const uint32_t *__restrict__ job_bits, const uint32_t *__restrict__ job_prefix,
                                                               uint32_t *__restrict__ row_index, int32_t *__restrict__ err) {
  const uint64_t n_items = (uint64_t)n_slots * 4u, stride = (uint64_t)gridDim.x * FRAME_WG;
  const uint32_t q = threadIdx.x & 3u;
  // (uniform trip count per workgroup: the shuffle below needs the whole lane group; n_items is a multiple of 4)
  for (uint64_t first = (uint64_t)blockIdx.x * FRAME_WG; first < n_items; first += stride) {
    const uint64_t e = first + threadIdx.x;
    float4 g = make_float4(0.0f, 0.0f, __int_as_float(-1), 0.0f);
    if (e < n_items) g = rg[e];
    const int32_t pid = __shfl(__float_as_int(g.z), (int)((threadIdx.x & 63u) | 3u));  // (RecG.pid: word 2 of float4 3)
    bool ok = e < n_items && pid >= 0;
    if (ok && (uint32_t)pid >= top) {
      if (q == 0) atomicMax(&err[FRAME_ERR_RANGE], pid);
      ok = false;
    }
    uint32_t j = 0;
    if (ok && (!frame_rank(bits, prefix, (uint32_t)pid, j) || j >= n_rows)) {
      if (q == 0) atomicMax(&err[FRAME_ERR_ABSENT], pid);
      ok = false;
    }
    if (ok && job_bits) {
      uint32_t jj = 0;
      if (!frame_rank(job_bits, job_prefix, (uint32_t)pid, jj)) {
        if (q == 0) atomicMax(&err[FRAME_ERR_ABSENT], pid);
        ok = false;
      } else if (q == 0) {
        row_index[j] = jj;
      }
    }
    if (ok) {
      const uint64_t s = e >> 2;
      out_rg[(size_t)j * 4 + q] = g;
      out_rp[(size_t)j * 4 + q] = rp[e];
      if (q < 3) out_rb[(size_t)j * 3 + q] = rb[s * 3 + q];
    }
  }
}

// is record i of the staged RecG section live, and does this rank own it?  placeable: live and live_base_cell accepts it
__device__ __forceinline__ bool snap_owned(const Params &P, const Tiling &T, const float4 *__restrict__ rg, uint32_t i, bool &live, bool &placeable,
                                           int b[3]) {
  live = __float_as_int(rg[(size_t)i * 4 + 3].z) >= 0;
  placeable = live && live_base_cell(P, rg[(size_t)i * 4], b);
  return placeable && owner_rank(T, b) == T.rank;
}

// a lane per record, SNAP_SPAN records per workgroup: totals[workgroup] = owned records of the span; small[SNAP_W_LIVE] += live records,
// small[SNAP_W_LOST] += live records live_base_cell rejects, small[SNAP_W_BOUNDS ..] = min / max + 1 of the base cells of ALL placeable
// records (every rank computes the same six words from the same blob)
__global__ __launch_bounds__(256) void k_snap_own_count(Params P, Tiling T, uint32_t n, const float4 *__restrict__ rg, uint32_t *__restrict__ totals,
                                                        uint32_t *__restrict__ small) {
  __shared__ uint32_t wave_n[4][3];
  int lo[3] = {1 << 30, 1 << 30, 1 << 30}, hi[3] = {-1, -1, -1};
  uint32_t own = 0, alive = 0, lost = 0;
#pragma unroll
  for (int k = 0; k < SNAP_SPAN / 256; k++) {
    const uint32_t i = blockIdx.x * (uint32_t)SNAP_SPAN + (uint32_t)k * 256u + threadIdx.x;
    if (i >= n) continue;
    bool live, placeable;
    int b[3];
    own += snap_owned(P, T, rg, i, live, placeable, b) ? 1u : 0u;
    alive += live ? 1u : 0u;
    lost += live && !placeable ? 1u : 0u;
    if (placeable) {
#pragma unroll
      for (int a = 0; a < 3; a++) { lo[a] = min(lo[a], b[a]); hi[a] = max(hi[a], b[a] + 1); }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    own += __shfl_xor(own, o);
    alive += __shfl_xor(alive, o);
    lost += __shfl_xor(lost, o);
  }
  if ((threadIdx.x & 63) == 0) {
    wave_n[threadIdx.x >> 6][0] = own; wave_n[threadIdx.x >> 6][1] = alive; wave_n[threadIdx.x >> 6][2] = lost;
  }
  bounds_epilogue(lo, hi, reinterpret_cast<int *>(small + SNAP_W_BOUNDS));  // (synchronises the workgroup: wave_n is complete behind it)
  if (threadIdx.x == 0) {
    totals[blockIdx.x] = wave_n[0][0] + wave_n[1][0] + wave_n[2][0] + wave_n[3][0];
    const uint32_t a = wave_n[0][1] + wave_n[1][1] + wave_n[2][1] + wave_n[3][1], l = wave_n[0][2] + wave_n[1][2] + wave_n[2][2] + wave_n[3][2];
    if (a) atomicAdd(&small[SNAP_W_LIVE], a);
    if (l) atomicAdd(&small[SNAP_W_LOST], l);
  }
}

// 64 records a round, a lane group of four per record (k_snap_rows_ranked's layout); the rank of an owned record inside the span by
// ballot and popcount: bit 4 g of the ballot word speaks for lane group g, the waves' sums go through four words of LDS.  offs =
// the exclusive scan of k_snap_own_count's totals, at this chunk's first workgroup.  A slot at or beyond cap is not written:
// small[SNAP_W_ERR] (the host sized the ctx by the scan's total, so this says the blob changed between the passes).
__global__ __launch_bounds__(256) void k_snap_own_emit(Params P, Tiling T, uint32_t n, const float4 *__restrict__ rg, const float4 *__restrict__ rp,
                                                       const float4 *__restrict__ rb, const uint32_t *__restrict__ offs, uint32_t cap,
                                                       float4 *__restrict__ out_rg, float4 *__restrict__ out_rp, float4 *__restrict__ out_rb,
                                                       uint32_t *__restrict__ small) {
  __shared__ uint32_t wave_own[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, q = threadIdx.x & 3u;
  const uint32_t first = blockIdx.x * (uint32_t)SNAP_SPAN;
  uint32_t at = offs[blockIdx.x];
  for (uint32_t k = 0; k < (uint32_t)SNAP_SPAN && first + k < n; k += 64u) {  // (uniform per workgroup)
    const uint32_t i = first + k + (threadIdx.x >> 2);
    bool live, placeable, own = false;
    int b[3];
    if (i < n) own = snap_owned(P, T, rg, i, live, placeable, b);
    const unsigned long long m = __ballot(own) & 0x1111111111111111ull;
    const uint32_t below = (uint32_t)__popcll(m & ((1ull << (lane & ~3u)) - 1ull));
    if (lane == 0) wave_own[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) {
      const uint32_t s = wave_own[w];
      before += w < wave ? s : 0u;
      total += s;
    }
    __syncthreads();
    if (own) {
      const uint32_t d = at + before + below;
      if (d < cap) {
        out_rg[(size_t)d * 4 + q] = rg[(size_t)i * 4 + q];
        out_rp[(size_t)d * 4 + q] = rp[(size_t)i * 4 + q];
        if (q < 3) out_rb[(size_t)d * 3 + q] = rb[(size_t)i * 3 + q];
      } else if (q == 0) {
        atomicMax(reinterpret_cast<int32_t *>(&small[SNAP_W_ERR]), (int32_t)min(d, 0x7fffffffu));
      }
    }
    at += total;
  }
}

}  // namespace mpm
