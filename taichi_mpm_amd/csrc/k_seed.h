// taichi_mpm_amd/csrc/k_seed.h — kernels of mpmhip_seed_particles (D = 3) and mpmhip2d_seed_particles (D = 2) (rules: include/mpmhip.h;
// host side: seed_api.h).  Part of libmpmhip.  One lane per candidate c = tile point * n_replicas + replica; three passes over the
// candidates' workgroups:
//   k_seed_bounds  "get ready": the box of the grid's cell centres inside the region (integer min / max: order-free)
//   k_seed_count   the acceptance test; a wave's ballot is stored as one 64-bit word per 64 candidates, a workgroup's popcount as its total
//   k_seed_scan    exclusive scan of the workgroup totals (one workgroup)
//   k_seed_write   reads the ballot words back — the test is not evaluated twice — and hands every survivor with its rank to a sink
// The rank of a survivor is the number of survivors with a smaller c: the order is the reference's and does not depend on scheduling.
// A rank of a tiled job (mpmhip_seed_particles_brick) runs the same three passes over ALL candidates with a second ballot, "this
// survivor's base cell lies in my brick", and a scan of two sums: k_seed_count_brick, k_seed_scan2, k_seed_write_brick.  A survivor's
// id comes from its global rank, its slot from its rank among this brick's survivors, so the ranks of a job agree on every id
// without a message.  k_seed_hist counts the survivors' base cells per axis (mpmhip_seed_histogram: the partition's input).
// The candidate arithmetic is written once for both dimensions.  What differs comes in as a template argument: the region (where a
// point is inside: SeedRegion, SeedRegion2) and the sink (how a ctx stores a particle: SeedSink3, SeedSink2).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "mpm_common.h"

namespace mpm {

// no multiply-add of the candidate arithmetic may be fused: tests/seed_model.py and tests/seed2d_model.py reproduce the positions to
// the bit (a sampled region's field is read by mpm_math.h's sampler, which forbids the same for itself)
#define SEED_NO_CONTRACT _Pragma("clang fp contract(off)")

constexpr int SEED_WG = 256;            // lanes per workgroup
constexpr int SEED_ROUNDS = 4;          // candidates per lane: round j of workgroup w holds c = 1024 w + 256 j + lane
constexpr int SEED_PER_WG = SEED_WG * SEED_ROUNDS;
constexpr int SEED_WORDS = SEED_PER_WG / 64;  // ballot words per workgroup
constexpr int SEED_SCAN_WG = 1024;

// where a region's level set is negative: shapes, or (sdf.phi0 != null) one frame of a sampled field read by the boundary's own
// sampler (mpm_math.h: sdf_locate, sdf_phi_frame), so the seeding and the boundary decide alike for one array
struct SeedRegion {
  int n_shapes;
  ShapeDev s[MPMHIP_MAX_SHAPES];
  SdfDev sdf;

  __device__ __forceinline__ bool inside(const float x[3], float idx) const {
    if (sdf.phi0) {
      int c[3];
      float f[3];
      if (!sdf_locate<3>(sdf, x, c, f)) return false;  // outside the lattice: not in the region
      return sdf_phi_frame<3>(sdf, sdf.phi0, c, f) < 0.0f;
    }
    float phi, n[3];
    return levelset_eval_key(s, n_shapes, x, idx, phi, n) && phi < 0.0f;
  }
};

// the same in the plane: shapes read as mpmhip2d_set_levelset stores them, or a field phi [res0][res1]
struct SeedRegion2 {
  int n_shapes;
  ShapeDev s[MPMHIP_MAX_SHAPES];
  SdfDev sdf;

  __device__ __forceinline__ bool inside(const float x[2], float idx) const {
    if (sdf.phi0) {
      int c[2];
      float f[2];
      if (!sdf_locate<2>(sdf, x, c, f)) return false;
      return sdf_phi_frame<2>(sdf, sdf.phi0, c, f) < 0.0f;
    }
    const float xw[3] = {x[0], x[1], 0.0f};
    float phi, n[3];
    return levelset_eval_key(s, n_shapes, xw, idx, phi, n) && phi < 0.0f;
  }
};

template <int D>
struct SeedParams {
  int res[D];
  float dx, idx;
  float min_corner[D];
  float min_distance, region_size;
  uint32_t nrep[D];  // replicas per axis; the replica index counts the last axis fastest
  uint32_t n_rep, n_tile, n_cand;
  int source;
  float offset[D];     // source: velocity * current_t
  float advection[D];  // source: where a particle is one source_delta_t later
  // what every particle takes (a sink stores them)
  float velocity[D];
  float dg, aux;
  int32_t gid, pid0;
};

// MPM::near_boundary (src/mpm.h:269-276), the expressions of particle_key
template <int D>
__device__ __forceinline__ bool seed_near_boundary(const SeedParams<D> &S, const float x[D]) {
  SEED_NO_CONTRACT
  float mn = 0.0f, mx = 0.0f;
#pragma unroll
  for (int d = 0; d < D; d++) {  // (min and max are exact: any association)
    const float X = x[d] * S.idx, Y = X - (float)S.res[d];
    mn = d ? fminf(mn, X) : X;
    mx = d ? fmaxf(mx, Y) : Y;
  }
  return mn < 7.0f || mx > -7.0f;
}

// position of candidate c (sample_from_periodic_data :177-185, sample_from_source :232-243)
template <int D>
__device__ __forceinline__ void seed_position(const SeedParams<D> &S, const float *__restrict__ tile, uint32_t c, float x[D]) {
  SEED_NO_CONTRACT
  const uint32_t i = c / S.n_rep;
  uint32_t r = c - i * S.n_rep;
  int ind[D];
#pragma unroll
  for (int d = D - 1; d > 0; d--) {
    const uint32_t up = r / S.nrep[d];
    ind[d] = (int)(r - up * S.nrep[d]);
    r = up;
  }
  ind[0] = (int)r;
#pragma unroll
  for (int d = 0; d < D; d++) {
    float q = tile[D * (size_t)i + d] * S.min_distance;
    if (S.source) {
      q = q + S.offset[d];
      const float w = floorf(q / S.region_size + 0.5f);
      q = q - w * S.region_size;
    }
    const float a = q + S.min_corner[d];
    const float b = S.region_size * ((float)ind[d] + 0.5f);
    x[d] = a + b;
  }
}

// the acceptance test of candidate c; x = its position
template <int D, class Region>
__device__ __forceinline__ bool seed_keep_at(const Region &R, const SeedParams<D> &S, const float *__restrict__ tile, uint32_t c, float x[D]) {
  SEED_NO_CONTRACT
  float y[D];
  seed_position<D>(S, tile, c, x);
  if (!R.inside(x, S.idx) || seed_near_boundary<D>(S, x)) return false;
  if (!S.source) return true;
#pragma unroll
  for (int d = 0; d < D; d++) y[d] = x[d] + S.advection[d];
  return !R.inside(y, S.idx);
}
template <int D, class Region>
__device__ __forceinline__ bool seed_keep(const Region &R, const SeedParams<D> &S, const float *__restrict__ tile, uint32_t c) {
  float x[D];
  return seed_keep_at<D>(R, S, tile, c, x);
}

// The bricks of a tiled job as the seeding kernels take them (of Tiling: the whole struct costs ~80 SGPRs more).  A particle belongs
// to the brick that holds its base cell b[k] = (int)fl(fl(x[k] * idx) - 0.5f) — dest_rank of k_tiling.h, here with nothing contracted:
// tiled.base_cells and Partition.rank_of_cells restate it to the bit.  Should the compiler contract the migration's own expression
// differently for a particle at an exact cell face, that particle simply migrates at the next check (it is within the margin).
// A survivor's x * idx is >= 7 (seed_near_boundary), so the base cell is never negative.
struct SeedBricks {
  int rank;
  int dims[3];
  int cuts[3][MPMHIP_MAX_PARTS + 1];
};
template <int D>
__device__ __forceinline__ void seed_base_cell(const SeedParams<D> &S, const float x[D], int b[D]) {
  SEED_NO_CONTRACT
#pragma unroll
  for (int k = 0; k < D; k++) {
    const float X = x[k] * S.idx;
    b[k] = (int)(X - 0.5f);
  }
}
__device__ __forceinline__ int seed_part_index(const int *cuts, int n, int c) {  // (part_index of k_tiling.h)
  int p = 0;
  while (p + 1 < n && c >= cuts[p + 1]) p++;
  return p;
}
__device__ __forceinline__ int seed_owner(const SeedParams<3> &S, const SeedBricks &K, const float x[3]) {
  int b[3];
  seed_base_cell<3>(S, x, b);
  return (seed_part_index(K.cuts[0], K.dims[0], b[0]) * K.dims[1] + seed_part_index(K.cuts[1], K.dims[1], b[1])) * K.dims[2] +
         seed_part_index(K.cuts[2], K.dims[2], b[2]);
}

__device__ __forceinline__ int seed_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int seed_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// box[0..D-1] = min cell index per axis of the cell centres inside the region (INT_MAX: none), box[D..2D-1] = max (-1: none)
template <int D, class Region>
__global__ __launch_bounds__(SEED_WG) void k_seed_bounds(Region R, SeedParams<D> S, int *__restrict__ box) {
  SEED_NO_CONTRACT
  using Count = std::conditional_t<D == 2, uint32_t, uint64_t>;  // of cells (2D: res <= 16384 per axis, below 2^32)
  Count rest = 1;  // cells per index of axis 0
#pragma unroll
  for (int d = 1; d < D; d++) rest *= (Count)S.res[d];
  const Count total = (Count)S.res[0] * rest;
  int lo[D], hi[D];
#pragma unroll
  for (int d = 0; d < D; d++) { lo[d] = 0x7fffffff; hi[d] = -1; }
  for (Count n = (Count)blockIdx.x * SEED_WG + threadIdx.x; n < total; n += (Count)gridDim.x * SEED_WG) {
    int cell[D];
    cell[0] = (int)(n / rest);
    uint32_t rem = (uint32_t)(n - (Count)cell[0] * rest);
#pragma unroll
    for (int d = D - 1; d > 0; d--) {
      const uint32_t up = rem / (uint32_t)S.res[d];
      cell[d] = (int)(rem - up * (uint32_t)S.res[d]);
      rem = up;
    }
    float x[D];
#pragma unroll
    for (int d = 0; d < D; d++) x[d] = ((float)cell[d] + 0.5f) * S.dx;
    if (R.inside(x, S.idx)) {
#pragma unroll
      for (int d = 0; d < D; d++) { lo[d] = min(lo[d], cell[d]); hi[d] = max(hi[d], cell[d]); }
    }
  }
#pragma unroll
  for (int d = 0; d < D; d++) {
    const int a = seed_wave_min(lo[d]), b = seed_wave_max(hi[d]);
    if ((threadIdx.x & 63) == 0 && b >= 0) { atomicMin(&box[d], a); atomicMax(&box[D + d], b); }
  }
}

template <int D, class Region>
__global__ __launch_bounds__(SEED_WG) void k_seed_count(Region R, SeedParams<D> S, const float *__restrict__ tile,
                                                        unsigned long long *__restrict__ words, uint32_t *__restrict__ totals) {
  __shared__ uint32_t wave_cnt[SEED_WG / 64];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t cnt = 0;
#pragma unroll
  for (int j = 0; j < SEED_ROUNDS; j++) {
    const uint32_t c = blockIdx.x * (uint32_t)SEED_PER_WG + (uint32_t)j * SEED_WG + threadIdx.x;
    const bool keep = c < S.n_cand && seed_keep<D>(R, S, tile, c);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) words[(size_t)blockIdx.x * SEED_WORDS + j * (SEED_WG / 64) + wave] = m;
    cnt += (uint32_t)__popcll(m);
  }
  if (lane == 0) wave_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) totals[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// totals[n] -> exclusive prefix in place, the sum to *total.  One workgroup: lane t owns a contiguous run of the array.
__global__ __launch_bounds__(SEED_SCAN_WG) void k_seed_scan(uint32_t *__restrict__ totals, uint32_t n, uint32_t *__restrict__ total) {
  __shared__ uint32_t part[SEED_SCAN_WG];
  const uint32_t per = (n + SEED_SCAN_WG - 1) / SEED_SCAN_WG;
  const uint32_t lo = min(threadIdx.x * per, n), hi = min(lo + per, n);
  uint32_t s = 0;
  for (uint32_t i = lo; i < hi; i++) s += totals[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (uint32_t o = 1; o < SEED_SCAN_WG; o <<= 1) {  // inclusive scan of the lanes' sums
    const uint32_t v = threadIdx.x >= o ? part[threadIdx.x - o] : 0u;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t run = part[threadIdx.x] - s;
  for (uint32_t i = lo; i < hi; i++) {
    const uint32_t v = totals[i];
    totals[i] = run;
    run += v;
  }
  if (threadIdx.x == SEED_SCAN_WG - 1) *total = part[threadIdx.x];
}

// k_seed_count with a second ballot per round: `mine` = a survivor whose base cell lies in brick K.rank.  totals[w] = the workgroup's
// survivors in the low word, those of this brick in the high word (both below 2^31 over all workgroups: one 64-bit sum carries both).
template <int D, class Region>
__global__ __launch_bounds__(SEED_WG) void k_seed_count_brick(Region R, SeedParams<D> S, SeedBricks K, const float *__restrict__ tile,
                                                              unsigned long long *__restrict__ words, unsigned long long *__restrict__ words_mine,
                                                              unsigned long long *__restrict__ totals) {
  __shared__ unsigned long long wave_cnt[SEED_WG / 64];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t cnt = 0, cnt_mine = 0;
#pragma unroll
  for (int j = 0; j < SEED_ROUNDS; j++) {
    const uint32_t c = blockIdx.x * (uint32_t)SEED_PER_WG + (uint32_t)j * SEED_WG + threadIdx.x;
    float x[D];
    const bool keep = c < S.n_cand && seed_keep_at<D>(R, S, tile, c, x);
    const bool mine = keep && seed_owner(S, K, x) == K.rank;
    const unsigned long long m = __ballot(keep), mm = __ballot(mine);
    if (lane == 0) {
      const size_t at = (size_t)blockIdx.x * SEED_WORDS + j * (SEED_WG / 64) + wave;
      words[at] = m;
      words_mine[at] = mm;
    }
    cnt += (uint32_t)__popcll(m);
    cnt_mine += (uint32_t)__popcll(mm);
  }
  if (lane == 0) wave_cnt[wave] = (unsigned long long)cnt | ((unsigned long long)cnt_mine << 32);
  __syncthreads();
  if (threadIdx.x == 0) totals[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// k_seed_scan over the two sums of k_seed_count_brick at once (neither half carries into the other)
__global__ __launch_bounds__(SEED_SCAN_WG) void k_seed_scan2(unsigned long long *__restrict__ totals, uint32_t n, unsigned long long *__restrict__ total) {
  __shared__ unsigned long long part[SEED_SCAN_WG];
  const uint32_t per = (n + SEED_SCAN_WG - 1) / SEED_SCAN_WG;
  const uint32_t lo = min(threadIdx.x * per, n), hi = min(lo + per, n);
  unsigned long long s = 0;
  for (uint32_t i = lo; i < hi; i++) s += totals[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (uint32_t o = 1; o < SEED_SCAN_WG; o <<= 1) {  // inclusive scan of the lanes' sums
    const unsigned long long v = threadIdx.x >= o ? part[threadIdx.x - o] : 0ull;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  unsigned long long run = part[threadIdx.x] - s;
  for (uint32_t i = lo; i < hi; i++) {
    const unsigned long long v = totals[i];
    totals[i] = run;
    run += v;
  }
  if (threadIdx.x == SEED_SCAN_WG - 1) *total = part[threadIdx.x];
}

// Per-axis histograms of the survivors' base cells: hist[offset of axis a + cell], integer counts — exact, whatever the order.  A
// workgroup walks its share of the candidates (a grid-stride loop over chunks of SEED_WG), counts into rows of its own in LDS
// (use_lds: the D rows fit) and adds its nonzero bins to the global rows once at the end: one global atomic per workgroup and
// occupied bin.  Where the rows do not fit, every survivor adds to the global rows itself (the 3D ctx holds res <= 1000 per axis, 12 KB
// of rows at most: its calls always take the LDS path).
template <int D, class Region>
__global__ __launch_bounds__(SEED_WG) void k_seed_hist(Region R, SeedParams<D> S, const float *__restrict__ tile, uint32_t n_chunks,
                                                       int use_lds, uint32_t *__restrict__ hist) {
  extern __shared__ uint32_t seed_rows[];
  uint32_t off[D + 1];
  off[0] = 0;
#pragma unroll
  for (int k = 0; k < D; k++) off[k + 1] = off[k] + (uint32_t)S.res[k];
  if (use_lds) {
    for (uint32_t i = threadIdx.x; i < off[D]; i += SEED_WG) seed_rows[i] = 0;
    __syncthreads();
  }
  for (uint32_t q = blockIdx.x; q < n_chunks; q += gridDim.x) {
    const uint32_t c = q * (uint32_t)SEED_WG + threadIdx.x;
    float x[D];
    if (c < S.n_cand && seed_keep_at<D>(R, S, tile, c, x)) {
      int b[D];
      seed_base_cell<D>(S, x, b);
#pragma unroll
      for (int k = 0; k < D; k++) {
        const uint32_t at = off[k] + (uint32_t)min(max(b[k], 0), S.res[k] - 1);  // (a survivor's base cell is inside the grid: the clamp only guards the rows)
        if (use_lds) atomicAdd(&seed_rows[at], 1u);
        else atomicAdd(&hist[at], 1u);
      }
    }
  }
  if (use_lds) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < off[D]; i += SEED_WG) {
      const uint32_t v = seed_rows[i];
      if (v) atomicAdd(&hist[i], v);
    }
  }
}

// the 3D ctx's records behind its resident ones: RecG / RecP / apic_b rows, 11 float4 stores per particle
struct SeedSink3 {
  float4 *__restrict__ rg, *__restrict__ rp, *__restrict__ rb;
  float mass;
  __device__ __forceinline__ void store(const SeedParams<3> &S, uint32_t rank, const float x[3]) const {
    float4 *g = rg + 4 * (size_t)rank, *p = rp + 4 * (size_t)rank, *b = rb + 3 * (size_t)rank;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    g[0] = make_float4(x[0], x[1], x[2], S.aux);                       // RecG {x3, aux, F9, gid, pid, pad}
    g[1] = make_float4(S.dg, 0.0f, 0.0f, 0.0f);
    g[2] = make_float4(S.dg, 0.0f, 0.0f, 0.0f);
    g[3] = make_float4(S.dg, __int_as_float(S.gid), __int_as_float(S.pid0 + (int32_t)rank), 0.0f);
    p[0] = make_float4(x[0], x[1], x[2], S.velocity[0]);               // RecP {x3, v3, A9, mass}
    p[1] = make_float4(S.velocity[1], S.velocity[2], 0.0f, 0.0f);
    p[2] = zero;
    p[3] = make_float4(0.0f, 0.0f, 0.0f, mass);
    b[0] = zero; b[1] = zero; b[2] = zero;                             // apic_b
  }
  // The same rows with slot and creation id apart (a rank of a tiled job: the slot counts this brick's survivors, the id all of
  // them).  `store` does not go through it: k_seed_write stays instruction for instruction what it was (profiles/kernel_diff.py).
  __device__ __forceinline__ void store_at(const SeedParams<3> &S, uint32_t slot, int32_t pid, const float x[3]) const {
    float4 *g = rg + 4 * (size_t)slot, *p = rp + 4 * (size_t)slot, *b = rb + 3 * (size_t)slot;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    g[0] = make_float4(x[0], x[1], x[2], S.aux);
    g[1] = make_float4(S.dg, 0.0f, 0.0f, 0.0f);
    g[2] = make_float4(S.dg, 0.0f, 0.0f, 0.0f);
    g[3] = make_float4(S.dg, __int_as_float(S.gid), __int_as_float(pid), 0.0f);
    p[0] = make_float4(x[0], x[1], x[2], S.velocity[0]);
    p[1] = make_float4(S.velocity[1], S.velocity[2], 0.0f, 0.0f);
    p[2] = zero;
    p[3] = make_float4(0.0f, 0.0f, 0.0f, mass);
    b[0] = zero; b[1] = zero; b[2] = zero;
  }
};

// the 2D ctx's SoA arrays from their first free slot: x, v as float2, F, B as float4, aux, gid, pid as words; consecutive ranks
// write consecutive addresses of every array
struct SeedSink2 {
  float2 *__restrict__ x, *__restrict__ v;
  float4 *__restrict__ F, *__restrict__ B;
  float *__restrict__ aux;
  int32_t *__restrict__ gid, *__restrict__ pid;
  __device__ __forceinline__ void store(const SeedParams<2> &S, uint32_t rank, const float p[2]) const {
    x[rank] = make_float2(p[0], p[1]);
    v[rank] = make_float2(S.velocity[0], S.velocity[1]);
    F[rank] = make_float4(S.dg, 0.0f, 0.0f, S.dg);
    B[rank] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    aux[rank] = S.aux;
    gid[rank] = S.gid;
    pid[rank] = S.pid0 + (int32_t)rank;
  }
};

template <int D, class Sink>
__global__ __launch_bounds__(SEED_WG) void k_seed_write(SeedParams<D> S, const float *__restrict__ tile,
                                                        const unsigned long long *__restrict__ words, const uint32_t *__restrict__ offs,
                                                        Sink sink) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long *w = words + (size_t)blockIdx.x * SEED_WORDS;
  uint32_t before = offs[blockIdx.x];  // survivors in front of this wave's word of round j
  for (uint32_t q = 0; q < wave; q++) before += (uint32_t)__popcll(w[q]);
#pragma unroll
  for (int j = 0; j < SEED_ROUNDS; j++) {
    const uint32_t word = (uint32_t)j * (SEED_WG / 64) + wave;
    const unsigned long long m = w[word];
    if ((m >> lane) & 1ull) {
      const uint32_t rank = before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      const uint32_t c = blockIdx.x * (uint32_t)SEED_PER_WG + (uint32_t)j * SEED_WG + threadIdx.x;
      float x[D];
      seed_position<D>(S, tile, c, x);
      sink.store(S, rank, x);
    }
    // the words of this round behind this wave's, and those of the next round in front of it
    for (uint32_t q = word; q < word + SEED_WG / 64; q++)
      if (q < SEED_WORDS) before += (uint32_t)__popcll(w[q]);
  }
}

// k_seed_write for one brick: a survivor with its bit in words_mine goes to slot (survivors of this brick in front of it) with the id
// pid0 + (survivors of the job in front of it); offs = the prefixes of k_seed_scan2 (low word the job's, high word the brick's)
template <int D, class Sink>
__global__ __launch_bounds__(SEED_WG) void k_seed_write_brick(SeedParams<D> S, const float *__restrict__ tile,
                                                              const unsigned long long *__restrict__ words,
                                                              const unsigned long long *__restrict__ words_mine,
                                                              const unsigned long long *__restrict__ offs, Sink sink) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long *w = words + (size_t)blockIdx.x * SEED_WORDS, *wm = words_mine + (size_t)blockIdx.x * SEED_WORDS;
  const unsigned long long o = offs[blockIdx.x];
  uint32_t before = (uint32_t)o, before_mine = (uint32_t)(o >> 32);  // in front of this wave's word of round j
  for (uint32_t q = 0; q < wave; q++) { before += (uint32_t)__popcll(w[q]); before_mine += (uint32_t)__popcll(wm[q]); }
#pragma unroll
  for (int j = 0; j < SEED_ROUNDS; j++) {
    const uint32_t word = (uint32_t)j * (SEED_WG / 64) + wave;
    const unsigned long long m = w[word], mm = wm[word];
    if ((mm >> lane) & 1ull) {
      const unsigned long long below = (1ull << lane) - 1ull;
      const uint32_t rank = before + (uint32_t)__popcll(m & below), slot = before_mine + (uint32_t)__popcll(mm & below);
      const uint32_t c = blockIdx.x * (uint32_t)SEED_PER_WG + (uint32_t)j * SEED_WG + threadIdx.x;
      float x[D];
      seed_position<D>(S, tile, c, x);
      sink.store_at(S, slot, S.pid0 + (int32_t)rank, x);
    }
    for (uint32_t q = word; q < word + SEED_WG / 64; q++)
      if (q < SEED_WORDS) { before += (uint32_t)__popcll(w[q]); before_mine += (uint32_t)__popcll(wm[q]); }
  }
}

#undef SEED_NO_CONTRACT

// what a ctx of either dimension keeps between seeding calls (host side; an emitter calls before every frame): buffers only grow
struct SeedWork {
  DevBuf<float> d_tile;  // the periodic tile, [n_tile][D]
  uint32_t n_tile = 0;
  DevBuf<unsigned long long> d_words;  // [workgroups][SEED_WORDS] ballots of the acceptance test
  DevBuf<uint32_t> d_totals;           // [workgroups] survivors per workgroup, then their exclusive prefix
  size_t wg_cap = 0;
  DevBuf<int> d_box;                   // [2 D] get-ready box, then as uint32 the survivors' count
  DevBuf<float> d_phi;                 // a sampled region's field
  size_t phi_cap = 0;
  // a rank of a tiled job (mpmhip_seed_particles_brick) and mpmhip_seed_histogram
  DevBuf<unsigned long long> d_words_mine;  // [workgroups][SEED_WORDS] ballots of "a survivor of this brick"
  DevBuf<unsigned long long> d_totals2;     // [workgroups + 1] the two sums per workgroup, then their prefixes; the last word their totals
  size_t wg_cap2 = 0;
  DevBuf<uint32_t> d_hist;                  // [sum of res] the histogram rows
  size_t hist_cap = 0;
};

}  // namespace mpm
