// taichi_mpm_amd/csrc/k_seed.h — kernels of mpmhip_seed_particles (rules: include/mpmhip.h; host side: seed_api.h)
// Part of libmpmhip.  One lane per candidate c = tile point * n_replicas + replica; three passes over the candidates' workgroups:
//   k_seed_bounds  "get ready": the box of the grid's cell centres inside the region (integer min / max: order-free)
//   k_seed_count   the acceptance test; a wave's ballot is stored as one 64-bit word per 64 candidates, a workgroup's popcount as its total
//   k_seed_scan    exclusive scan of the workgroup totals (one workgroup)
//   k_seed_write   reads the ballot words back — the test is not evaluated twice — and writes RecG / RecP / apic_b rows of the
//                  survivors at their rank, 11 float4 stores per particle
// The rank of a survivor is the number of survivors with a smaller c: the order is the reference's and does not depend on scheduling.
#pragma once
#include <hip/hip_runtime.h>

#include "mpm_common.h"

namespace mpm {

// no multiply-add of the candidate arithmetic may be fused: tests/seed_model.py reproduces the positions to the bit
#define SEED_NO_CONTRACT _Pragma("clang fp contract(off)")

constexpr int SEED_WG = 256;            // lanes per workgroup
constexpr int SEED_ROUNDS = 4;          // candidates per lane: round j of workgroup w holds c = 1024 w + 256 j + lane
constexpr int SEED_PER_WG = SEED_WG * SEED_ROUNDS;
constexpr int SEED_WORDS = SEED_PER_WG / 64;  // ballot words per workgroup
constexpr int SEED_SCAN_WG = 1024;

// where the region's level set is negative: shapes, or (sdf.phi0 != null) one sampled frame
struct SeedRegion {
  int n_shapes;
  ShapeDev s[MPMHIP_MAX_SHAPES];
  SdfDev sdf;
};

struct SeedParams {
  int res[3];
  float dx, idx;
  float min_corner[3];
  float min_distance, region_size;
  int nrep[3];
  uint32_t n_rep, n_tile, n_cand;
  int source;
  float offset[3];     // source: velocity * current_t
  float advection[3];  // source: where a particle is one source_delta_t later
  // what the records take
  float velocity[3];
  float dg, aux, mass;
  uint32_t gid;
  int32_t pid0;
};

__device__ __forceinline__ bool seed_inside(const SeedRegion &R, const float x[3], float idx) {
  if (R.sdf.phi0) {
    int c[3];
    float f[3];
    if (!sdf_locate(R.sdf, x, c, f)) return false;  // outside the lattice: not in the region
    return sdf_phi_frame(R.sdf, R.sdf.phi0, c, f) < 0.0f;
  }
  float phi, n[3];
  return levelset_eval_key(R.s, R.n_shapes, x, idx, phi, n) && phi < 0.0f;
}

// MPM::near_boundary (src/mpm.h:269-276), the expressions of particle_key
__device__ __forceinline__ bool seed_near_boundary(const SeedParams &S, const float x[3]) {
  SEED_NO_CONTRACT
  const float X0 = x[0] * S.idx, X1 = x[1] * S.idx, X2 = x[2] * S.idx;
  const float mn = fminf(X0, fminf(X1, X2));
  const float mx = fmaxf(X0 - (float)S.res[0], fmaxf(X1 - (float)S.res[1], X2 - (float)S.res[2]));
  return mn < 7.0f || mx > -7.0f;
}

// position of candidate c (sample_from_periodic_data :177-185, sample_from_source :232-243)
__device__ __forceinline__ void seed_position(const SeedParams &S, const float *__restrict__ tile, uint32_t c, float x[3]) {
  SEED_NO_CONTRACT
  const uint32_t i = c / S.n_rep, r = c - i * S.n_rep;
  const uint32_t r01 = r / (uint32_t)S.nrep[2];
  const int ind[3] = {(int)(r01 / (uint32_t)S.nrep[1]), (int)(r01 % (uint32_t)S.nrep[1]), (int)(r - r01 * (uint32_t)S.nrep[2])};
#pragma unroll
  for (int d = 0; d < 3; d++) {
    float q = tile[3 * (size_t)i + d] * S.min_distance;
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

__device__ __forceinline__ bool seed_keep(const SeedRegion &R, const SeedParams &S, const float *__restrict__ tile, uint32_t c) {
  SEED_NO_CONTRACT
  float x[3];
  seed_position(S, tile, c, x);
  if (!seed_inside(R, x, S.idx) || seed_near_boundary(S, x)) return false;
  if (!S.source) return true;
  const float y[3] = {x[0] + S.advection[0], x[1] + S.advection[1], x[2] + S.advection[2]};
  return !seed_inside(R, y, S.idx);
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

// box[0..2] = min cell index per axis of the cell centres inside the region (INT_MAX: none), box[3..5] = max (-1: none)
__global__ __launch_bounds__(SEED_WG) void k_seed_bounds(SeedRegion R, SeedParams S, int *__restrict__ box) {
  SEED_NO_CONTRACT
  const uint64_t plane = (uint64_t)S.res[1] * (uint64_t)S.res[2], total = (uint64_t)S.res[0] * plane;
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1};
  for (uint64_t n = (uint64_t)blockIdx.x * SEED_WG + threadIdx.x; n < total; n += (uint64_t)gridDim.x * SEED_WG) {
    const int i = (int)(n / plane);
    const uint32_t rem = (uint32_t)(n - (uint64_t)i * plane);
    const int j = (int)(rem / (uint32_t)S.res[2]), k = (int)(rem - (uint32_t)j * (uint32_t)S.res[2]);
    const int cell[3] = {i, j, k};
    const float x[3] = {((float)i + 0.5f) * S.dx, ((float)j + 0.5f) * S.dx, ((float)k + 0.5f) * S.dx};
    if (seed_inside(R, x, S.idx)) {
#pragma unroll
      for (int d = 0; d < 3; d++) { lo[d] = min(lo[d], cell[d]); hi[d] = max(hi[d], cell[d]); }
    }
  }
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const int a = seed_wave_min(lo[d]), b = seed_wave_max(hi[d]);
    if ((threadIdx.x & 63) == 0 && b >= 0) { atomicMin(&box[d], a); atomicMax(&box[3 + d], b); }
  }
}

__global__ __launch_bounds__(SEED_WG) void k_seed_count(SeedRegion R, SeedParams S, const float *__restrict__ tile,
                                                        unsigned long long *__restrict__ words, uint32_t *__restrict__ totals) {
  __shared__ uint32_t wave_cnt[SEED_WG / 64];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t cnt = 0;
#pragma unroll
  for (int j = 0; j < SEED_ROUNDS; j++) {
    const uint32_t c = blockIdx.x * (uint32_t)SEED_PER_WG + (uint32_t)j * SEED_WG + threadIdx.x;
    const bool keep = c < S.n_cand && seed_keep(R, S, tile, c);
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

__global__ __launch_bounds__(SEED_WG) void k_seed_write(SeedParams S, const float *__restrict__ tile,
                                                        const unsigned long long *__restrict__ words, const uint32_t *__restrict__ offs,
                                                        float4 *__restrict__ rg, float4 *__restrict__ rp, float4 *__restrict__ rb) {
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
      float x[3];
      seed_position(S, tile, c, x);
      float4 *g = rg + 4 * (size_t)rank, *p = rp + 4 * (size_t)rank, *b = rb + 3 * (size_t)rank;
      const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      g[0] = make_float4(x[0], x[1], x[2], S.aux);                       // RecG {x3, aux, F9, gid, pid, pad}
      g[1] = make_float4(S.dg, 0.0f, 0.0f, 0.0f);
      g[2] = make_float4(S.dg, 0.0f, 0.0f, 0.0f);
      g[3] = make_float4(S.dg, __uint_as_float(S.gid), __int_as_float(S.pid0 + (int32_t)rank), 0.0f);
      p[0] = make_float4(x[0], x[1], x[2], S.velocity[0]);               // RecP {x3, v3, A9, mass}
      p[1] = make_float4(S.velocity[1], S.velocity[2], 0.0f, 0.0f);
      p[2] = zero;
      p[3] = make_float4(0.0f, 0.0f, 0.0f, S.mass);
      b[0] = zero; b[1] = zero; b[2] = zero;                             // apic_b
    }
    // the words of this round behind this wave's, and those of the next round in front of it
    for (uint32_t q = word; q < word + SEED_WG / 64; q++)
      if (q < SEED_WORDS) before += (uint32_t)__popcll(w[q]);
  }
}

#undef SEED_NO_CONTRACT

// what a ctx keeps between seeding calls (host side; an emitter calls before every frame): buffers only grow
struct SeedWork {
  DevBuf<float> d_tile;  // the periodic tile, [n_tile][3]
  uint32_t n_tile = 0;
  DevBuf<unsigned long long> d_words;  // [workgroups][SEED_WORDS] ballots of the acceptance test
  DevBuf<uint32_t> d_totals;           // [workgroups] survivors per workgroup, then their exclusive prefix
  size_t wg_cap = 0;
  DevBuf<int> d_box;                   // [6] get-ready box, [6] as uint32: the survivors' count
  DevBuf<float> d_phi;                 // a sampled region's field
  size_t phi_cap = 0;
};

}  // namespace mpm
