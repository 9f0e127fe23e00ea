// taichi_mpm_amd/csrc/k_seed2d.h — kernels of mpmhip2d_seed_particles (rules: include/mpmhip.h; host side: seed2d_api.h)
// Part of libmpmhip.  The three passes of k_seed.h with dim = 2, one lane per candidate c = tile point * n_replicas + replica:
//   k2_seed_bounds  "get ready": the box of the grid's cell centres inside the region (integer min / max: order-free)
//   k2_seed_count   the acceptance test; a wave's ballot is stored as one 64-bit word per 64 candidates, a workgroup's popcount as its total
//   k_seed_scan     (k_seed.h: nothing in it is 3D) exclusive scan of the workgroup totals
//   k2_seed_write   reads the ballot words back — the test is not evaluated twice — and writes the survivors at their rank into the
//                   2D ctx's SoA arrays: x, v as float2, F, B as float4, aux, gid, pid as words; consecutive ranks write consecutive
//                   addresses of every array
// The rank of a survivor is the number of survivors with a smaller c: the order is the reference's and does not depend on scheduling.
#pragma once
#include <hip/hip_runtime.h>

#include "k_seed.h"

namespace mpm2d {

using mpm::SEED_PER_WG;
using mpm::SEED_ROUNDS;
using mpm::SEED_WG;
using mpm::SEED_WORDS;

// no multiply-add of the candidate arithmetic or of the field sampler may be fused: tests/seed2d_model.py reproduces the positions
// to the bit
#define SEED2_NO_CONTRACT _Pragma("clang fp contract(off)")

// a sampled region: phi [res0][res1] (the last axis fastest) in world units, sample (0, 0) at `origin`, one `spacing`
struct Sdf2Dev {
  const float *phi;
  int res[2];
  float origin[2];
  float spacing, inv_spacing;
};

// where the region's level set is negative: shapes read in the plane (as mpmhip2d_set_levelset stores them), or (sdf.phi != null)
// a sampled field
struct SeedRegion2 {
  int n_shapes;
  mpm::ShapeDev s[MPMHIP_MAX_SHAPES];
  Sdf2Dev sdf;
};

struct SeedParams2 {
  int res[2];
  float dx, idx;
  float min_corner[2];
  float min_distance, region_size;
  uint32_t nrep1;  // replicas along axis 1 (the replica index is ind0 * nrep1 + ind1)
  uint32_t n_rep, n_tile, n_cand;
  int source;
  float offset[2];     // source: velocity * current_t
  float advection[2];  // source: where a particle is one source_delta_t later
  // what the rows take
  float velocity[2];
  float dg, aux;
  int32_t gid, pid0;
};

// the 3D sampler's rules (mpm_math.h: sdf_locate, sdf_phi_frame) with one axis fewer: bilinear, the last axis first; a point outside
// the lattice is not in the region
__device__ __forceinline__ bool sdf2_inside(const Sdf2Dev &S, const float x[2]) {
  SEED2_NO_CONTRACT
  bool in = true;
  int c[2];
  float f[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const float u = (x[k] - S.origin[k]) * S.inv_spacing;
    in = in && u >= 0.0f && u <= (float)(S.res[k] - 1);  // (false for a NaN)
    c[k] = min(max((int)u, 0), S.res[k] - 2);
    f[k] = u - (float)c[k];
  }
  if (!in) return false;
  const float *p = S.phi + (size_t)c[0] * S.res[1] + c[1];
  const float a = mpm::sdf_lerp(p[0], p[1], f[1]);
  const float b = mpm::sdf_lerp(p[S.res[1]], p[S.res[1] + 1], f[1]);
  return mpm::sdf_lerp(a, b, f[0]) < 0.0f;
}

__device__ __forceinline__ bool seed2_inside(const SeedRegion2 &R, const float x[2], float idx) {
  if (R.sdf.phi) return sdf2_inside(R.sdf, x);
  const float xw[3] = {x[0], x[1], 0.0f};
  float phi, n[3];
  return mpm::levelset_eval_key(R.s, R.n_shapes, xw, idx, phi, n) && phi < 0.0f;
}

// MPM::near_boundary (src/mpm.h:269-276), the form of seed_near_boundary
__device__ __forceinline__ bool seed2_near_boundary(const SeedParams2 &S, const float x[2]) {
  SEED2_NO_CONTRACT
  const float X0 = x[0] * S.idx, X1 = x[1] * S.idx;
  const float mn = fminf(X0, X1);
  const float mx = fmaxf(X0 - (float)S.res[0], X1 - (float)S.res[1]);
  return mn < 7.0f || mx > -7.0f;
}

// position of candidate c (sample_from_periodic_data :177-185, sample_from_source :232-243)
__device__ __forceinline__ void seed2_position(const SeedParams2 &S, const float *__restrict__ tile, uint32_t c, float x[2]) {
  SEED2_NO_CONTRACT
  const uint32_t i = c / S.n_rep, r = c - i * S.n_rep;
  const uint32_t r0 = r / S.nrep1;
  const int ind[2] = {(int)r0, (int)(r - r0 * S.nrep1)};
  const float2 t = reinterpret_cast<const float2 *>(tile)[i];
  const float tp[2] = {t.x, t.y};
#pragma unroll
  for (int d = 0; d < 2; d++) {
    float q = tp[d] * S.min_distance;
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

__device__ __forceinline__ bool seed2_keep(const SeedRegion2 &R, const SeedParams2 &S, const float *__restrict__ tile, uint32_t c) {
  SEED2_NO_CONTRACT
  float x[2];
  seed2_position(S, tile, c, x);
  if (!seed2_inside(R, x, S.idx) || seed2_near_boundary(S, x)) return false;
  if (!S.source) return true;
  const float y[2] = {x[0] + S.advection[0], x[1] + S.advection[1]};
  return !seed2_inside(R, y, S.idx);
}

// box[0..1] = min cell index per axis of the cell centres inside the region (INT_MAX: none), box[2..3] = max (-1: none)
__global__ __launch_bounds__(SEED_WG) void k2_seed_bounds(SeedRegion2 R, SeedParams2 S, int *__restrict__ box) {
  SEED2_NO_CONTRACT
  const uint32_t total = (uint32_t)S.res[0] * (uint32_t)S.res[1];  // (res <= 16384 per axis: below 2^32)
  int lo[2] = {0x7fffffff, 0x7fffffff}, hi[2] = {-1, -1};
  for (uint32_t n = blockIdx.x * SEED_WG + threadIdx.x; n < total; n += gridDim.x * SEED_WG) {
    const int i = (int)(n / (uint32_t)S.res[1]), j = (int)(n - (uint32_t)i * (uint32_t)S.res[1]);
    const int cell[2] = {i, j};
    const float x[2] = {((float)i + 0.5f) * S.dx, ((float)j + 0.5f) * S.dx};
    if (seed2_inside(R, x, S.idx)) {
#pragma unroll
      for (int d = 0; d < 2; d++) { lo[d] = min(lo[d], cell[d]); hi[d] = max(hi[d], cell[d]); }
    }
  }
#pragma unroll
  for (int d = 0; d < 2; d++) {
    const int a = mpm::seed_wave_min(lo[d]), b = mpm::seed_wave_max(hi[d]);
    if ((threadIdx.x & 63) == 0 && b >= 0) { atomicMin(&box[d], a); atomicMax(&box[2 + d], b); }
  }
}

__global__ __launch_bounds__(SEED_WG) void k2_seed_count(SeedRegion2 R, SeedParams2 S, const float *__restrict__ tile,
                                                         unsigned long long *__restrict__ words, uint32_t *__restrict__ totals) {
  __shared__ uint32_t wave_cnt[SEED_WG / 64];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t cnt = 0;
#pragma unroll
  for (int j = 0; j < SEED_ROUNDS; j++) {
    const uint32_t c = blockIdx.x * (uint32_t)SEED_PER_WG + (uint32_t)j * SEED_WG + threadIdx.x;
    const bool keep = c < S.n_cand && seed2_keep(R, S, tile, c);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) words[(size_t)blockIdx.x * SEED_WORDS + j * (SEED_WG / 64) + wave] = m;
    cnt += (uint32_t)__popcll(m);
  }
  if (lane == 0) wave_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) totals[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// x, v, F, B, aux, gid, pid point at the first free slot of the ctx's arrays
__global__ __launch_bounds__(SEED_WG) void k2_seed_write(SeedParams2 S, const float *__restrict__ tile,
                                                         const unsigned long long *__restrict__ words, const uint32_t *__restrict__ offs,
                                                         float2 *__restrict__ x, float2 *__restrict__ v, float4 *__restrict__ F,
                                                         float4 *__restrict__ B, float *__restrict__ aux, int32_t *__restrict__ gid,
                                                         int32_t *__restrict__ pid) {
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
      float p[2];
      seed2_position(S, tile, c, p);
      x[rank] = make_float2(p[0], p[1]);
      v[rank] = make_float2(S.velocity[0], S.velocity[1]);
      F[rank] = make_float4(S.dg, 0.0f, 0.0f, S.dg);
      B[rank] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      aux[rank] = S.aux;
      gid[rank] = S.gid;
      pid[rank] = S.pid0 + (int32_t)rank;
    }
    // the words of this round behind this wave's, and those of the next round in front of it
    for (uint32_t q = word; q < word + SEED_WG / 64; q++)
      if (q < SEED_WORDS) before += (uint32_t)__popcll(w[q]);
  }
}

#undef SEED2_NO_CONTRACT

// what a 2D ctx keeps between seeding calls (host side; an emitter calls before every frame): buffers only grow
struct SeedWork2 {
  DevBuf<float> d_tile;  // the periodic tile, [n_tile][2]
  uint32_t n_tile = 0;
  DevBuf<unsigned long long> d_words;  // [workgroups][SEED_WORDS] ballots of the acceptance test
  DevBuf<uint32_t> d_totals;           // [workgroups] survivors per workgroup, then their exclusive prefix
  size_t wg_cap = 0;
  DevBuf<int> d_box;                   // [4] get-ready box, [4] as uint32: the survivors' count
  DevBuf<float> d_phi;                 // a sampled region's field
  size_t phi_cap = 0;
};

}  // namespace mpm2d
