// taichi_mpm_amd/csrc/k_mesh_sdf.h — triangles -> signed-distance lattice (mpmhip_mesh_to_sdf, mpmhip_set_levelset_mesh)
// Part of libmpmhip (see mpmhip.hip for the substep overview; the rules of the voxeliser are stated in include/mpmhip.h and the
// float64 model of them is tests/mesh_sdf_model.py).  Host side: mesh_sdf_api.h.
//
//   k_msdf_prep      a lane per triangle: vertices into lexicographic order (in place: orientation and vertex order drop out of
//                    every later number), the 64-byte record the distance kernel reads
//   k_msdf_bin       a lane per triangle, run twice (count, fill): the triangle goes on the list of every 8^3 tile of samples its
//                    bounding box grown by `band` overlaps, and of every 8x8 tile of columns its xy box overlaps.  Integer atomics
//                    only; the order inside a list is arbitrary and nothing downstream depends on it (min and xor)
//   k_msdf_scan      counts -> offsets, one workgroup per list family
//   k_msdf_parity    a wave per 8x8 tile of columns, a lane per column (i, j, .): exact fp64 crossing test against the tile's
//                    triangles, one toggle bit per crossing at its height in the lane's own LDS words, then the suffix parity as a
//                    bit per sample; a column with an odd total is counted in a device flag
//   k_msdf_distance  a workgroup per 8^3 tile: the tile's records staged through LDS 64 at a time with whole-record loads, two
//                    samples per lane, running minimum of the squared distance; writes phi = s min(d, band) once per sample
#pragma once
#include "mpm_common.h"

namespace mpm {

struct MeshLattice {
  int res[3];
  float origin[3];
  float spacing;
  int tiles[3];  // ceil(res / 8)
  int words;     // res[2] / 32 + 1: 32-bit words of a column's bit row (one bit more than samples: a crossing above the last one)
};
enum { MSDF_F_VALID = 0, MSDF_F_ODD = 1, MSDF_F_TOTAL2 = 2, MSDF_F_TOTAL3_LO = 3, MSDF_F_TOTAL3_HI = 4, MSDF_F_WORDS = 8 };
constexpr int MSDF_CHUNK = 64;  // records per LDS chunk of k_msdf_distance (4 KB)

// where sample index i sits on an axis: fl(origin + fl(i * spacing)), never fused — the one definition every kernel and the model use
__device__ __forceinline__ float msdf_coord(float o, float sp, int i) { return __fadd_rn(o, __fmul_rn((float)i, sp)); }

__device__ __forceinline__ bool msdf_lex_less(const float *a, const float *b) {
  if (a[0] != b[0]) return a[0] < b[0];
  if (a[1] != b[1]) return a[1] < b[1];
  return a[2] < b[2];
}
__device__ __forceinline__ void msdf_swap3(float *a, float *b) {
  for (int k = 0; k < 3; k++) { const float t = a[k]; a[k] = b[k]; b[k] = t; }
}

// record: (a, valid) (ab, ab.ab) (ac, ac.ac) (ab.ac, 0, 0, 0); valid = 0 for a triangle of zero area (cross product exactly zero)
__global__ __launch_bounds__(256) void k_msdf_prep(uint32_t n, float *__restrict__ tri, float4 *__restrict__ rec,
                                                   uint32_t *__restrict__ flags) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  float v[3][3];
  for (int m = 0; m < 9; m++) v[m / 3][m % 3] = tri[(size_t)t * 9 + m];
  if (msdf_lex_less(v[1], v[0])) msdf_swap3(v[0], v[1]);
  if (msdf_lex_less(v[2], v[1])) msdf_swap3(v[1], v[2]);
  if (msdf_lex_less(v[1], v[0])) msdf_swap3(v[0], v[1]);
  for (int m = 0; m < 9; m++) tri[(size_t)t * 9 + m] = v[m / 3][m % 3];
  float ab[3], ac[3];
  for (int k = 0; k < 3; k++) { ab[k] = v[1][k] - v[0][k]; ac[k] = v[2][k] - v[0][k]; }
  const float nx = __fsub_rn(__fmul_rn(ab[1], ac[2]), __fmul_rn(ab[2], ac[1]));
  const float ny = __fsub_rn(__fmul_rn(ab[2], ac[0]), __fmul_rn(ab[0], ac[2]));
  const float nz = __fsub_rn(__fmul_rn(ab[0], ac[1]), __fmul_rn(ab[1], ac[0]));
  const bool valid = nx != 0.0f || ny != 0.0f || nz != 0.0f;
  rec[(size_t)t * 4] = make_float4(v[0][0], v[0][1], v[0][2], valid ? 1.0f : 0.0f);
  rec[(size_t)t * 4 + 1] = make_float4(ab[0], ab[1], ab[2], ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2]);
  rec[(size_t)t * 4 + 2] = make_float4(ac[0], ac[1], ac[2], ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2]);
  rec[(size_t)t * 4 + 3] = make_float4(ab[0] * ac[0] + ab[1] * ac[1] + ab[2] * ac[2], 0.0f, 0.0f, 0.0f);
  if (valid) atomicAdd(&flags[MSDF_F_VALID], 1u);
}

// conservative range of sample indices on one axis whose coordinate can lie in [lo, hi]: one index of slack on either side covers
// the rounding of the division.  false: the interval misses the lattice.
__device__ __forceinline__ bool msdf_index_range(float lo, float hi, float o, float sp, int res, int &i0, int &i1) {
  const float last = (float)(res - 1);
  float a = floorf((lo - o) / sp) - 1.0f, b = ceilf((hi - o) / sp) + 1.0f;
  if (!(b >= 0.0f) || !(a <= last)) return false;  // (a NaN cannot come from finite input; it would land here)
  a = fmaxf(a, 0.0f); b = fminf(b, last);
  i0 = (int)a; i1 = (int)b;
  return true;
}

// FILL = false: count the triangle into cnt[tile]; true: write it at off[tile] + (cursor in cnt[tile], zeroed by the scan)
template <bool FILL>
__global__ __launch_bounds__(256) void k_msdf_bin(MeshLattice L, float band, uint32_t n, const float *__restrict__ tri,
                                                  const float4 *__restrict__ rec, uint32_t *__restrict__ cnt2,
                                                  const uint32_t *__restrict__ off2, uint32_t *__restrict__ list2,
                                                  uint32_t *__restrict__ cnt3 /* nullptr: no 3D lists (every tile reads all) */,
                                                  const uint32_t *__restrict__ off3, uint32_t *__restrict__ list3) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  if (rec[(size_t)t * 4].w == 0.0f) return;  // zero area: no distance, and its projection has zero area too
  float lo[3], hi[3];
  for (int k = 0; k < 3; k++) {
    const float a = tri[(size_t)t * 9 + k], b = tri[(size_t)t * 9 + 3 + k], c = tri[(size_t)t * 9 + 6 + k];
    lo[k] = fminf(a, fminf(b, c)); hi[k] = fmaxf(a, fmaxf(b, c));
  }
  int i0[3], i1[3];
  if (msdf_index_range(lo[0], hi[0], L.origin[0], L.spacing, L.res[0], i0[0], i1[0]) &&
      msdf_index_range(lo[1], hi[1], L.origin[1], L.spacing, L.res[1], i0[1], i1[1])) {
    for (int a = i0[0] >> 3; a <= i1[0] >> 3; a++)
      for (int b = i0[1] >> 3; b <= i1[1] >> 3; b++) {
        const uint32_t tile = (uint32_t)(a * L.tiles[1] + b);
        const uint32_t at = atomicAdd(&cnt2[tile], 1u);
        if (FILL) list2[off2[tile] + at] = t;
      }
  }
  if (!cnt3) return;
  bool hit = true;
  for (int k = 0; k < 3; k++) hit = hit && msdf_index_range(lo[k] - band, hi[k] + band, L.origin[k], L.spacing, L.res[k], i0[k], i1[k]);
  if (!hit) return;
  for (int a = i0[0] >> 3; a <= i1[0] >> 3; a++)
    for (int b = i0[1] >> 3; b <= i1[1] >> 3; b++)
      for (int c = i0[2] >> 3; c <= i1[2] >> 3; c++) {
        const uint32_t tile = (uint32_t)((a * L.tiles[1] + b) * L.tiles[2] + c);
        const uint32_t at = atomicAdd(&cnt3[tile], 1u);
        if (FILL) list3[off3[tile] + at] = t;
      }
}

// exclusive scan of cnt[0, n) into off[0, n], cnt zeroed behind it (the fill pass uses it as its cursors); the 64-bit total to
// flags.  Workgroup 0 scans the column-tile family, workgroup 1 (launched only when there are 3D lists) the 3D one.
__global__ __launch_bounds__(1024) void k_msdf_scan(uint32_t *__restrict__ cnt2, uint32_t *__restrict__ off2, uint32_t n2,
                                                    uint32_t *__restrict__ cnt3, uint32_t *__restrict__ off3, uint32_t n3,
                                                    uint32_t *__restrict__ flags) {
  __shared__ unsigned long long part[1024];
  uint32_t *cnt = blockIdx.x ? cnt3 : cnt2, *off = blockIdx.x ? off3 : off2;
  const uint32_t n = blockIdx.x ? n3 : n2;
  const uint32_t per = (n + 1023u) / 1024u, b = min(n, threadIdx.x * per), e = min(n, b + per);
  unsigned long long s = 0;
  for (uint32_t i = b; i < e; i++) s += cnt[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (uint32_t d = 1; d < 1024u; d <<= 1) {
    const unsigned long long add = threadIdx.x >= d ? part[threadIdx.x - d] : 0ull;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  unsigned long long run = part[threadIdx.x] - s;
  for (uint32_t i = b; i < e; i++) {
    const uint32_t v = cnt[i];
    off[i] = (uint32_t)run;
    cnt[i] = 0u;
    run += v;
  }
  if (threadIdx.x == 1023u) {
    const unsigned long long total = part[1023];
    off[n] = (uint32_t)total;
    if (blockIdx.x) { flags[MSDF_F_TOTAL3_LO] = (uint32_t)total; flags[MSDF_F_TOTAL3_HI] = (uint32_t)(total >> 32); }
    else flags[MSDF_F_TOTAL2] = total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)total;
  }
}

// does the ray from (px, py) towards +x cross the projected edge a-b?  Half-open in y (an end point exactly at py counts as below),
// the side by the sign of the edge function taken from the lower end point: differences of fp32 numbers and their products are
// exact in fp64, so the sign of the difference of the two products is exact; a zero (the point ON the edge) is not a crossing.
// The answer depends on the edge and the point only, not on the triangle asking: the two triangles of an edge always agree, which
// is what makes the column test watertight.
__device__ __forceinline__ bool msdf_edge_cross(double ax, double ay, double bx, double by, double px, double py) {
  if ((ay > py) == (by > py)) return false;
  if (ay > by) { double t = ax; ax = bx; bx = t; t = ay; ay = by; by = t; }
  return (bx - ax) * (py - ay) - (by - ay) * (px - ax) > 0.0;
}

extern __shared__ __attribute__((aligned(16))) uint32_t msdf_bits[];  // [word][lane]: a lane only ever touches its own column

__global__ __launch_bounds__(64) void k_msdf_parity(MeshLattice L, const float *__restrict__ tri, const uint32_t *__restrict__ off,
                                                    const uint32_t *__restrict__ list, uint32_t *__restrict__ sign,
                                                    uint32_t *__restrict__ flags) {
  const int lane = threadIdx.x;
  const int i = (int)(blockIdx.x / (uint32_t)L.tiles[1]) * 8 + (lane >> 3), j = (int)(blockIdx.x % (uint32_t)L.tiles[1]) * 8 + (lane & 7);
  const bool live = i < L.res[0] && j < L.res[1];
  for (int w = 0; w < L.words; w++) msdf_bits[w * 64 + lane] = 0u;
  const double px = (double)msdf_coord(L.origin[0], L.spacing, i), py = (double)msdf_coord(L.origin[1], L.spacing, j);
  const int nz = L.res[2];
  uint32_t crossings = 0;
  const uint32_t b = off[blockIdx.x], e = off[blockIdx.x + 1];
  for (uint32_t m = b; m < e; m++) {
    const float *v = tri + (size_t)list[m] * 9;  // (wave-uniform address)
    const double x0 = v[0], y0 = v[1], z0 = v[2], x1 = v[3], y1 = v[4], z1 = v[5], x2 = v[6], y2 = v[7], z2 = v[8];
    const bool in = msdf_edge_cross(x0, y0, x1, y1, px, py) ^ msdf_edge_cross(x1, y1, x2, y2, px, py) ^
                    msdf_edge_cross(x0, y0, x2, y2, px, py);
    const double area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0);
    if (!live || !in || area == 0.0) continue;
    // height of the triangle over the column: barycentric weights from the edge functions
    const double e1 = (x0 - x2) * (py - y2) - (y0 - y2) * (px - x2), e2 = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0);
    const double zc = z0 + (e1 * (z1 - z0) + e2 * (z2 - z0)) / area;
    // kc = how many samples of the column lie strictly below the crossing (their own height is compared with >)
    const double g = (zc - (double)L.origin[2]) / (double)L.spacing;
    int kc = !(g >= 0.0) ? 0 : (g >= (double)nz ? nz : (int)g);
    while (kc < nz && (double)msdf_coord(L.origin[2], L.spacing, kc) < zc) kc++;
    while (kc > 0 && !((double)msdf_coord(L.origin[2], L.spacing, kc - 1) < zc)) kc--;
    msdf_bits[(kc >> 5) * 64 + lane] ^= 1u << (kc & 31);
    crossings++;
  }
  if (!live) return;
  if (crossings & 1u) atomicAdd(&flags[MSDF_F_ODD], 1u);
  // sample k is inside iff an odd number of crossings lie above it: the xor of the toggle bits at positions > k
  uint32_t carry = 0u;
  for (int w = L.words - 1; w >= 0; w--) {
    const uint32_t tg = msdf_bits[w * 64 + lane];
    uint32_t y = tg;
    y ^= y >> 1; y ^= y >> 2; y ^= y >> 4; y ^= y >> 8; y ^= y >> 16;  // y bit k = xor of tg bits >= k
    sign[((size_t)i * L.res[1] + j) * L.words + w] = (y ^ tg) ^ carry;
    if (__popc(tg) & 1) carry = ~carry;
  }
}

// squared distance from p to the triangle of a record: closest point by the regions of the triangle's Voronoi diagram (vertex a, b,
// edge ab, vertex c, edge ac, edge bc, face, tested in that order) from d1 = ab.ap and d2 = ac.ap and the record's three dot
// products; the closest point is a + v ab + w ac with (v, w) = (nv, nw) / den.
__device__ __forceinline__ float msdf_dist2(const float4 &q0, const float4 &q1, const float4 &q2, const float4 &q3, float px, float py,
                                            float pz) {
  const float ax = px - q0.x, ay = py - q0.y, az = pz - q0.z;
  const float d1 = q1.x * ax + q1.y * ay + q1.z * az, d2 = q2.x * ax + q2.y * ay + q2.z * az;
  const float d3 = d1 - q1.w, d4 = d2 - q3.x, d5 = d1 - q3.x, d6 = d2 - q2.w;
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float t1 = d4 - d3, t2 = d5 - d6;
  float nv = vb, nw = vc, den = va + vb + vc;
  if (va <= 0.0f && t1 >= 0.0f && t2 >= 0.0f) { nv = t2; nw = t1; den = t1 + t2; }
  if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { nv = 0.0f; nw = d2; den = d2 - d6; }
  if (d6 >= 0.0f && d5 <= d6) { nv = 0.0f; nw = 1.0f; den = 1.0f; }
  if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { nv = d1; nw = 0.0f; den = d1 - d3; }
  if (d3 >= 0.0f && d4 <= d3) { nv = 1.0f; nw = 0.0f; den = 1.0f; }
  if (d1 <= 0.0f && d2 <= 0.0f) { nv = 0.0f; nw = 0.0f; den = 1.0f; }
  const float v = nv / den, w = nw / den;
  const float rx = ax - v * q1.x - w * q2.x, ry = ay - v * q1.y - w * q2.y, rz = az - v * q1.z - w * q2.z;
  return rx * rx + ry * ry + rz * rz;
}

// list == nullptr: every tile reads all n_tri records (band = +inf, or lists that would not fit)
__global__ __launch_bounds__(256) void k_msdf_distance(MeshLattice L, float band, uint32_t n_tri, const float4 *__restrict__ rec,
                                                       const uint32_t *__restrict__ off, const uint32_t *__restrict__ list,
                                                       const uint32_t *__restrict__ sign, float *__restrict__ phi) {
  __shared__ float4 s_rec[MSDF_CHUNK * 4];
  const uint32_t tile = blockIdx.x;
  const int tk = (int)(tile % (uint32_t)L.tiles[2]), tj = (int)((tile / (uint32_t)L.tiles[2]) % (uint32_t)L.tiles[1]),
            ti = (int)(tile / ((uint32_t)L.tiles[2] * (uint32_t)L.tiles[1]));
  const int t = threadIdx.x;
  const int i0 = ti * 8 + (t >> 6), i1 = i0 + 4, j = tj * 8 + ((t >> 3) & 7), k = tk * 8 + (t & 7);
  const float px0 = msdf_coord(L.origin[0], L.spacing, i0), px1 = msdf_coord(L.origin[0], L.spacing, i1);
  const float py = msdf_coord(L.origin[1], L.spacing, j), pz = msdf_coord(L.origin[2], L.spacing, k);
  const uint32_t b = list ? off[tile] : 0u, e = list ? off[tile + 1] : n_tri;
  float best0 = __builtin_inff(), best1 = __builtin_inff();
  for (uint32_t base = b; base < e; base += MSDF_CHUNK) {
    const uint32_t m = min((uint32_t)MSDF_CHUNK, e - base);
    __syncthreads();
    if ((uint32_t)t < 4u * m) {  // a record is 4 consecutive float4: lanes 4r .. 4r+3 fetch record r whole
      const uint32_t r = base + ((uint32_t)t >> 2);
      s_rec[t] = rec[(size_t)(list ? list[r] : r) * 4 + (t & 3)];
    }
    __syncthreads();
    for (uint32_t r = 0; r < m; r++) {
      const float4 q0 = s_rec[4 * r];  // (the same address in every lane: an LDS broadcast)
      if (q0.w == 0.0f) continue;      // zero area (reached only without lists; wave-uniform)
      const float4 q1 = s_rec[4 * r + 1], q2 = s_rec[4 * r + 2], q3 = s_rec[4 * r + 3];
      best0 = fminf(best0, msdf_dist2(q0, q1, q2, q3, px0, py, pz));
      best1 = fminf(best1, msdf_dist2(q0, q1, q2, q3, px1, py, pz));
    }
  }
  if (j >= L.res[1] || k >= L.res[2]) return;
  const uint32_t bit = 1u << (k & 31);
  if (i0 < L.res[0]) {
    const size_t col = (size_t)i0 * L.res[1] + j;
    const float d = fminf(sqrtf(best0), band);
    phi[col * L.res[2] + k] = (sign[col * L.words + (k >> 5)] & bit) ? -d : d;
  }
  if (i1 < L.res[0]) {
    const size_t col = (size_t)i1 * L.res[1] + j;
    const float d = fminf(sqrtf(best1), band);
    phi[col * L.res[2] + k] = (sign[col * L.words + (k >> 5)] & bit) ? -d : d;
  }
}

// ------------------------------------------------------------------------------------------------ host side: the work buffers
// One voxelisation's device buffers; a ctx keeps one per key frame and every call reuses what is large enough.
struct MeshSdfWork {
  DevBuf<float> d_tri;    // [n_tri][3][3], vertices in lexicographic order behind k_msdf_prep
  DevBuf<float4> d_rec;   // [n_tri][4]
  size_t tri_cap = 0;
  DevBuf<uint32_t> d_cnt2, d_off2, d_cnt3, d_off3;
  size_t tiles2_cap = 0, tiles3_cap = 0;
  DevBuf<uint32_t> d_list2, d_list3;
  size_t list2_cap = 0, list3_cap = 0;
  DevBuf<uint32_t> d_sign;  // [res0][res1][words]
  size_t sign_cap = 0;
  DevBuf<uint32_t> d_flags;  // MSDF_F_*
  uint32_t n_tri = 0;
  bool lists3 = false;  // this voxelisation has 3D lists (else every tile reads every record)
};

}  // namespace mpm
