// taichi_mpm_amd/csrc/k_async.h — AsyncMPM<dim> on the device, for both dimensions: the particle pools of the asynchronous stepper
// and the kernels that move particles between them and the working set of an advance (AsyncMPM<dim>::advance,
// src/async/async_mpm.cpp:255-373; gather_from_pool, src/async/async_mpm.h:198-234; create_simulation2('async_mpm'):
// TC_IMPLEMENTATION(Simulation2D, AsyncMPM2D, "async_mpm"), :423-427).  Part of libmpmhip; host side: async_api.h.
//
// The reference keeps, per scheduler block (SPGrid block of 4 x 4 x 8 nodes, 8 x 16 in 2D), a `particle_pool` (containers at the
// block's own time) and a `backup_pool` (copies at an earlier time).  Here both live in ONE device-resident STORE of containers
// with a tag word each; a pool is the set of containers carrying its tag:
//     tag = block | AS_BACKUP bit,  AS_FREE for a dropped container.
// An advance never moves a container inside the store: it re-tags (pool -> backup, clear) in place, copies the winners of
// the gather into the ctx's particle arrays (the working set of ONE ordinary substep), and appends the results behind the
// store's end.  Freed containers are squeezed out by an order-preserving compaction when they outnumber the live ones.
// No particle data crosses the PCIe bus during stepping: the host sees block tables and four counters.
//
// The kernels are written once, over two small views passed by value: where a container's words lie (Store3, Store2) and how
// the working set is laid out (Work3: the 3D ctx's records, Work2: the 2D object's arrays).
#pragma once
#include "mpm_common.h"
#include "k_sort.h"
#include "async_sched.h"  // the action bits AT_* of the per-block table, ASYNC_BLOCK_SHIFT

namespace mpm {

constexpr uint32_t AS_BACKUP = 0x80000000u, AS_FREE = INVALID;
struct AsyncCounters {
  uint32_t n_work, n_append, n_freed, n_live;  // transient: reset by the host behind every read-back
  uint32_t size, pad[3];                       // persistent: containers in use incl. freed ones (the append cursor); pad[0]: sticky
                                               // error word (bit 8: a chained scan of the compaction waited in vain, k_sort.h)
};

// A 3D container: two 64-byte records + an id word.  g = the ctx's RecG image (x3, aux, F9, gid, id, -), w = {v3, -},
// {apic_b[0..3]}, {apic_b[4..7]}, {apic_b[8], -, -, -}.
struct Store3 {
  static constexpr int D = 3;
  uint32_t *tag;
  int32_t *idw;
  float4 *g, *w;
  __device__ __forceinline__ int32_t id(uint32_t e) const { return idw[e]; }
  __device__ __forceinline__ void copy_to(uint32_t e, const Store3 &to, uint32_t o) const {  // (every load before the first store)
    const int32_t i = idw[e];
    const float4 *sg = g + (size_t)e * 4, *sw = w + (size_t)e * 4;
    const float4 g0 = sg[0], g1 = sg[1], g2 = sg[2], g3 = sg[3], w0 = sw[0], w1 = sw[1], w2 = sw[2], w3 = sw[3];
    float4 *dg = to.g + (size_t)o * 4, *dw = to.w + (size_t)o * 4;
    to.idw[o] = i;
    dg[0] = g0; dg[1] = g1; dg[2] = g2; dg[3] = g3; dw[0] = w0; dw[1] = w1; dw[2] = w2; dw[3] = w3;
  }
  __device__ __forceinline__ void state(uint32_t e, mat3 &F, float v[3], float &aux, uint32_t &gid) const {
    const float4 g0 = g[(size_t)e * 4], g1 = g[(size_t)e * 4 + 1], g2 = g[(size_t)e * 4 + 2], g3 = g[(size_t)e * 4 + 3];
    const float4 w0 = w[(size_t)e * 4];
    F.m[0] = g1.x; F.m[1] = g1.y; F.m[2] = g1.z; F.m[3] = g1.w; F.m[4] = g2.x; F.m[5] = g2.y; F.m[6] = g2.z; F.m[7] = g2.w; F.m[8] = g3.x;
    v[0] = w0.x; v[1] = w0.y; v[2] = w0.z;
    aux = g0.w; gid = __float_as_uint(g3.y);
  }
  static constexpr int ROW = 27;  // floats of an export row {x3, v3, F9, apic_b9, aux, gid bits, id bits} (k_async_export's)
  __device__ __forceinline__ void row(uint32_t e, float *__restrict__ r) const {
    const float *sg = reinterpret_cast<const float *>(g + (size_t)e * 4), *sw = reinterpret_cast<const float *>(w + (size_t)e * 4);
    r[0] = sg[0]; r[1] = sg[1]; r[2] = sg[2];
    r[3] = sw[0]; r[4] = sw[1]; r[5] = sw[2];
#pragma unroll
    for (int k = 0; k < 9; k++) { r[6 + k] = sg[4 + k]; r[15 + k] = sw[4 + k]; }
    r[24] = sg[3]; r[25] = sg[13]; r[26] = sg[14];
  }
};
// A 2D container: ONE 64-byte record {x2, v2}, {F4}, {apic_b4}, {aux, gid bits, id bits, -}.
struct Store2 {
  static constexpr int D = 2;
  uint32_t *tag;
  float4 *rec;
  __device__ __forceinline__ int32_t id(uint32_t e) const { return __float_as_int(rec[(size_t)e * 4 + 3].z); }
  __device__ __forceinline__ void copy_to(uint32_t e, const Store2 &to, uint32_t o) const {
    const float4 *s = rec + (size_t)e * 4;
    const float4 r0 = s[0], r1 = s[1], r2 = s[2], r3 = s[3];
    float4 *d = to.rec + (size_t)o * 4;
    d[0] = r0; d[1] = r1; d[2] = r2; d[3] = r3;
  }
  // get_allowed_dt has no dim-dependent term (src/particles.cpp:136-155 ...): the 2 x 2 F is embedded in a 3 x 3 one
  __device__ __forceinline__ void state(uint32_t e, mat3 &F, float v[3], float &aux, uint32_t &gid) const {
    const float4 r0 = rec[(size_t)e * 4], r1 = rec[(size_t)e * 4 + 1], r3 = rec[(size_t)e * 4 + 3];
    F.m[0] = r1.x; F.m[1] = r1.y; F.m[2] = 0.0f; F.m[3] = r1.z; F.m[4] = r1.w; F.m[5] = 0.0f; F.m[6] = 0.0f; F.m[7] = 0.0f; F.m[8] = 1.0f;
    v[0] = r0.z; v[1] = r0.w; v[2] = 0.0f;
    aux = r3.x; gid = __float_as_uint(r3.y);
  }
  static constexpr int ROW = 16;  // an export row is the record itself: {x2, v2, F4, apic_b4, aux, gid bits, id bits, -}
  __device__ __forceinline__ void row(uint32_t e, float *__restrict__ r) const {
    const float4 *s = rec + (size_t)e * 4;
    const float4 r0 = s[0], r1 = s[1], r2 = s[2], r3 = s[3];
    float4 *d = reinterpret_cast<float4 *>(r);  // (rows of 64 bytes in a hipMalloc'ed array: aligned)
    d[0] = r0; d[1] = r1; d[2] = r2; d[3] = r3;
  }
};

// The working set of a 3D ctx: its records (the P2G matrix A of RecP is rebuilt by k_affine: it depends on the advance's dt).
struct Work3 {
  using Store = Store3;
  float4 *rg, *rp, *rb;
  const GroupParams *groups;
  __device__ __forceinline__ void from_store(uint32_t s, const Store3 &S, uint32_t e) const {
    const float4 g0 = S.g[(size_t)e * 4], g1 = S.g[(size_t)e * 4 + 1], g2 = S.g[(size_t)e * 4 + 2], g3 = S.g[(size_t)e * 4 + 3];
    const float4 w0 = S.w[(size_t)e * 4], w1 = S.w[(size_t)e * 4 + 1], w2 = S.w[(size_t)e * 4 + 2], w3 = S.w[(size_t)e * 4 + 3];
    const float mass = groups[__float_as_uint(g3.y)].p[0];
    rg[(size_t)s * 4] = g0; rg[(size_t)s * 4 + 1] = g1; rg[(size_t)s * 4 + 2] = g2; rg[(size_t)s * 4 + 3] = g3;
    rp[(size_t)s * 4] = make_float4(g0.x, g0.y, g0.z, w0.x);
    rp[(size_t)s * 4 + 1] = make_float4(w0.y, w0.z, 0.0f, 0.0f);
    rp[(size_t)s * 4 + 2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    rp[(size_t)s * 4 + 3] = make_float4(0.0f, 0.0f, 0.0f, mass);
    rb[(size_t)s * 3] = w1; rb[(size_t)s * 3 + 1] = w2; rb[(size_t)s * 3 + 2] = w3;
  }
  __device__ __forceinline__ int32_t id(uint32_t i) const { return __float_as_int(rg[(size_t)i * 4 + 3].z); }
  __device__ __forceinline__ void pos(uint32_t i, float x[3]) const {
    const float4 g0 = rg[(size_t)i * 4];
    x[0] = g0.x; x[1] = g0.y; x[2] = g0.z;
  }
  __device__ __forceinline__ void to_store(uint32_t i, const Store3 &S, uint32_t e) const {
    const float4 g0 = rg[(size_t)i * 4], g1 = rg[(size_t)i * 4 + 1], g2 = rg[(size_t)i * 4 + 2], g3 = rg[(size_t)i * 4 + 3];
    const float4 p0 = rp[(size_t)i * 4], p1 = rp[(size_t)i * 4 + 1];
    const float4 b0 = rb[(size_t)i * 3], b1 = rb[(size_t)i * 3 + 1], b2 = rb[(size_t)i * 3 + 2];
    S.g[(size_t)e * 4] = g0; S.g[(size_t)e * 4 + 1] = g1; S.g[(size_t)e * 4 + 2] = g2; S.g[(size_t)e * 4 + 3] = g3;
    S.w[(size_t)e * 4] = make_float4(p0.w, p1.x, p1.y, 0.0f);
    S.w[(size_t)e * 4 + 1] = b0; S.w[(size_t)e * 4 + 2] = b1; S.w[(size_t)e * 4 + 3] = b2;
    S.idw[e] = __float_as_int(g3.z);
  }
};
// The working set of the 2D object: its particle arrays (k_mpm2d.h).
struct Work2 {
  using Store = Store2;
  float *x, *v, *F, *B, *aux;
  int32_t *gid, *pid;
  __device__ __forceinline__ void from_store(uint32_t s, const Store2 &S, uint32_t e) const {
    const float4 r0 = S.rec[(size_t)e * 4], r1 = S.rec[(size_t)e * 4 + 1], r2 = S.rec[(size_t)e * 4 + 2], r3 = S.rec[(size_t)e * 4 + 3];
    x[2 * s] = r0.x; x[2 * s + 1] = r0.y; v[2 * s] = r0.z; v[2 * s + 1] = r0.w;
    F[4 * s] = r1.x; F[4 * s + 1] = r1.y; F[4 * s + 2] = r1.z; F[4 * s + 3] = r1.w;
    B[4 * s] = r2.x; B[4 * s + 1] = r2.y; B[4 * s + 2] = r2.z; B[4 * s + 3] = r2.w;
    aux[s] = r3.x; gid[s] = __float_as_int(r3.y); pid[s] = __float_as_int(r3.z);
  }
  __device__ __forceinline__ int32_t id(uint32_t i) const { return pid[i]; }
  __device__ __forceinline__ void pos(uint32_t i, float p[3]) const { p[0] = x[2 * i]; p[1] = x[2 * i + 1]; p[2] = 0.0f; }
  __device__ __forceinline__ void to_store(uint32_t i, const Store2 &S, uint32_t e) const {
    const float4 r0 = make_float4(x[2 * i], x[2 * i + 1], v[2 * i], v[2 * i + 1]);
    const float4 r1 = make_float4(F[4 * i], F[4 * i + 1], F[4 * i + 2], F[4 * i + 3]);
    const float4 r2 = make_float4(B[4 * i], B[4 * i + 1], B[4 * i + 2], B[4 * i + 3]);
    const float4 r3 = make_float4(aux[i], __int_as_float(gid[i]), __int_as_float(pid[i]), 0.0f);
    S.rec[(size_t)e * 4] = r0; S.rec[(size_t)e * 4 + 1] = r1; S.rec[(size_t)e * 4 + 2] = r2; S.rec[(size_t)e * 4 + 3] = r3;
  }
};

// gather_from_pool's "the first copy of an id wins" (particles_cnt[id] != global_cnt): copies are ordered by gather phase
// (smaller-step pools, this step's pools, larger-step backups), then by the reference's block order, then by position in the
// store (= insertion order).  Smallest key wins.
__device__ __forceinline__ unsigned long long async_key(uint32_t cat, uint32_t rank, uint32_t e) {
  return ((unsigned long long)cat << 60) | ((unsigned long long)rank << 32) | e;
}
__device__ __forceinline__ int async_category(uint32_t tag, uint8_t act) {
  if (tag == AS_FREE) return -1;
  if (!(tag & AS_BACKUP)) return (act & AT_POOL0) ? 0 : ((act & AT_POOL1) ? 1 : -1);
  return (act & AT_BACKUP) ? 2 : -1;
}

template <class Store>
__global__ __launch_bounds__(256) void k_async_mark(uint32_t size, Store S, const uint8_t *__restrict__ tbl,
                                                    const uint32_t *__restrict__ rank_of, unsigned long long *__restrict__ best) {
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < size; e += gridDim.x * blockDim.x) {
    const uint32_t t = S.tag[e];
    if (t == AS_FREE) continue;
    const uint32_t b = t & ~AS_BACKUP;
    const int cat = async_category(t, tbl[b]);
    if (cat >= 0) atomicMin(&best[S.id(e)], async_key((uint32_t)cat, rank_of[b], e));
  }
}

// winners -> the working set (slot = order of arrival), then the in-place re-tagging of backup_current_dt_limit
template <class Work>
__global__ __launch_bounds__(256) void k_async_gather(uint32_t size, typename Work::Store S, const uint8_t *__restrict__ tbl,
                                                      const uint32_t *__restrict__ rank_of, unsigned long long *__restrict__ best,
                                                      Work W, AsyncCounters *cnt) {
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < size; e += gridDim.x * blockDim.x) {
    const uint32_t t = S.tag[e];
    if (t == AS_FREE) continue;
    const uint32_t b = t & ~AS_BACKUP;
    const uint8_t act = tbl[b];
    const int cat = async_category(t, act);
    if (cat >= 0) {
      const int32_t id = S.id(e);
      if (best[id] == async_key((uint32_t)cat, rank_of[b], e)) {
        best[id] = ~0ull;  // (one winner per id: the table is clean again after the pass)
        W.from_store(atomicAdd(&cnt->n_work, 1u), S, e);
      }
    }
    if (act & AT_SWAP) {
      if (t & AS_BACKUP) { S.tag[e] = AS_FREE; atomicAdd(&cnt->n_freed, 1u); }
      else S.tag[e] = t | AS_BACKUP;
    }
  }
}

// after the substep: backups that have served (":337-341 backup_pool[offset].clear()")
__global__ __launch_bounds__(256) void k_async_clear(uint32_t size, uint32_t *__restrict__ tag, const uint8_t *__restrict__ tbl,
                                                     AsyncCounters *cnt) {
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < size; e += gridDim.x * blockDim.x) {
    const uint32_t t = tag[e];
    if (t != AS_FREE && (t & AS_BACKUP) && (tbl[t & ~AS_BACKUP] & AT_CLEAR)) { tag[e] = AS_FREE; atomicAdd(&cnt->n_freed, 1u); }
  }
}

// scheduler block of a position: the reference's SPGrid block holding the particle's base node (get_grid_base_pos,
// src/mpm.h:252-255; src/async/async_mpm.cpp:350-355); INVALID outside the block table (nb[2] = 1 in 2D)
template <int D>
__device__ __forceinline__ uint32_t async_block_of(float idx, const float x[3], int nbx, int nby, int nbz) {
  constexpr int s0 = ASYNC_BLOCK_SHIFT[D][0], s1 = ASYNC_BLOCK_SHIFT[D][1], s2 = ASYNC_BLOCK_SHIFT[D][2];
  const float X0 = x[0] * idx, X1 = x[1] * idx, X2 = D == 3 ? x[2] * idx : 0.5f;
  if (!(X0 >= 0.5f && X1 >= 0.5f && X2 >= 0.5f)) return INVALID;
  const int bx = (int)(X0 - 0.5f) >> s0, by = (int)(X1 - 0.5f) >> s1, bz = (int)(X2 - 0.5f) >> s2;
  if (bx >= nbx || by >= nby || bz >= nbz) return INVALID;
  return ((uint32_t)bx * nby + by) * nbz + bz;
}

// the working set after its substep -> containers behind the store's end (":345-375 update backup_pool and particle_pool").
// all_to_pool: AsyncMPM::add_particles (src/async/async_mpm.cpp:57-75) — every particle goes to its block's pool.
template <class Work>
__global__ __launch_bounds__(256) void k_async_file(float idx, uint32_t n, Work W, const uint8_t *__restrict__ tbl, int all_to_pool,
                                                    int nbx, int nby, int nbz, uint32_t cap, typename Work::Store S, AsyncCounters *cnt) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (W.id(i) < 0) continue;  // deleted by the substep (clear_boundary_particles): not filed back, as in the reference
    float x[3];
    W.pos(i, x);
    const uint32_t b = async_block_of<Work::Store::D>(idx, x, nbx, nby, nbz);
    if (b == INVALID) continue;
    const uint8_t act = all_to_pool ? (uint8_t)AT_DEST_POOL : tbl[b];
    if (!(act & (AT_DEST_POOL | AT_DEST_BACKUP))) continue;
    const uint32_t e = atomicAdd(&cnt->size, 1u);  // (the append cursor lives on the device: the host knows an upper bound)
    if (e >= cap) { atomicSub(&cnt->size, 1u); continue; }  // (the host sized the store for the whole working set: cannot happen)
    atomicAdd(&cnt->n_append, 1u);
    W.to_store(i, S, e);
    S.tag[e] = (act & AT_DEST_POOL) ? b : (b | AS_BACKUP);
  }
}

// order-preserving compaction of the store (chained single-pass scan of k_sort.h: chunk = 1024 containers)
template <class Store>
__global__ __launch_bounds__(256) void k_async_compact(uint32_t size, Store S, Store S2, unsigned long long *__restrict__ slots,
                                                       uint32_t epoch, AsyncCounters *cnt) {
  __shared__ uint32_t lds[8];
  const uint32_t nchunks = (size + 1023u) / 1024u;
  uint32_t round = 0;
  while (true) {
    const uint32_t chunk = next_chunk(round);
    if (chunk >= nchunks) return;
    const uint32_t e0 = chunk * 1024u + threadIdx.x * 4u;
    uint32_t t[4], live = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      t[j] = (e0 + j < size) ? S.tag[e0 + j] : AS_FREE;
      live += t[j] != AS_FREE;
    }
    uint32_t total;
    const uint32_t excl = wg_exclusive_scan_256(live, lds, total);
    if (threadIdx.x == 0) publish(slots + chunk, epoch, total);
    uint32_t o = sum_predecessors(slots, chunk, epoch, lds, &cnt->pad[0]) + excl;  // (a wait that expires: sticky bit in pad[0], read back by the host)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (t[j] == AS_FREE) continue;
      S2.tag[o] = t[j];
      S.copy_to(e0 + j, S2, o);
      o++;
    }
    if (chunk == nchunks - 1 && threadIdx.x == 255) { cnt->n_live = o; cnt->size = o; }
  }
}

// (min allowed dt = 0.1, max |v|^2 = 1e-16, count = 0) per block: the start values of the reduction (":104-105")
__global__ __launch_bounds__(256) void k_async_table_reset(uint32_t nblk, uint32_t *__restrict__ tab) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < nblk; b += gridDim.x * blockDim.x) {
    tab[3 * (size_t)b] = __float_as_uint(0.1f); tab[3 * (size_t)b + 1] = __float_as_uint(1e-16f); tab[3 * (size_t)b + 2] = 0u;
  }
}

// update_dt_limits, device half (src/async/async_mpm.cpp:91-111) over the POOL containers of the store: per block the
// smallest get_allowed_dt(dx), the largest |v|^2 and the number of containers (same table as k_async_block_reduce)
template <class Store>
__global__ __launch_bounds__(256) void k_async_store_reduce(float dx, uint32_t size, Store S, const GroupParams *__restrict__ groups,
                                                            uint32_t *__restrict__ tab) {
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < size; e += gridDim.x * blockDim.x) {
    const uint32_t t = S.tag[e];
    if (t == AS_FREE || (t & AS_BACKUP)) continue;
    mat3 F;
    float v[3], aux;
    uint32_t gid;
    S.state(e, F, v, aux, gid);
    const float adt = allowed_dt(groups[gid], F, aux, v, dx);
    float v2 = v[0] * v[0];
#pragma unroll
    for (int k = 1; k < Store::D; k++) v2 += v[k] * v[k];
    atomicMin(&tab[3 * (size_t)t + 0], __float_as_uint(fmaxf(adt, 0.0f)));
    atomicMax(&tab[3 * (size_t)t + 1], __float_as_uint(v2));
    atomicAdd(&tab[3 * (size_t)t + 2], 1u);
  }
}

// every pool container -> the working set (AsyncMPM::visualize's particle list: duplicates of an id included, each with the
// block of the pool it sits in, src/async/async_visualize.cpp:17-26,86-96)
template <class Work>
__global__ __launch_bounds__(256) void k_async_load(uint32_t size, typename Work::Store S, Work W, uint32_t *__restrict__ blk_of,
                                                    AsyncCounters *cnt) {
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < size; e += gridDim.x * blockDim.x) {
    const uint32_t t = S.tag[e];
    if (t == AS_FREE || (t & AS_BACKUP)) continue;
    const uint32_t s = atomicAdd(&cnt->n_work, 1u);
    W.from_store(s, S, e);
    blk_of[s] = t;
  }
}

// pool containers -> flat arrays (tests, frame output): one row per container, in order of arrival (in store order:
// k_async_export_ordered below)
__global__ __launch_bounds__(256) void k_async_export(uint32_t size, const uint32_t *__restrict__ tag, const float4 *__restrict__ sg,
                                                      const float4 *__restrict__ sw, float *__restrict__ out27, uint32_t *__restrict__ blk,
                                                      AsyncCounters *cnt) {
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < size; e += gridDim.x * blockDim.x) {
    const uint32_t t = tag[e];
    if (t == AS_FREE || (t & AS_BACKUP)) continue;
    const uint32_t o = atomicAdd(&cnt->n_work, 1u);
    const float *g = reinterpret_cast<const float *>(sg + (size_t)e * 4), *w = reinterpret_cast<const float *>(sw + (size_t)e * 4);
    float *r = out27 + (size_t)o * 27;
    r[0] = g[0]; r[1] = g[1]; r[2] = g[2];                      // x
    r[3] = w[0]; r[4] = w[1]; r[5] = w[2];                      // v
#pragma unroll
    for (int k = 0; k < 9; k++) { r[6 + k] = g[4 + k]; r[15 + k] = w[4 + k]; }  // F, apic_b
    r[24] = g[3]; r[25] = g[13]; r[26] = g[14];                 // aux, gid (bits), id (bits)
    blk[o] = t;
  }
}

// the 2D store's export (mpmhip2d_async_download_pools): one row of Store2::ROW floats per pool container, in order of arrival
__global__ __launch_bounds__(256) void k_async_export2(uint32_t size, Store2 S, float *__restrict__ out, uint32_t *__restrict__ blk,
                                                       AsyncCounters *cnt) {
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < size; e += gridDim.x * blockDim.x) {
    const uint32_t t = S.tag[e];
    if (t == AS_FREE || (t & AS_BACKUP)) continue;
    const uint32_t o = atomicAdd(&cnt->n_work, 1u);
    S.row(e, out + (size_t)o * Store2::ROW);
    blk[o] = t;
  }
}

// ---- deterministic mode (mpmhip_config.deterministic / mpmhip2d_config.deterministic): the ORDERED forms of the four kernels above
// that take a destination from a global counter.  There the order of the working set, of the store and of everything read from the
// store is the order in which lanes arrived.  Here each kernel is a stream compaction like k_async_compact: chunks of 1024 elements
// per workgroup, four consecutive ones per lane, flag = "this element is written", slot = exclusive prefix of the flags in element
// order (chained single-pass scan of k_sort.h over the store's scan words, a fresh epoch per launch; the host launches no more
// workgroups than stay resident; a wait that expires sets the sticky bit of cnt->pad[0] and counts the missing sums as zero: every
// slot is then too small, i.e. inside its array).  What comes out is a function of the input arrays alone, whatever the launch size.
//
// where a chunk's written elements go: `slot` of this lane's first one, [begin, end) of the whole chunk.  `fold` is added to what the
// chunk publishes: k_async_file_ordered's chunk 0 hands the append cursor on that way (every other caller and chunk: 0).
struct OrderedSlots { uint32_t slot, begin, end; };
__device__ __forceinline__ OrderedSlots async_ordered_slots(uint32_t mine, uint32_t chunk, uint32_t fold, unsigned long long *__restrict__ slots,
                                                            uint32_t epoch, uint32_t *lds, uint32_t *err) {
  uint32_t total;
  const uint32_t excl = wg_exclusive_scan_256(mine, lds, total);
  if (threadIdx.x == 0) publish(slots + chunk, epoch, total + fold);
  const uint32_t pre = sum_predecessors(slots, chunk, epoch, lds, err) + fold;
  return OrderedSlots{pre + excl, pre, pre + total};
}

// k_async_gather with the winners in ascending store position
template <class Work>
__global__ __launch_bounds__(256) void k_async_gather_ordered(uint32_t size, typename Work::Store S, const uint8_t *__restrict__ tbl,
                                                              const uint32_t *__restrict__ rank_of, unsigned long long *__restrict__ best,
                                                              Work W, unsigned long long *__restrict__ slots, uint32_t epoch,
                                                              AsyncCounters *cnt) {
  __shared__ uint32_t lds[8];
  const uint32_t nchunks = (size + 1023u) / 1024u;
  uint32_t round = 0;
  while (true) {
    const uint32_t chunk = next_chunk(round);
    if (chunk >= nchunks) return;
    const uint32_t e0 = chunk * 1024u + threadIdx.x * 4u;
    uint32_t win = 0, nwin = 0, freed = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t e = e0 + j;
      const uint32_t t = e < size ? S.tag[e] : AS_FREE;
      if (t == AS_FREE) continue;
      const uint32_t b = t & ~AS_BACKUP;
      const uint8_t act = tbl[b];
      const int cat = async_category(t, act);
      if (cat >= 0) {
        const int32_t id = S.id(e);
        if (best[id] == async_key((uint32_t)cat, rank_of[b], e)) {
          best[id] = ~0ull;  // (one winner per id: the table is clean again after the pass)
          win |= 1u << j;
          nwin++;
        }
      }
      if (act & AT_SWAP) {
        if (t & AS_BACKUP) { S.tag[e] = AS_FREE; freed++; }
        else S.tag[e] = t | AS_BACKUP;
      }
    }
    if (freed) atomicAdd(&cnt->n_freed, freed);  // (an integer sum: the same whatever the order)
    const OrderedSlots R = async_ordered_slots(nwin, chunk, 0u, slots, epoch, lds, &cnt->pad[0]);
    uint32_t o = R.slot;
#pragma unroll
    for (int j = 0; j < 4; j++)
      if ((win >> j) & 1u) W.from_store(o++, S, e0 + j);
    if (chunk == nchunks - 1 && threadIdx.x == 255) cnt->n_work = R.end;
  }
}

// k_async_file with the filed particles behind the store's end in ascending working-set slot.  The base of the append is the
// device's cnt->size (the host knows an upper bound while an earlier advance's appends are pending): chunk 0 — nobody else —
// reads it and folds it into what it publishes, every later chunk gets it with the sum of its predecessors, and the last chunk —
// nobody else — writes the new cursor, which it can only know after chunk 0 has read the old one.
template <class Work>
__global__ __launch_bounds__(256) void k_async_file_ordered(float idx, uint32_t n, Work W, const uint8_t *__restrict__ tbl, int all_to_pool,
                                                            int nbx, int nby, int nbz, uint32_t cap, typename Work::Store S,
                                                            unsigned long long *__restrict__ slots, uint32_t epoch, AsyncCounters *cnt) {
  __shared__ uint32_t lds[8];
  const uint32_t nchunks = (n + 1023u) / 1024u;
  uint32_t round = 0;
  while (true) {
    const uint32_t chunk = next_chunk(round);
    if (chunk >= nchunks) return;
    const uint32_t i0 = chunk * 1024u + threadIdx.x * 4u;
    uint32_t tag[4], nfiled = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t i = i0 + j;
      tag[j] = AS_FREE;
      if (i >= n || W.id(i) < 0) continue;  // deleted by the substep (clear_boundary_particles): not filed back, as in the reference
      float x[3];
      W.pos(i, x);
      const uint32_t b = async_block_of<Work::Store::D>(idx, x, nbx, nby, nbz);
      if (b == INVALID) continue;
      const uint8_t act = all_to_pool ? (uint8_t)AT_DEST_POOL : tbl[b];
      if (!(act & (AT_DEST_POOL | AT_DEST_BACKUP))) continue;
      tag[j] = (act & AT_DEST_POOL) ? b : (b | AS_BACKUP);
      nfiled++;
    }
    const uint32_t base = chunk == 0u ? cnt->size : 0u;
    const OrderedSlots R = async_ordered_slots(nfiled, chunk, base, slots, epoch, lds, &cnt->pad[0]);
    uint32_t e = R.slot;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (tag[j] == AS_FREE) continue;
      if (e < cap) {  // (the host sized the store for the whole working set: cannot happen)
        W.to_store(i0 + j, S, e);
        S.tag[e] = tag[j];
      }
      e++;
    }
    if (threadIdx.x == 255) {
      atomicAdd(&cnt->n_append, min(R.end, cap) - min(R.begin, cap));  // (an integer sum: the same whatever the order)
      if (chunk == nchunks - 1) cnt->size = min(R.end, cap);
    }
  }
}

// k_async_load with the view in store order
template <class Work>
__global__ __launch_bounds__(256) void k_async_load_ordered(uint32_t size, typename Work::Store S, Work W, uint32_t *__restrict__ blk_of,
                                                            unsigned long long *__restrict__ slots, uint32_t epoch, AsyncCounters *cnt) {
  __shared__ uint32_t lds[8];
  const uint32_t nchunks = (size + 1023u) / 1024u;
  uint32_t round = 0;
  while (true) {
    const uint32_t chunk = next_chunk(round);
    if (chunk >= nchunks) return;
    const uint32_t e0 = chunk * 1024u + threadIdx.x * 4u;
    uint32_t t[4], npool = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      t[j] = (e0 + j < size) ? S.tag[e0 + j] : AS_FREE;
      if (t[j] & AS_BACKUP) t[j] = AS_FREE;  // (AS_FREE has the bit too: what stays is a pool container)
      npool += t[j] != AS_FREE;
    }
    const OrderedSlots R = async_ordered_slots(npool, chunk, 0u, slots, epoch, lds, &cnt->pad[0]);
    uint32_t s = R.slot;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (t[j] == AS_FREE) continue;
      W.from_store(s, S, e0 + j);
      blk_of[s] = t[j];
      s++;
    }
    if (chunk == nchunks - 1 && threadIdx.x == 255) cnt->n_work = R.end;
  }
}

// k_async_export / k_async_export2 with the rows in store order
template <class Store>
__global__ __launch_bounds__(256) void k_async_export_ordered(uint32_t size, Store S, float *__restrict__ out, uint32_t *__restrict__ blk,
                                                              unsigned long long *__restrict__ slots, uint32_t epoch, AsyncCounters *cnt) {
  __shared__ uint32_t lds[8];
  const uint32_t nchunks = (size + 1023u) / 1024u;
  uint32_t round = 0;
  while (true) {
    const uint32_t chunk = next_chunk(round);
    if (chunk >= nchunks) return;
    const uint32_t e0 = chunk * 1024u + threadIdx.x * 4u;
    uint32_t t[4], npool = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      t[j] = (e0 + j < size) ? S.tag[e0 + j] : AS_FREE;
      if (t[j] & AS_BACKUP) t[j] = AS_FREE;
      npool += t[j] != AS_FREE;
    }
    const OrderedSlots R = async_ordered_slots(npool, chunk, 0u, slots, epoch, lds, &cnt->pad[0]);
    uint32_t o = R.slot;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (t[j] == AS_FREE) continue;
      S.row(e0 + j, out + (size_t)o * Store::ROW);
      blk[o] = t[j];
      o++;
    }
    if (chunk == nchunks - 1 && threadIdx.x == 255) cnt->n_work = R.end;
  }
}

}  // namespace mpm
