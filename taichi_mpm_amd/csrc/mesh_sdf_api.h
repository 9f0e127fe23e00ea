// taichi_mpm_amd/csrc/mesh_sdf_api.h — host side of the mesh voxeliser (kernels: k_mesh_sdf.h; rules: include/mpmhip.h)
// Included by mpmhip.hip.  A voxelisation runs in two halves so that a refused mesh writes no output: msdf_stage (upload, records,
// lists, column parity) and, once msdf_verdict has read the flags, msdf_distance into the destination array.
#pragma once

extern "C++" {  // (mpmhip.hip includes this inside its extern "C" block)
namespace {

constexpr uint32_t MSDF_MAX_TRI = 1u << 26;
constexpr unsigned long long MSDF_MAX_LIST3 = 1ull << 27;  // entries (512 MB); above it the tiles read every record instead

int msdf_reserve(mpmhip_ctx *c, DevBuf<uint32_t> &p, size_t &cap, size_t count) {
  if (count <= cap && p) return MPMHIP_OK;
  cap = 0;
  if (p.alloc(count) != hipSuccess) return fail(c, MPMHIP_ENOMEM, "mesh voxeliser: device allocation of %zu bytes failed", count * sizeof(uint32_t));
  cap = count;
  return MPMHIP_OK;
}

// argument checks shared by the two entry points; fills L
int msdf_check_args(mpmhip_ctx *c, const char *who, const mpmhip_sdf_desc *d, int32_t n_tri, const float *tri, float band, MeshLattice &L) {
  if (!d || !tri) return fail(c, MPMHIP_EINVAL, "%s: the lattice description and the triangles are required", who);
  std::string why;
  if (!sdf_lattice::check<3>(d->res, d->origin, d->spacing, why)) return fail(c, MPMHIP_EINVAL, "%s: %s", who, why.c_str());
  for (int k = 0; k < 3; k++) { L.res[k] = d->res[k]; L.origin[k] = d->origin[k]; L.tiles[k] = (d->res[k] + 7) / 8; }
  L.spacing = d->spacing;
  L.words = d->res[2] / 32 + 1;
  if (L.words > 256) return fail(c, MPMHIP_EINVAL, "%s: res[2] = %d, the column pass holds at most 8191 samples per column", who, d->res[2]);
  if (n_tri <= 0 || (uint32_t)n_tri > MSDF_MAX_TRI) return fail(c, MPMHIP_EINVAL, "%s: n_tri = %d, between 1 and 2^26 triangles are needed", who, n_tri);
  if (!(band > 0.0f)) return fail(c, MPMHIP_EINVAL, "%s: band must be > 0 (+inf is allowed)", who);
  for (size_t m = 0; m < (size_t)n_tri * 9; m++)
    if (!std::isfinite(tri[m])) return fail(c, MPMHIP_EINVAL, "%s: triangle %zu has a non-finite vertex", who, m / 9);
  return MPMHIP_OK;
}

// upload + k_msdf_prep + lists + k_msdf_parity, all on `stream`; synchronises once (the list sizes)
int msdf_stage(mpmhip_ctx *c, MeshSdfWork &W, hipStream_t stream, const MeshLattice &L, uint32_t n_tri, const float *tri, float band) {
  const size_t tiles2 = (size_t)L.tiles[0] * L.tiles[1], tiles3 = tiles2 * L.tiles[2];
  const size_t cols = (size_t)L.res[0] * L.res[1];
  int rc;
  if (n_tri > W.tri_cap || !W.d_tri) {
    W.tri_cap = 0;
    if (W.d_tri.alloc((size_t)n_tri * 9) != hipSuccess || W.d_rec.alloc((size_t)n_tri * 4) != hipSuccess)
      return fail(c, MPMHIP_ENOMEM, "mesh voxeliser: device allocation for %u triangles failed", n_tri);
    W.tri_cap = n_tri;
  }
  if (tiles2 > W.tiles2_cap) {
    size_t cap = W.tiles2_cap;
    if ((rc = msdf_reserve(c, W.d_cnt2, cap, tiles2))) return rc;
    if ((rc = msdf_reserve(c, W.d_off2, W.tiles2_cap, tiles2 + 1))) return rc;
    W.tiles2_cap = tiles2;
  }
  W.lists3 = std::isfinite(band);
  if (W.lists3 && tiles3 > W.tiles3_cap) {
    size_t cap = W.tiles3_cap;
    if ((rc = msdf_reserve(c, W.d_cnt3, cap, tiles3))) return rc;
    if ((rc = msdf_reserve(c, W.d_off3, W.tiles3_cap, tiles3 + 1))) return rc;
    W.tiles3_cap = tiles3;
  }
  if ((rc = msdf_reserve(c, W.d_sign, W.sign_cap, cols * (size_t)L.words))) return rc;
  if (!W.d_flags) HIPCHK(c, W.d_flags.alloc((size_t)MSDF_F_WORDS));
  W.n_tri = n_tri;
  HIPCHK(c, hipMemcpyAsync(W.d_tri, tri, sizeof(float) * 9 * n_tri, hipMemcpyHostToDevice, stream));
  HIPCHK(c, hipMemsetAsync(W.d_flags, 0, sizeof(uint32_t) * MSDF_F_WORDS, stream));
  HIPCHK(c, hipMemsetAsync(W.d_cnt2, 0, sizeof(uint32_t) * tiles2, stream));
  if (W.lists3) HIPCHK(c, hipMemsetAsync(W.d_cnt3, 0, sizeof(uint32_t) * tiles3, stream));
  const dim3 tgrid((n_tri + 255u) / 256u);
  hipLaunchKernelGGL(k_msdf_prep, tgrid, dim3(256), 0, stream, n_tri, W.d_tri, W.d_rec, W.d_flags);
  hipLaunchKernelGGL(k_msdf_bin<false>, tgrid, dim3(256), 0, stream, L, band, n_tri, (const float *)W.d_tri, (const float4 *)W.d_rec, W.d_cnt2,
                     (const uint32_t *)nullptr, (uint32_t *)nullptr, W.lists3 ? W.d_cnt3 : nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr);
  hipLaunchKernelGGL(k_msdf_scan, dim3(W.lists3 ? 2 : 1), dim3(1024), 0, stream, W.d_cnt2, W.d_off2, (uint32_t)tiles2, W.d_cnt3, W.d_off3,
                     (uint32_t)(W.lists3 ? tiles3 : 0), W.d_flags);
  if ((rc = launch_check(c, "mesh_sdf lists"))) return rc;
  uint32_t fl[MSDF_F_WORDS];
  HIPCHK(c, hipMemcpyAsync(fl, W.d_flags, sizeof fl, hipMemcpyDeviceToHost, stream));
  HIPCHK(c, hipStreamSynchronize(stream));
  if (fl[MSDF_F_VALID] == 0) return fail(c, MPMHIP_EINVAL, "mesh voxeliser: every one of the %u triangles has zero area", n_tri);
  if (fl[MSDF_F_TOTAL2] >= 0x80000000u) return fail(c, MPMHIP_EINVAL, "mesh voxeliser: the column lists would hold more than 2^31 entries");
  const unsigned long long total3 = ((unsigned long long)fl[MSDF_F_TOTAL3_HI] << 32) | fl[MSDF_F_TOTAL3_LO];
  if (W.lists3 && total3 > MSDF_MAX_LIST3) W.lists3 = false;  // a superset of every list is as good: all records
  if ((rc = msdf_reserve(c, W.d_list2, W.list2_cap, (size_t)fl[MSDF_F_TOTAL2] + 1))) return rc;
  if (W.lists3 && (rc = msdf_reserve(c, W.d_list3, W.list3_cap, (size_t)total3 + 1))) return rc;
  hipLaunchKernelGGL(k_msdf_bin<true>, tgrid, dim3(256), 0, stream, L, band, n_tri, (const float *)W.d_tri, (const float4 *)W.d_rec, W.d_cnt2,
                     (const uint32_t *)W.d_off2, W.d_list2, W.lists3 ? W.d_cnt3 : nullptr, (const uint32_t *)W.d_off3, W.d_list3);
  hipLaunchKernelGGL(k_msdf_parity, dim3((uint32_t)tiles2), dim3(64), sizeof(uint32_t) * 64 * (size_t)L.words, stream, L, (const float *)W.d_tri,
                     (const uint32_t *)W.d_off2, (const uint32_t *)W.d_list2, W.d_sign, W.d_flags);
  return launch_check(c, "mesh_sdf parity");
}

// the watertightness verdict of a staged voxelisation (synchronises)
int msdf_verdict(mpmhip_ctx *c, MeshSdfWork &W, hipStream_t stream, const char *who, const char *which) {
  uint32_t fl[MSDF_F_WORDS];
  HIPCHK(c, hipMemcpyAsync(fl, W.d_flags, sizeof fl, hipMemcpyDeviceToHost, stream));
  HIPCHK(c, hipStreamSynchronize(stream));
  if (fl[MSDF_F_ODD])
    return fail(c, MPMHIP_EINVAL, "%s: the mesh%s is not closed: %u lattice columns cross it an odd number of times", who, which, fl[MSDF_F_ODD]);
  return MPMHIP_OK;
}

int msdf_distance(mpmhip_ctx *c, MeshSdfWork &W, hipStream_t stream, const MeshLattice &L, float band, float *d_phi) {
  const uint32_t tiles3 = (uint32_t)L.tiles[0] * L.tiles[1] * L.tiles[2];
  hipLaunchKernelGGL(k_msdf_distance, dim3(tiles3), dim3(256), 0, stream, L, band, W.n_tri, (const float4 *)W.d_rec, (const uint32_t *)W.d_off3,
                     (const uint32_t *)(W.lists3 ? W.d_list3 : nullptr), (const uint32_t *)W.d_sign, d_phi);
  return launch_check(c, "mesh_sdf distance");
}

}  // namespace
}  // extern "C++"

// triangles -> a host array, no ctx (include/mpmhip.h)
int mpmhip_mesh_to_sdf(int32_t device, const mpmhip_sdf_desc *d, int32_t n_tri, const float *tri, float band, float *phi_out) {
  MeshLattice L;
  if (!phi_out) return fail(nullptr, MPMHIP_EINVAL, "mesh_to_sdf: the output array is required");
  if (int rc = msdf_check_args(nullptr, "mesh_to_sdf", d, n_tri, tri, band, L)) return rc;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
    return fail(nullptr, MPMHIP_EINVAL, "mesh_to_sdf: device %d is not one of the %d visible GPUs", device, n_dev);
  HIPCHK(nullptr, hipSetDevice(device));
  const size_t count = (size_t)L.res[0] * L.res[1] * L.res[2];
  MeshSdfWork W;
  DevBuf<float> d_phi;
  if (int rc = msdf_stage(nullptr, W, nullptr, L, (uint32_t)n_tri, tri, band)) return rc;
  if (int rc = msdf_verdict(nullptr, W, nullptr, "mesh_to_sdf", "")) return rc;
  if (d_phi.alloc(count) != hipSuccess) return fail(nullptr, MPMHIP_ENOMEM, "mesh_to_sdf: device allocation of %zu bytes failed", count * 4);
  if (int rc = msdf_distance(nullptr, W, nullptr, L, band, d_phi)) return rc;
  HIPCHK(nullptr, hipMemcpy(phi_out, d_phi, sizeof(float) * count, hipMemcpyDeviceToHost));
  return MPMHIP_OK;
}

// triangles -> the ctx's own sampled level set: mpmhip_set_levelset_sdf without the host arrays (include/mpmhip.h)
int mpmhip_set_levelset_mesh(mpmhip_ctx *c, const mpmhip_sdf_desc *d, int32_t n_tri0, const float *tri0, int32_t n_tri1, const float *tri1,
                             float t0, float t1, float band, float friction) {
  if (!c) return MPMHIP_EINVAL;
  if (c->in_substep) return fail(c, MPMHIP_EINVAL, "set_levelset_mesh inside a substep");
  MeshLattice L;
  if (int rc = msdf_check_args(c, "set_levelset_mesh", d, n_tri0, tri0, band, L)) return rc;
  if (tri1) {
    if (int rc = msdf_check_args(c, "set_levelset_mesh (second key frame)", d, n_tri1, tri1, band, L)) return rc;
    if (!(t1 > t0)) return fail(c, MPMHIP_EINVAL, "key frame times must satisfy t0 < t1");
  }
  if (c->rigid.ls_collision) return fail(c, MPMHIP_EINVAL, "rigid_body_levelset_collision is not supported with a sampled level set");
  HIPCHK(c, hipSetDevice(c->device));
  // both meshes are judged before anything of the installed set is touched: a refused call leaves it in force
  int rc = msdf_stage(c, c->mesh_work[0], c->stream, L, (uint32_t)n_tri0, tri0, band);
  if (!rc && tri1) rc = msdf_stage(c, c->mesh_work[1], c->stream, L, (uint32_t)n_tri1, tri1, band);
  if (!rc) rc = msdf_verdict(c, c->mesh_work[0], c->stream, "set_levelset_mesh", tri1 ? " of the first key frame" : "");
  if (!rc && tri1) rc = msdf_verdict(c, c->mesh_work[1], c->stream, "set_levelset_mesh", " of the second key frame");
  if (rc) return rc;  // (msdf_verdict synchronised the stream: no kernel in flight reads the arrays below)
  if ((rc = sdf_reserve(c, d, tri1 != nullptr))) return rc;
  if ((rc = msdf_distance(c, c->mesh_work[0], c->stream, L, band, c->sdf.frame[0]))) return rc;
  if (tri1 && (rc = msdf_distance(c, c->mesh_work[1], c->stream, L, band, c->sdf.frame[1]))) return rc;
  return sdf_install(c, d, tri1 != nullptr, t0, t1, friction);
}

// the installed sampled set's key frame, back to the host
int mpmhip_download_levelset_sdf(mpmhip_ctx *c, int32_t frame, float *dst, int64_t capacity) {
  if (!c) return MPMHIP_EINVAL;
  if (!dst) return fail(c, MPMHIP_EINVAL, "download_levelset_sdf: the destination is required");
  if (!c->LS.sdf.phi0) return fail(c, MPMHIP_EINVAL, "download_levelset_sdf: no sampled level set is installed");
  if (frame < 0 || frame > 1 || (frame == 1 && !c->LS.sdf.phi1)) return fail(c, MPMHIP_EINVAL, "download_levelset_sdf: there is no key frame %d", frame);
  if (capacity < (int64_t)c->sdf.count)
    return fail(c, MPMHIP_EINVAL, "download_levelset_sdf: room for %lld samples, the set has %zu", (long long)capacity, c->sdf.count);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(dst, c->sdf.frame[frame], sizeof(float) * c->sdf.count, hipMemcpyDeviceToHost));
  return MPMHIP_OK;
}
