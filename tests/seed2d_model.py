"""numpy model of mpmhip2d_seed_particles (include/mpmhip.h; csrc/k_seed.h, csrc/seed_api.h at D = 2) — the yardstick of the 2D seeding
tests.  tests/seed_model.py with dim = 2: it restates, in fp32 and in the device's order of operations (every operation rounded),
PoissonDiskSampler<2>::sample_from_periodic_data and sample_from_source (src/poisson_disk_sampler.h:157-252) behind get_ready (:34-69):

  get ready   cell centres ((i + 0.5) * dx); box of the centres inside the region; min_corner = min - dx, max_corner = max + dx;
              min_distance = float32(sqrt(dx^2 / ppc * 2 / 3)) (double); region_size = 40 * min_distance;
              replicas per axis = max(1, ceil((max_corner - min_corner) / region_size))
  candidates  c = i * n_replicas + r (r: the replica index in C order);  q = tile_i * min_distance
              [source: q += velocity * current_t;  q -= floor(q / region_size + 0.5) * region_size]
              position = (q + min_corner) + region_size * (ind + 0.5)
  acceptance  inside the region, not within 7 cells of a wall (X = x * (1 / dx): min X < 7 or max (X - res) > -7)
              [source: and position + advection NOT inside; advection = v * d + ((0.5 * g) * (d + base_dt)) * d]
  order       survivors in ascending c, creation ids first_id + rank

A sampled region is read by the boundary's own sampler (csrc/mpm_math.h: sdf_locate, sdf_phi_frame at D = 2; the device forbids
contraction there, so the model is exact); shapes are evaluated with the formulas of levelset_eval_key in the plane, where the device's compiler may contract a
multiply and an add: a shape test sets candidates with |phi| below a margin aside."""
import ctypes as C

import numpy as np

F = np.float32


def load_tile():
    """the library's tile (mpmhip2d_poisson_tile: host code, no GPU)"""
    import taichi_mpm_amd as tm
    L = tm.load()
    n = int(L.mpmhip2d_poisson_tile(None, 0))
    out = np.empty((n, 2), F)
    assert L.mpmhip2d_poisson_tile(out.ctypes.data_as(C.POINTER(C.c_float)), n) == n
    return out


class SampledRegion2D:
    """where the bilinear interpolant of phi (res0, res1; world units) is negative; outside the lattice: not in the region"""

    def __init__(self, phi, origin, spacing, dx):
        self.p = np.ascontiguousarray(phi, F)
        self.res = np.array(self.p.shape, np.int64)
        self.origin = np.asarray(origin, F)
        self.inv_spacing = F(1.0) / F(spacing)
        self.idx = F(1.0) / F(dx)

    @staticmethod
    def _lerp(a, b, f):
        return (((F(1.0) - f).astype(F) * a).astype(F) + (f * b).astype(F)).astype(F)

    def phi(self, x):
        """(phi in grid units, +inf outside the lattice; inside flags)"""
        x = np.asarray(x, F).reshape(-1, 2)
        u = ((x - self.origin[None, :]).astype(F) * self.inv_spacing).astype(F)
        hit = np.all((u >= 0) & (u <= (self.res - 1).astype(F)[None, :]), axis=1)
        with np.errstate(invalid="ignore"):
            c = np.clip(np.trunc(np.where(np.isfinite(u), u, 0)).astype(np.int64), 0, (self.res - 2)[None, :])
        f = (u - c.astype(F)).astype(F)
        p, i, j = self.p, c[:, 0], c[:, 1]
        a = self._lerp(p[i, j], p[i, j + 1], f[:, 1])  # the last axis first
        b = self._lerp(p[i + 1, j], p[i + 1, j + 1], f[:, 1])
        v = self._lerp(a, b, f[:, 0])
        return np.where(hit, (v * self.idx).astype(F), F(np.inf)), hit & (v < 0)

    def inside(self, x):
        return self.phi(x)[1]


class ShapeRegion2D:
    """where min over the shapes of phi is negative: mpmhip_shape rows (type, inside_out, p[6]) read in the plane as
    mpmhip2d_set_levelset reads them (plane: n.x + d with n's z dropped; sphere: a disc; cuboid: unbounded along z), the formulas of
    levelset_eval_key (csrc/mpm_math.h) at z = 0, fp32"""

    def __init__(self, shapes, dx):
        self.shapes = [(int(t), int(io), np.asarray(p, F)) for t, io, p in shapes]
        self.idx = F(1.0) / F(dx)

    def phi(self, x):
        x = np.asarray(x, F).reshape(-1, 2)
        phi = np.full(len(x), F(1e30), F)
        for t, io, q in self.shapes:
            if t == 0:
                ph = ((x[:, 0] * q[0]).astype(F) + (x[:, 1] * q[1]).astype(F)).astype(F) + q[3]
            elif t == 1:
                d = (x - q[None, :2]).astype(F)
                ph = np.sqrt(((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F)).astype(F) - q[3]
            else:
                lo, hi = q[None, 0:2], q[None, 3:5]
                ins = np.all((lo <= x) & (x <= hi), axis=1)
                depth = np.minimum((x - lo).astype(F), (hi - x).astype(F)).min(axis=1)
                d = (x - np.minimum(np.maximum(x, lo), hi)).astype(F)
                out = np.sqrt(((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F)).astype(F)
                ph = np.where(ins, -depth, out)
            if t != 0 and io:
                ph = -ph
            ph = (ph.astype(F) * self.idx).astype(F)
            phi = np.minimum(phi, ph)
        return phi, phi < 0

    def inside(self, x):
        return self.phi(x)[1]


class SeedModel2D:
    def __init__(self, res, dx, region, ppc=4.0, velocity=(0.0, 0.0), source=False, delta_t=1e-3, current_t=0.0,
                 gravity=(0.0, -10.0), base_dt=1e-4, tile=None):
        self.res = np.array([res] * 2 if np.isscalar(res) else res, np.int64)
        self.dx, self.idx = F(dx), F(1.0) / F(dx)
        self.region = region
        self.tile = load_tile() if tile is None else np.asarray(tile, F)
        self.source = bool(source)
        self.velocity = np.asarray(velocity, F)
        self.offset = (self.velocity * F(current_t)).astype(F)
        d, g = F(delta_t), np.asarray(gravity, F)
        self.advection = ((self.velocity * d).astype(F) + (((F(0.5) * g).astype(F) * F(d + F(base_dt))).astype(F) * d).astype(F)).astype(F)
        self._get_ready(float(F(ppc)))

    def _get_ready(self, ppc):
        ax = [((np.arange(r).astype(F) + F(0.5)) * self.dx).astype(F) for r in self.res]
        pts = np.stack(np.meshgrid(ax[0], ax[1], indexing="ij"), axis=-1).reshape(-1, 2)
        any_inside = self.region.inside(pts).reshape(len(ax[0]), len(ax[1]))
        self.empty = not any_inside.any()
        if self.empty:
            return
        idx = np.argwhere(any_inside)
        lo, hi = idx.min(axis=0), idx.max(axis=0)
        self.min_corner = np.array([ax[k][lo[k]] - self.dx for k in range(2)], F)
        self.max_corner = np.array([ax[k][hi[k]] + self.dx for k in range(2)], F)
        dx = float(self.dx)
        self.min_distance = F(np.sqrt(dx * dx / ppc * 2.0 / 3.0))
        self.region_size = F(F(40.0) * self.min_distance)
        self.nrep = np.maximum(1, np.ceil(((self.max_corner - self.min_corner).astype(F) / self.region_size).astype(F)).astype(np.int64))
        self.n_rep = int(np.prod(self.nrep))
        self.n_cand = self.n_rep * len(self.tile)

    def near_boundary(self, x):
        X = (x * self.idx).astype(F)
        return (X.min(axis=1) < F(7.0)) | ((X - self.res.astype(F)[None, :]).astype(F).max(axis=1) > F(-7.0))

    def positions(self, lo=0, hi=None):
        """positions of the candidates c = i * n_replicas + r for the tile points lo <= i < hi, (n, 2) fp32 in the order of c"""
        q = (self.tile[lo:hi] * self.min_distance).astype(F)
        rs = self.region_size
        if self.source:
            q = (q + self.offset[None, :]).astype(F)
            w = np.floor(((q / rs).astype(F) + F(0.5)).astype(F)).astype(F)
            q = (q - (w * rs).astype(F)).astype(F)
        a = (q + self.min_corner[None, :]).astype(F)
        ind = np.stack(np.meshgrid(*[np.arange(n) for n in self.nrep], indexing="ij"), axis=-1).reshape(-1, 2)
        b = (rs * (ind.astype(F) + F(0.5)).astype(F)).astype(F)
        return (a[:, None, :] + b[None, :, :]).astype(F).reshape(-1, 2)

    def run(self, margin=None):
        """-> dict(x (n, 2) fp32 survivors in order, c their candidate numbers, n_cand, unsure: candidate numbers with
        |phi| < margin (grid units) at the position — or, source mode, at the advected position — when a margin is given)"""
        x = self.positions()
        c = np.arange(len(x), dtype=np.int64)
        phi, ins = self.region.phi(x)
        keep = ins & ~self.near_boundary(x)
        out = dict(n_cand=self.n_cand)
        if margin is not None:
            near = np.abs(phi) < F(margin)
        if self.source:
            phi2, ins2 = self.region.phi((x + self.advection[None, :]).astype(F))
            keep &= ~ins2
            if margin is not None:
                near |= np.abs(phi2) < F(margin)
        out.update(x=x[keep], c=c[keep])
        if margin is not None:
            out["unsure"] = c[near]
        return out
