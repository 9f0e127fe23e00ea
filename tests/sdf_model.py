"""numpy model of the sampled level set's sampler in space and in the plane (include/mpmhip.h: mpmhip_set_levelset_sdf,
mpmhip2d_set_levelset_sdf; csrc/mpm_math.h: the sdf_* templates) — the yardstick of the sampler tests of both dimensions.  The
dimension D is phi0.ndim.  In fp32 and in the device's order of operations:

  locate    u = (x - origin) * (1 / spacing);  no level set unless 0 <= u <= res - 1 on every axis;
            cell c = clip(trunc(u), 0, res - 2), f = u - c
  lerp      (1 - f) * a + f * b
  phi       the cell's 2^D samples interpolated along the last axis first and the first axis last; times 1 / dx
  gradient  per sample (phi[+1] - phi[-1]) * (w / spacing), w = 1/2 (1 on the array's faces, one-sided); the 2^D gradients
            interpolated like phi; normalised (the squares summed from axis 0 upward), a length below 1e-10 gives the zero vector
  two key frames   a = (t - t0) / (t1 - t0);  phi = (1 - a) phi0 + a phi1;  d phi / dt = (phi1 - phi0) / (t1 - t0);
            normal = normalised (n0 (1 - a) + n1 a) of the two UNIT gradients

The device's sampler forbids the contraction of a multiply and an add (csrc/mpm_math.h: SDF_NO_CONTRACT), so every operation here
is rounded on its own and the device is held to the model's bits.  The model itself is checked against closed forms in
tests/test_sdf_cpu.py and tests/test_sdf2d_cpu.py, and its sign against the seeding's sampled region (tests/seed2d_model.py)."""
import itertools

import numpy as np

F = np.float32


class SdfModel:
    def __init__(self, phi0, origin, spacing, dx, phi1=None, t0=0.0, t1=1.0):
        self.phi0 = np.ascontiguousarray(phi0, F)
        self.phi1 = None if phi1 is None else np.ascontiguousarray(phi1, F)
        self.dim = self.phi0.ndim
        self.res = np.array(self.phi0.shape, np.int64)
        self.origin = np.asarray(origin, F)
        assert self.dim in (2, 3) and self.origin.shape == (self.dim,)
        self.inv_spacing = F(1.0) / F(spacing)
        self.idx = F(1.0) / F(dx)
        self.t0, self.t1 = F(t0), F(t1)

    def frames(self):
        return [p for p in (self.phi0, self.phi1) if p is not None]

    def locate(self, x):
        x = np.asarray(x, F).reshape(-1, self.dim)
        u = ((x - self.origin[None, :]).astype(F) * self.inv_spacing).astype(F)
        hit = np.all((u >= 0) & (u <= (self.res - 1).astype(F)[None, :]), axis=1)
        with np.errstate(invalid="ignore"):
            c = np.clip(np.trunc(np.where(np.isfinite(u), u, 0)).astype(np.int64), 0, (self.res - 2)[None, :])
        f = (u - c.astype(F)).astype(F)
        return hit, c, f

    @staticmethod
    def _lerp(a, b, f):
        return (((F(1.0) - f).astype(F) * a).astype(F) + (f * b).astype(F)).astype(F)

    def _sample_grad(self, p, i):
        """central differences at the samples i (n, D) -> (n, D)"""
        g = []
        for ax in range(self.dim):
            lo, hi = i.copy(), i.copy()
            lo[:, ax] = np.maximum(i[:, ax] - 1, 0)
            hi[:, ax] = np.minimum(i[:, ax] + 1, self.res[ax] - 1)
            w = (np.where(hi[:, ax] - lo[:, ax] == 2, F(0.5), F(1.0)).astype(F) * self.inv_spacing).astype(F)
            g.append(((p[tuple(hi.T)] - p[tuple(lo.T)]).astype(F) * w).astype(F))
        return np.stack(g, axis=-1)

    def _corners(self, c):
        """the 2^D samples of each cell: offset tuple -> indices (n, D)"""
        return {o: c + np.array(o, np.int64) for o in itertools.product((0, 1), repeat=self.dim)}

    def _interp(self, at, c, f):
        """at(samples (n, D)) -> values (n,) or (n, D), interpolated in the cells c: the last axis first, the first axis last"""
        v = {o: at(i) for o, i in self._corners(c).items()}
        for ax in reversed(range(self.dim)):
            w = f[:, ax]
            v = {o: self._lerp(v[o + (0,)], v[o + (1,)], w if v[o + (0,)].ndim == 1 else w[:, None])
                 for o in itertools.product((0, 1), repeat=ax)}
        return v[()]

    def _phi_frame(self, p, c, f):
        return self._interp(lambda i: p[tuple(i.T)], c, f)

    @staticmethod
    def _normalize(g):
        s = (g[:, 0] * g[:, 0]).astype(F)
        for k in range(1, g.shape[1]):
            s = (s + (g[:, k] * g[:, k]).astype(F)).astype(F)
        ln = np.sqrt(s).astype(F)
        with np.errstate(divide="ignore"):
            inv = np.where(ln < F(1e-10), F(0), F(1.0) / np.where(ln == 0, F(1), ln)).astype(F)
        return (g * inv[:, None]).astype(F)

    def raw_gradient(self, p, c, f):
        """the interpolated gradient of one frame before it is normalised"""
        return self._interp(lambda i: self._sample_grad(p, i), c, f)

    def cell_max_abs(self, c):
        """max |phi| (grid units) over the 2^D samples of each cell, over both frames"""
        out = np.zeros(len(c), F)
        for p in self.frames():
            for i in self._corners(c).values():
                out = np.maximum(out, np.abs((p[tuple(i.T)] * self.idx).astype(F)))
        return out

    def cell_max_grad(self, c):
        """largest |component| of the 2^D samples' gradients of each cell, over both frames"""
        out = np.zeros(len(c), F)
        for p in self.frames():
            for i in self._corners(c).values():
                out = np.maximum(out, np.abs(self._sample_grad(p, i)).max(axis=1))
        return out

    def sample(self, x, t=0.0):
        """-> phi (grid units), unit gradient (n, D), d phi / dt, hit; rows without a hit are zero"""
        hit, c, f = self.locate(x)
        p0 = self._phi_frame(self.phi0, c, f)
        n = self._normalize(self.raw_gradient(self.phi0, c, f))
        dphidt = np.zeros(len(p0), F)
        if self.phi1 is None:
            phi = (p0 * self.idx).astype(F)
        else:
            p0 = (p0 * self.idx).astype(F)
            p1 = (self._phi_frame(self.phi1, c, f) * self.idx).astype(F)
            a = F(F(F(t) - self.t0) / F(self.t1 - self.t0))
            dphidt = ((p1 - p0).astype(F) / F(self.t1 - self.t0)).astype(F)
            phi = (((F(1.0) - a) * p0).astype(F) + (a * p1).astype(F)).astype(F)
            n1 = self._normalize(self.raw_gradient(self.phi1, c, f))
            n = self._normalize(((n * F(F(1.0) - a)).astype(F) + (n1 * a).astype(F)).astype(F))
        z = ~hit
        phi[z] = 0
        n[z] = 0
        dphidt[z] = 0
        return phi, n, dphidt, hit

    def inside(self, x, t=0.0):
        """where a particle counts as inside the solid: a level set there and phi < 0"""
        phi, _, _, hit = self.sample(x, t)
        return hit & (phi < 0)

    def projection_residual(self, x, dx, t=0.0):
        """particle_collision pushes a particle with phi < 0 by -phi n dx.  For the points of x with -1 < phi < 0: the largest depth
        (cells) that is LEFT after one push, max(0, -phi(x - phi n dx)) — what the interpolated normal and the curvature of the
        interpolant cost in a single step."""
        phi, n, _, hit = self.sample(x, t)
        m = hit & (phi < 0) & (phi > -1)
        if not m.any():
            return 0.0
        xp = (np.asarray(x, F).reshape(-1, self.dim)[m] - n[m] * (phi[m] * F(dx))[:, None]).astype(F)
        phi2, _, _, hit2 = self.sample(xp, t)
        return float(np.max(np.where(hit2, np.maximum(-phi2, 0), 0), initial=0.0))


# ---- what the device sampler tests of both dimensions (tests/test_gpu_sdf.py, tests/test_gpu_sdf2d.py:
# test_device_sampler_matches_the_model) and the 2D one's CPU companion share
def sampler_points(rng, n, res, origin, spacing):
    """n points for a lattice: inside cells, on cell faces, exactly on samples, outside the lattice (and a NaN)"""
    res, org = np.array(res), np.array(origin)
    dim = len(res)
    hi = org + (res - 1) * spacing
    inside = rng.uniform(org, hi, (n // 2, dim))
    face = rng.uniform(org, hi, (n // 5, dim))
    ax = rng.integers(0, dim, len(face))
    face[np.arange(len(face)), ax] = org[ax] + rng.integers(0, res[ax], len(face)) * spacing
    on = org + np.stack([rng.integers(0, res[k], n // 5) for k in range(dim)], 1) * spacing
    out = rng.uniform(org - 0.2, hi + 0.2, (n - len(inside) - len(face) - len(on), dim))
    x = np.concatenate([inside, face, on, out]).astype(F)
    x[-1] = 0.3
    x[-1, 0] = np.nan
    return x


def well_conditioned(model, x, t=None):
    """the points where the normal is compared: a hit, and the raw gradient g of every frame has G <= 2 |g| (G: the largest
    component among the cell's samples' gradients), and with two frames (t given) the blend of the unit normals is no shorter
    than 0.97.  -> hit, well"""
    hit, c, f = model.locate(x)
    G = model.cell_max_grad(c)
    raw = model.raw_gradient(model.phi0, c, f)
    well = hit & (G <= 2 * np.linalg.norm(raw, axis=1))
    if t is not None:
        raw1 = model.raw_gradient(model.phi1, c, f)
        well &= G <= 2 * np.linalg.norm(raw1, axis=1)
        n0 = raw / np.maximum(np.linalg.norm(raw, axis=1), 1e-30)[:, None]
        n1 = raw1 / np.maximum(np.linalg.norm(raw1, axis=1), 1e-30)[:, None]
        a = (t - float(model.t0)) / (float(model.t1) - float(model.t0))
        well &= np.linalg.norm(n0 * (1 - a) + n1 * a, axis=1) >= 0.97
    return hit, well
