"""numpy model of the 2D sampled level set's sampler (include/mpmhip.h: mpmhip2d_set_levelset_sdf; csrc/mpm_math.h: sdf2_*) — the
yardstick of the 2D sampler tests.  tests/sdf_model.py with one axis fewer: in fp32 and in the device's order of operations

  locate    u = (x - origin) * (1 / spacing);  no level set unless 0 <= u <= res - 1 on both axes;
            cell c = clip(trunc(u), 0, res - 2), f = u - c
  lerp      (1 - f) * a + f * b
  phi       the cell's four samples interpolated along the last axis, then the first; times 1 / dx
  gradient  per sample (phi[+1] - phi[-1]) * (w / spacing), w = 1/2 (1 on the array's edges, one-sided); the four gradients
            interpolated like phi; normalised, a length below 1e-10 gives the zero vector
  two key frames   a = (t - t0) / (t1 - t0);  phi = (1 - a) phi0 + a phi1;  d phi / dt = (phi1 - phi0) / (t1 - t0);
            normal = normalised (n0 (1 - a) + n1 a) of the two UNIT gradients

The device's sampler forbids the contraction of a multiply and an add (csrc/mpm_math.h: SDF_NO_CONTRACT), so every operation here
is rounded on its own.  The model is checked against closed forms, and its sign against the seeding's sampled region
(tests/seed2d_model.py), in tests/test_sdf2d_cpu.py."""
import numpy as np

F = np.float32


class Sdf2DModel:
    def __init__(self, phi0, origin, spacing, dx, phi1=None, t0=0.0, t1=1.0):
        self.phi0 = np.ascontiguousarray(phi0, F)
        self.phi1 = None if phi1 is None else np.ascontiguousarray(phi1, F)
        assert self.phi0.ndim == 2
        self.res = np.array(self.phi0.shape, np.int64)
        self.origin = np.asarray(origin, F)
        self.inv_spacing = F(1.0) / F(spacing)
        self.idx = F(1.0) / F(dx)
        self.t0, self.t1 = F(t0), F(t1)

    def locate(self, x):
        x = np.asarray(x, F).reshape(-1, 2)
        u = ((x - self.origin[None, :]).astype(F) * self.inv_spacing).astype(F)
        hit = np.all((u >= 0) & (u <= (self.res - 1).astype(F)[None, :]), axis=1)
        with np.errstate(invalid="ignore"):
            c = np.clip(np.trunc(np.where(np.isfinite(u), u, 0)).astype(np.int64), 0, (self.res - 2)[None, :])
        f = (u - c.astype(F)).astype(F)
        return hit, c, f

    @staticmethod
    def _lerp(a, b, f):
        return (((F(1.0) - f).astype(F) * a).astype(F) + (f * b).astype(F)).astype(F)

    def _sample_grad(self, p, i, j):
        idx = [i, j]
        g = []
        for ax in range(2):
            m = [q.copy() for q in idx]
            pl = [q.copy() for q in idx]
            m[ax] = np.maximum(idx[ax] - 1, 0)
            pl[ax] = np.minimum(idx[ax] + 1, self.res[ax] - 1)
            w = (np.where(pl[ax] - m[ax] == 2, F(0.5), F(1.0)).astype(F) * self.inv_spacing).astype(F)
            g.append(((p[pl[0], pl[1]] - p[m[0], m[1]]).astype(F) * w).astype(F))
        return np.stack(g, axis=-1)

    def _bi(self, corner, f):
        """corner(i, j offsets) -> values (n,) or (n, 2); the device's order: the last axis, then the first"""
        def L(a, b, w):
            return self._lerp(a, b, w if a.ndim == 1 else w[:, None])
        a = [L(corner(i, 0), corner(i, 1), f[:, 1]) for i in (0, 1)]
        return L(a[0], a[1], f[:, 0])

    def _phi_frame(self, p, c, f):
        return self._bi(lambda i, j: p[c[:, 0] + i, c[:, 1] + j], f)

    @staticmethod
    def _normalize(g):
        ln = np.sqrt(((g[:, 0] * g[:, 0]).astype(F) + (g[:, 1] * g[:, 1]).astype(F)).astype(F)).astype(F)
        with np.errstate(divide="ignore"):
            inv = np.where(ln < F(1e-10), F(0), F(1.0) / np.where(ln == 0, F(1), ln)).astype(F)
        return (g * inv[:, None]).astype(F)

    def raw_gradient(self, p, c, f):
        """the interpolated gradient of one frame before it is normalised"""
        return self._bi(lambda i, j: self._sample_grad(p, c[:, 0] + i, c[:, 1] + j), f)

    def cell_max_abs(self, c):
        """max |phi| (grid units) over the four samples of each cell, over both frames"""
        out = np.zeros(len(c), F)
        for p in (self.phi0, self.phi1):
            if p is None:
                continue
            for i in (0, 1):
                for j in (0, 1):
                    out = np.maximum(out, np.abs((p[c[:, 0] + i, c[:, 1] + j] * self.idx).astype(F)))
        return out

    def cell_max_grad(self, c):
        """largest |component| of the four samples' gradients of each cell, over both frames"""
        out = np.zeros(len(c), F)
        for p in (self.phi0, self.phi1):
            if p is None:
                continue
            for i in (0, 1):
                for j in (0, 1):
                    out = np.maximum(out, np.abs(self._sample_grad(p, c[:, 0] + i, c[:, 1] + j)).max(axis=1))
        return out

    def sample(self, x, t=0.0):
        """-> phi (grid units), unit gradient (n, 2), d phi / dt, hit; rows without a hit are zero"""
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
        xp = (np.asarray(x, F).reshape(-1, 2)[m] - n[m] * (phi[m] * F(dx))[:, None]).astype(F)
        phi2, _, _, hit2 = self.sample(xp, t)
        return float(np.max(np.where(hit2, np.maximum(-phi2, 0), 0), initial=0.0))


# ---- the lattice, fields and points of the device sampler test (tests/test_gpu_sdf2d.py::test_device_sampler_matches_the_model) and of
# its CPU companion (tests/test_sdf2d_cpu.py::test_the_sampler_tests_fields_are_well_conditioned):
# a shifted origin, a spacing that is not dx
RES1, ORG1, H1 = (83, 77), (-0.1, 0.02), 0.013
T0, T1, TIMES = 0.5, 2.0, (0.7, 1.25, 1.9)


def sampler_fields():
    line = lambda n, d: (lambda x: x @ np.asarray(n, np.float64) + d)
    disc = lambda c, r: (lambda x: np.linalg.norm(x - np.asarray(c, np.float64), axis=1) - r)
    ring = lambda c, R, w: (lambda x: np.abs(np.linalg.norm(x - np.asarray(c, np.float64), axis=1) - R) - w)
    return {"line": (line((0.6, 0.8), -0.6), line((0.6, 0.8), -0.63)),
            "disc": (disc((0.4, 0.5), 0.3), disc((0.42, 0.5), 0.33)),
            "ring": (ring((0.42, 0.5), 0.3, 0.08), ring((0.42, 0.52), 0.31, 0.09))}


def sampler_points(rng, n):
    """inside cells, on lattice lines, exactly on samples, outside the lattice (and a NaN)"""
    res, org = np.array(RES1), np.array(ORG1)
    hi = org + (res - 1) * H1
    inside = rng.uniform(org, hi, (n // 2, 2))
    line = rng.uniform(org, hi, (n // 5, 2))
    ax = rng.integers(0, 2, len(line))
    line[np.arange(len(line)), ax] = org[ax] + rng.integers(0, res[ax], len(line)) * H1
    on = org + np.stack([rng.integers(0, res[k], n // 5) for k in range(2)], 1) * H1
    out = rng.uniform(org - 0.2, hi + 0.2, (n - len(inside) - len(line) - len(on), 2))
    x = np.concatenate([inside, line, on, out]).astype(F)
    x[-1] = (np.nan, 0.3)
    return x


def well_conditioned(model, x, t=None):
    """the points where the normal is compared: a hit, and the raw gradient g of every frame has G <= 2 |g| (G: the largest
    component among the cell's samples' gradients), and with two frames the blend of the unit normals is no shorter than 0.97"""
    hit, c, f = model.locate(x)
    G = model.cell_max_grad(c)
    raw = model.raw_gradient(model.phi0, c, f)
    well = hit & (G <= 2 * np.linalg.norm(raw, axis=1))
    if t is not None:
        raw1 = model.raw_gradient(model.phi1, c, f)
        well &= G <= 2 * np.linalg.norm(raw1, axis=1)
        n0 = raw / np.maximum(np.linalg.norm(raw, axis=1), 1e-30)[:, None]
        n1 = raw1 / np.maximum(np.linalg.norm(raw1, axis=1), 1e-30)[:, None]
        a = (t - T0) / (T1 - T0)
        well &= np.linalg.norm(n0 * (1 - a) + n1 * a, axis=1) >= 0.97
    return hit, well
