"""numpy model of the sampled level set's sampler (include/mpmhip.h: mpmhip_set_levelset_sdf; csrc/mpm_math.h: sdf_*) — the yardstick
of the sampler tests.  It evaluates, in fp32 and in the device's order of operations, the same convex combinations:

  locate    u = (x - origin) * (1 / spacing);  no level set unless 0 <= u <= res - 1 on every axis;
            cell c = clip(trunc(u), 0, res - 2), f = u - c
  lerp      (1 - f) * a + f * b
  phi       the cell's eight samples interpolated along the last axis, then the middle one, then the first; times 1 / dx
  gradient  per sample (phi[+1] - phi[-1]) * (w / spacing), w = 1/2 (1 on the array's faces, one-sided); the eight gradients
            interpolated like phi; normalised, a length below 1e-10 gives the zero vector
  two key frames   a = (t - t0) / (t1 - t0);  phi = (1 - a) phi0 + a phi1;  d phi / dt = (phi1 - phi0) / (t1 - t0);
            normal = normalised (n0 (1 - a) + n1 a) of the two UNIT gradients

The one thing a compiler could do differently is contract a multiply and an add into one fused operation; the tests' tolerances
are derived from that.  (The device's sampler forbids the contraction, csrc/mpm_math.h: SDF_NO_CONTRACT, so that every kernel
that inlines it computes the same bits.)  The model itself is checked against closed forms in tests/test_sdf_cpu.py."""
import numpy as np

F = np.float32


class SdfModel:
    def __init__(self, phi0, origin, spacing, dx, phi1=None, t0=0.0, t1=1.0):
        self.phi0 = np.ascontiguousarray(phi0, F)
        self.phi1 = None if phi1 is None else np.ascontiguousarray(phi1, F)
        self.res = np.array(self.phi0.shape, np.int64)
        self.origin = np.asarray(origin, F)
        self.inv_spacing = F(1.0) / F(spacing)
        self.idx = F(1.0) / F(dx)
        self.t0, self.t1 = F(t0), F(t1)

    def locate(self, x):
        x = np.asarray(x, F).reshape(-1, 3)
        u = (x - self.origin[None, :]) * self.inv_spacing
        hit = np.all((u >= 0) & (u <= (self.res - 1).astype(F)[None, :]), axis=1)
        with np.errstate(invalid="ignore"):
            c = np.clip(np.trunc(np.where(np.isfinite(u), u, 0)).astype(np.int64), 0, (self.res - 2)[None, :])
        f = (u - c.astype(F)).astype(F)
        return hit, c, f

    @staticmethod
    def _lerp(a, b, f):
        return ((F(1.0) - f) * a + f * b).astype(F)

    def _sample_grad(self, p, i, j, k):
        idx = [i, j, k]
        g = []
        for ax in range(3):
            m = [q.copy() for q in idx]
            pl = [q.copy() for q in idx]
            m[ax] = np.maximum(idx[ax] - 1, 0)
            pl[ax] = np.minimum(idx[ax] + 1, self.res[ax] - 1)
            w = np.where(pl[ax] - m[ax] == 2, F(0.5), F(1.0)).astype(F) * self.inv_spacing
            g.append(((p[pl[0], pl[1], pl[2]] - p[m[0], m[1], m[2]]).astype(F) * w).astype(F))
        return np.stack(g, axis=-1)

    def _tri(self, corner, f):
        """corner(i, j, k offsets) -> values (n,) or (n, 3); the device's order: last axis, middle, first"""
        def L(a, b, w):
            return self._lerp(a, b, w if a.ndim == 1 else w[:, None])
        a = []
        for i in (0, 1):
            b = [L(corner(i, j, 0), corner(i, j, 1), f[:, 2]) for j in (0, 1)]
            a.append(L(b[0], b[1], f[:, 1]))
        return L(a[0], a[1], f[:, 0])

    def _phi_frame(self, p, c, f):
        return self._tri(lambda i, j, k: p[c[:, 0] + i, c[:, 1] + j, c[:, 2] + k], f)

    @staticmethod
    def _normalize(g):
        ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]).astype(F)).astype(F)
        with np.errstate(divide="ignore"):
            inv = np.where(ln < F(1e-10), F(0), F(1.0) / np.where(ln == 0, F(1), ln)).astype(F)
        return (g * inv[:, None]).astype(F)

    def raw_gradient(self, p, c, f):
        """the interpolated gradient of one frame before it is normalised"""
        return self._tri(lambda i, j, k: self._sample_grad(p, c[:, 0] + i, c[:, 1] + j, c[:, 2] + k), f)

    def cell_max_abs(self, c):
        """max |phi| (grid units) over the eight samples of each cell, over both frames"""
        out = np.zeros(len(c), F)
        for p in (self.phi0, self.phi1):
            if p is None:
                continue
            for i in (0, 1):
                for j in (0, 1):
                    for k in (0, 1):
                        out = np.maximum(out, np.abs(p[c[:, 0] + i, c[:, 1] + j, c[:, 2] + k] * self.idx))
        return out

    def cell_max_grad(self, c):
        """largest |component| of the eight samples' gradients of each cell, over both frames"""
        out = np.zeros(len(c), F)
        for p in (self.phi0, self.phi1):
            if p is None:
                continue
            for i in (0, 1):
                for j in (0, 1):
                    for k in (0, 1):
                        out = np.maximum(out, np.abs(self._sample_grad(p, c[:, 0] + i, c[:, 1] + j, c[:, 2] + k)).max(axis=1))
        return out

    def sample(self, x, t=0.0):
        """-> phi (grid units), unit gradient, d phi / dt, hit; rows without a hit are zero"""
        hit, c, f = self.locate(x)
        p0 = self._phi_frame(self.phi0, c, f)
        n = self._normalize(self.raw_gradient(self.phi0, c, f))
        dphidt = np.zeros(len(p0), F)
        if self.phi1 is None:
            phi = (p0 * self.idx).astype(F)
        else:
            p0 = (p0 * self.idx).astype(F)
            p1 = (self._phi_frame(self.phi1, c, f) * self.idx).astype(F)
            a = F((F(t) - self.t0) / (self.t1 - self.t0))
            dphidt = ((p1 - p0) / (self.t1 - self.t0)).astype(F)
            phi = ((F(1.0) - a) * p0 + a * p1).astype(F)
            n1 = self._normalize(self.raw_gradient(self.phi1, c, f))
            n = self._normalize((n * (F(1.0) - a) + n1 * a).astype(F))
        z = ~hit
        phi[z] = 0
        n[z] = 0
        dphidt[z] = 0
        return phi, n, dphidt, hit

    def projection_residual(self, x, dx, t=0.0):
        """particle_collision pushes a particle with phi < 0 by -phi n dx.  For the points of x with -1 < phi < 0: the largest depth
        (cells) that is LEFT after one push, max(0, -phi(x - phi n dx)) — what the interpolated normal and the curvature of the
        interpolant cost in a single step."""
        phi, n, _, hit = self.sample(x, t)
        m = hit & (phi < 0) & (phi > -1)
        if not m.any():
            return 0.0
        xp = (np.asarray(x, F).reshape(-1, 3)[m] - n[m] * (phi[m] * F(dx))[:, None]).astype(F)
        phi2, _, _, hit2 = self.sample(xp, t)
        return float(np.max(np.where(hit2, np.maximum(-phi2, 0), 0), initial=0.0))
