"""numpy model of the region expressions (include/mpmhip.h, "Region expressions"; csrc/k_region.h: RegionExpr<D>) for D = 2 and 3 — the
yardstick of the region tests.  A leaf's own distance comes from the models of the plain regions (tests/seed_model.py: ShapeRegion,
SampledRegion on tests/sdf_model.py's SdfModel; tests/seed2d_model.py: their 2D twins); this file adds, in fp32 with every operation
rounded and in the device's order:

  placement   d = x - t;  y_k = ((R_0k d_0 + R_1k d_1) + R_2k d_2)  (D = 2: R_0k d_0 + R_1k d_1);
              local_k = (y_k * (1 / s)) + p_k;  phi = phi_leaf(local) * s
              (D = 2: R = [c -s; s c], c = float32(cos(double(angle))), s = float32(sin(double(angle))), angle the fp32 the
              description holds)
  band        phi' = max(lo - phi, phi - hi)
  outside     a sampled leaf outside its lattice: +inf (so -inf after NEG: in the complement)
  operators   UNION = min, INTERSECT = max, NEG = -phi over a postfix program

A sampled leaf is exact (the device's sampler and the placement forbid contraction); a shape leaf is exact up to the contraction
the device's compiler may apply inside levelset_eval_key: tests set candidates within a margin of a leaf surface or band edge aside
(closeness()).  A model is built from explicit leaves and operations, or from the ctypes description the Python layer compiles
(from_desc), which is what the library is handed."""
import math

import numpy as np

from tests.seed2d_model import SampledRegion2D, ShapeRegion2D
from tests.seed_model import SampledRegion, ShapeRegion

F = np.float32
PUSH, UNION, INTERSECT, NEG = 0, 1, 2, 3


class Leaf:
    """base: an object with phi(x) -> (phi grid units [+inf outside a lattice], inside); place: None or dict(R (3, 3) fp32 row-major,
    s, t, p); band: None or (lo, hi)"""

    def __init__(self, base, place=None, band=None):
        self.base, self.place, self.band = base, place, band


def rotation2(angle):
    a = float(F(angle))
    c, s = F(math.cos(a)), F(math.sin(a))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], F)


class RegionModel:
    def __init__(self, dim, dx, leaves, ops):
        """ops: [(PUSH, leaf index) | (UNION,) | (INTERSECT,) | (NEG,)]"""
        self.dim, self.dx, self.idx = int(dim), F(dx), F(1.0) / F(dx)
        self.leaves, self.ops = list(leaves), [tuple(o) for o in ops]

    @classmethod
    def from_desc(cls, d, dim, dx):
        """from a taichi_mpm_amd._lib.RegionDesc"""
        fields = []
        for k in range(d.n_fields):
            f = d.fields[k]
            res = tuple(f.res[:dim])
            phi = np.ctypeslib.as_array(f.phi, shape=res).copy()
            origin = tuple(F(v) for v in f.origin[:dim])
            fields.append(SampledRegion(phi, origin, F(f.spacing), dx) if dim == 3 else SampledRegion2D(phi, origin, F(f.spacing), dx))
        leaves = []
        for k in range(d.n_leaves):
            L = d.leaves[k]
            if L.kind:
                base = fields[L.field]
            else:
                shape = (int(L.shape.type), int(L.shape.inside_out), [F(v) for v in L.shape.p])
                base = ShapeRegion([shape], dx) if dim == 3 else ShapeRegion2D([shape], dx)
            place = None
            if L.placed:
                R = np.array(L.rot[:], F).reshape(3, 3) if dim == 3 else rotation2(L.rot[0])
                place = dict(R=R, s=F(L.scale), t=np.array(L.translate[:dim], F), p=np.array(L.pivot[:dim], F))
            leaves.append(Leaf(base, place, (F(L.lo), F(L.hi)) if L.banded else None))
        return cls(dim, dx, leaves, [(o.op, o.leaf) for o in d.ops[:d.n_ops]])

    def _leaf(self, L, x):
        """(phi of the leaf, how close the point is to the leaf's surface or a band edge), grid units"""
        D = self.dim
        if L.place is not None:
            P = L.place
            R, inv_s = P["R"], F(1.0) / P["s"]
            d = (x - P["t"][None, :]).astype(F)
            local = np.empty_like(x)
            for k in range(D):
                y = ((R[0, k] * d[:, 0]).astype(F) + (R[1, k] * d[:, 1]).astype(F)).astype(F)
                if D == 3:
                    y = (y + (R[2, k] * d[:, 2]).astype(F)).astype(F)
                local[:, k] = ((y * inv_s).astype(F) + P["p"][k]).astype(F)
            with np.errstate(invalid="ignore"):
                phi = (L.base.phi(local)[0].astype(F) * P["s"]).astype(F)
        else:
            phi = L.base.phi(x)[0].astype(F)
        close = np.abs(phi)
        if L.band is not None:
            lo, hi = L.band
            a, b = (lo - phi).astype(F), (phi - hi).astype(F)
            close = np.minimum(close, np.minimum(np.abs(a), np.abs(b)))
            phi = np.maximum(a, b)
        return phi, close

    def _run(self, x):
        x = np.ascontiguousarray(x, F).reshape(-1, self.dim)
        stack, close = [], np.full(len(x), F(np.inf), F)
        for op in self.ops:
            if op[0] == PUSH:
                v, c = self._leaf(self.leaves[op[1]], x)
                close = np.minimum(close, c)
                stack.append(v)
            elif op[0] == NEG:
                stack[-1] = -stack[-1]
            else:
                b, a = stack.pop(), stack.pop()
                stack.append(np.minimum(a, b) if op[0] == UNION else np.maximum(a, b))
        assert len(stack) == 1
        return stack[0], close

    def phi(self, x):
        """(phi in grid units, inside flags) — the protocol of the seeding models' regions"""
        v = self._run(x)[0]
        return v, v < 0

    def inside(self, x):
        return self.phi(x)[1]

    def closeness(self, x):
        """min over the leaves of |leaf value| and of the two band-edge differences: a point below the margin is set aside"""
        return self._run(x)[1]

    def margin_view(self):
        """this region for a seeding model's run(margin=...): phi() reports the closeness in place of phi, so that the model's
        |phi| < margin sets aside what the protocol says; inside is unchanged"""
        return _MarginView(self)

    def bake(self, res, origin, spacing, band):
        """phi at the nodes fl(origin + fl(i * spacing)) in world units, fl(phi * dx), clamped to +-band; shape res"""
        ax = [(F(origin[k]) + (np.arange(res[k]).astype(F) * F(spacing)).astype(F)).astype(F) for k in range(self.dim)]
        pts = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, self.dim)
        out = np.empty(len(pts), F)
        for i in range(0, len(pts), 1 << 16):
            w = (self.phi(pts[i:i + (1 << 16)])[0] * self.dx).astype(F)
            out[i:i + (1 << 16)] = np.minimum(np.maximum(w, -F(band)), F(band))
        return out.reshape(tuple(res))


class _MarginView:
    def __init__(self, m):
        self.m = m

    def phi(self, x):
        v, close = self.m._run(x)
        return close, v < 0

    def inside(self, x):
        return self.m.inside(x)
