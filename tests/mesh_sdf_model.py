"""Numpy model of the mesh voxeliser's rules (include/mpmhip.h: mpmhip_mesh_to_sdf) — the yardstick of tests/test_mesh_sdf_cpu.py
and tests/test_gpu_mesh_sdf.py — and the closed meshes, with their closed-form distances, those tests use.

    phi = s * min(d, band) at the samples of a lattice; sample i of an axis sits at fl32(origin + fl32(i * spacing)).
    d   distance to the nearest triangle: closest point by the regions (vertex a, b, edge ab, vertex c, edge ac, edge bc, face, in
        that order) after the triangle's vertices were put in lexicographic order; zero-area triangles are skipped.  Evaluated in
        `dtype`: float64 is the model, float32 its transcription of the device's arithmetic (same expressions, same order; numpy
        fuses nothing).
    s   -1 iff an odd number of triangles cross the column above the sample.  A column lies in a triangle's xy-projection iff the ray
        towards +x crosses an odd number of its projected edges: exactly one end point has y' > y, and the edge function taken from
        the lower end point is > 0.  Always float64 on the float32 inputs (exact).  The crossing height is interpolated in float64
        and sample k is below it iff height > z_k.

The distance search prunes with bounding spheres (a triangle farther than the best upper bound cannot be the nearest); the pruning
has slack far above any rounding, so it changes no result."""
import numpy as np


# ------------------------------------------------------------------------------------------------------------------ the lattice
def lattice_axes(res, origin, spacing):
    """the three axes' sample coordinates as the device computes them (float32)"""
    return [np.float32(origin[k]) + np.arange(int(res[k]), dtype=np.float32) * np.float32(spacing) for k in range(3)]


def lattice_points(res, origin, spacing):
    """(n, 3) float64: the float32 sample positions in the array's order"""
    ax = [a.astype(np.float64) for a in lattice_axes(res, origin, spacing)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)


def canonical(tri):
    """every triangle's vertices in lexicographic (x, y, z) order"""
    t = np.asarray(tri)
    order = np.lexsort((t[:, :, 2], t[:, :, 1], t[:, :, 0]), axis=1)
    return np.take_along_axis(t, order[:, :, None], axis=1)


# ------------------------------------------------------------------------------------------------------------------ distance
def _records(tri, dtype):
    t = canonical(np.asarray(tri, dtype))
    a, ab, ac = t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    n = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                  ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], 1)
    dot = lambda u, v: (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]
    valid = np.any(n != 0, axis=1)
    return (a[valid], ab[valid], ac[valid], dot(ab, ab)[valid], dot(ab, ac)[valid], dot(ac, ac)[valid]), valid


def _dist2_pairs(a, ab, ac, abab, abac, acac, p):
    """squared distance of point p[m] to triangle record m, all arrays of one dtype: the expressions of msdf_dist2 (k_mesh_sdf.h)"""
    one, zero = np.ones_like(abab), np.zeros_like(abab)
    ap = p - a
    d1 = (ab[:, 0] * ap[:, 0] + ab[:, 1] * ap[:, 1]) + ab[:, 2] * ap[:, 2]
    d2 = (ac[:, 0] * ap[:, 0] + ac[:, 1] * ap[:, 1]) + ac[:, 2] * ap[:, 2]
    d3, d4, d5, d6 = d1 - abab, d2 - abac, d1 - abac, d2 - acac
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    t1, t2 = d4 - d3, d5 - d6
    nv, nw, den = vb, vc, (va + vb) + vc
    for cond, cv, cw, cd in (((va <= 0) & (t1 >= 0) & (t2 >= 0), t2, t1, t1 + t2),
                             ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2, d2 - d6),
                             ((d6 >= 0) & (d5 <= d6), zero, one, one),
                             ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, zero, d1 - d3),
                             ((d3 >= 0) & (d4 <= d3), one, zero, one),
                             ((d1 <= 0) & (d2 <= 0), zero, zero, one)):
        nv, nw, den = np.where(cond, cv, nv), np.where(cond, cw, nw), np.where(cond, cd, den)
    with np.errstate(divide="ignore", invalid="ignore"):
        v, w = nv / den, nw / den
    r = (ap - v[:, None] * ab) - w[:, None] * ac
    return (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]


def distance(tri, pts, dtype=np.float64, chunk=1024):
    """distance from every point (n, 3) to the nearest triangle, computed in dtype"""
    rec, valid = _records(tri, dtype)
    if not valid.any():
        return np.full(len(pts), np.inf, dtype)
    t64 = canonical(np.asarray(tri, np.float64))[valid]
    cen = t64.mean(axis=1)
    rad = np.linalg.norm(t64 - cen[:, None, :], axis=2).max(axis=1)
    p64 = np.asarray(pts, np.float64)
    out = np.empty(len(p64), dtype)
    for s in range(0, len(p64), chunk):
        q = p64[s:s + chunk]
        D = np.linalg.norm(q[:, None, :] - cen[None, :, :], axis=2)
        ub = (D + rad).min(axis=1)
        pi, ti = np.nonzero(D - rad <= ub[:, None] * (1 + 1e-5) + 1e-9)  # row-major: grouped by point, every point has a pair
        d2 = _dist2_pairs(*(r[ti] for r in rec), q[pi].astype(dtype))
        d2 = np.where(np.isnan(d2), np.inf, d2)
        starts = np.searchsorted(pi, np.arange(len(q)))
        out[s:s + chunk] = np.sqrt(np.minimum.reduceat(d2, starts))
    return out


# ------------------------------------------------------------------------------------------------------------------ parity
def _edge_cross(ax, ay, bx, by, px, py):
    if ay > by:
        ax, ay, bx, by = bx, by, ax, ay
    straddle = (ay > py) != (by > py)
    return straddle & ((bx - ax) * (py - ay) - (by - ay) * (px - ax) > 0)


def parity(tri, res, origin, spacing):
    """(inside [res] bool, number of columns with an odd total of crossings)"""
    X, Y, Z = [a.astype(np.float64) for a in lattice_axes(res, origin, spacing)]
    t = canonical(np.asarray(tri, np.float64))
    T = np.zeros((len(X), len(Y), len(Z) + 1), np.int64)
    for (x0, y0, z0), (x1, y1, z1), (x2, y2, z2) in t:
        area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
        if area == 0:
            continue
        i0, i1 = np.searchsorted(X, min(x0, x1, x2), "left"), np.searchsorted(X, max(x0, x1, x2), "right")
        j0, j1 = np.searchsorted(Y, min(y0, y1, y2), "left"), np.searchsorted(Y, max(y0, y1, y2), "right")
        if i0 >= i1 or j0 >= j1:
            continue
        px, py = X[i0:i1, None], Y[None, j0:j1]
        inside = _edge_cross(x0, y0, x1, y1, px, py) ^ _edge_cross(x1, y1, x2, y2, px, py) ^ _edge_cross(x0, y0, x2, y2, px, py)
        ii, jj = np.nonzero(inside)
        if len(ii) == 0:
            continue
        qx, qy = X[i0 + ii], Y[j0 + jj]
        e1 = (x0 - x2) * (qy - y2) - (y0 - y2) * (qx - x2)
        e2 = (x1 - x0) * (qy - y0) - (y1 - y0) * (qx - x0)
        zc = z0 + (e1 * (z1 - z0) + e2 * (z2 - z0)) / area
        np.add.at(T, (i0 + ii, j0 + jj, np.searchsorted(Z, zc, "left")), 1)  # searchsorted left = how many z_k < zc
    above = T[:, :, ::-1].cumsum(axis=2)[:, :, ::-1]  # above[k] = crossings at positions >= k
    return (above[:, :, 1:] & 1).astype(bool), int((above[:, :, 0] & 1).sum())


def voxelise(tri, res, origin, spacing, band=np.inf, dtype=np.float64):
    """(phi [res] in dtype, odd columns): the whole rule.  The triangles are taken as given (the device is given float32)"""
    res = tuple(int(r) for r in res)
    inside, odd = parity(tri, res, origin, spacing)
    d = distance(tri, lattice_points(res, origin, spacing), dtype).reshape(res)
    d = np.minimum(d, dtype(band))
    return np.where(inside, -d, d), odd


# ------------------------------------------------------------------------------------------------------------------ meshes
def cube_mesh(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = np.array([[lo[0] if not i & 1 else hi[0], lo[1] if not i & 2 else hi[1], lo[2] if not i & 4 else hi[2]] for i in range(8)])
    quads = [(0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)]
    f = [(q[0], q[1], q[2]) for q in quads] + [(q[0], q[2], q[3]) for q in quads]
    return c[np.array(f)]


def cube_sdf(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)

    def f(x):
        q = np.abs(x - (lo + hi) / 2) - (hi - lo) / 2
        return np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(axis=1), 0)
    return f


def icosphere(subdivisions, radius, centre):
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius + np.asarray(centre, np.float64))[np.array(f)]


def sphere_sdf(radius, centre):
    return lambda x: np.linalg.norm(x - np.asarray(centre, np.float64), axis=1) - radius


def torus_mesh(R, r, centre, n_major, n_minor):
    """torus around the y axis through centre, vertices on the surface, n_major x n_minor quads split in two"""
    u = np.arange(n_major) * 2 * np.pi / n_major
    w = np.arange(n_minor) * 2 * np.pi / n_minor
    U, W = np.meshgrid(u, w, indexing="ij")
    P = np.stack([(R + r * np.cos(W)) * np.cos(U), r * np.sin(W), (R + r * np.cos(W)) * np.sin(U)], -1) + np.asarray(centre, np.float64)
    I, J = np.meshgrid(np.arange(n_major), np.arange(n_minor), indexing="ij")
    I1, J1 = (I + 1) % n_major, (J + 1) % n_minor
    a, b, c, d = P[I, J], P[I1, J], P[I1, J1], P[I, J1]
    return np.concatenate([np.stack([a, b, c], -2).reshape(-1, 3, 3), np.stack([a, c, d], -2).reshape(-1, 3, 3)])


def torus_sdf(R, r, centre):
    c = np.asarray(centre, np.float64)

    def f(x):
        d = x - c
        return np.hypot(np.hypot(d[:, 0], d[:, 2]) - R, d[:, 1]) - r
    return f


def octahedron_mesh(radius, centre):
    c = np.asarray(centre, np.float64)
    ax = [c + radius * np.eye(3)[k] * s for k in range(3) for s in (1, -1)]  # +x -x +y -y +z -z
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return np.array(ax)[np.array(f)]


def octahedron_sign(radius, centre):
    """a function with the sign of the octahedron's signed distance (zero exactly on the surface)"""
    return lambda x: np.abs(x - np.asarray(centre, np.float64)).sum(axis=1) - radius


# the lattice and the three meshes both test files use; the bounds are on |phi_mesh - closed form| (world units)
RES, ORIGIN, SPACING = (41, 37, 33), (0.013, 0.021, 0.017), 0.025
CUBE = ((0.3, 0.25, 0.2), (0.8, 0.6, 0.7))
SPHERE = (0.3, (0.5, 0.45, 0.4))
TORUS = (0.28, 0.1, (0.5, 0.45, 0.41))
ALIGNED_RES, ALIGNED_ORIGIN, ALIGNED_SPACING = (33, 33, 33), (0.0, 0.0, 0.0), 1.0 / 32
ALIGNED_CUBE = ((0.25, 0.25, 0.25), (0.75, 0.5, 0.75))
ALIGNED_OCTA = (0.25, (0.5, 0.5, 0.5))


def case(name, fp32=True):
    """(triangles, closed form, bound) of 'cube' | 'sphere' | 'torus'; fp32: the vertices rounded to what the device is given"""
    if name == "cube":
        tri, f, bound = cube_mesh(*CUBE), cube_sdf(*CUBE), 1e-12
    elif name == "sphere":
        tri, f = icosphere(3, *SPHERE), sphere_sdf(*SPHERE)
        e = np.linalg.norm(tri - np.roll(tri, 1, axis=1), axis=2).max()
        bound = SPHERE[0] - np.sqrt(SPHERE[0] ** 2 - e * e / 3)
    else:
        tri, f = torus_mesh(TORUS[0], TORUS[1], TORUS[2], 64, 32), torus_sdf(*TORUS)
        bound = (TORUS[0] + TORUS[1]) * (1 - np.cos(np.pi / 64)) + TORUS[1] * (1 - np.cos(np.pi / 32))
    return (tri.astype(np.float32) if fp32 else tri), f, bound
