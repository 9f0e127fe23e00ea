"""The expression scenes the region tests share (tests/test_region_model_cpu.py, tests/test_gpu_region.py, tests/test_gpu_region2d.py):
each as the Region the Python layer compiles and, for the shape scenes, as a float64 function written directly from the definitions
(closed-form spheres, boxes, planes; phi in grid units) that returns phi and every leaf value and band-edge difference.
Grid: dx = 1/64."""
import numpy as np

DX = 1.0 / 64


# ---- float64, from the definitions (world positions in, grid units out)
def sphere(c, r):
    c = np.asarray(c, np.float64)
    return lambda x: (np.linalg.norm(x - c[None, :x.shape[1]], axis=1) - r) / DX


def box(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)

    def f(x):
        l, h = lo[None, :x.shape[1]], hi[None, :x.shape[1]]
        ins = np.all((l <= x) & (x <= h), axis=1)
        return np.where(ins, -np.minimum(x - l, h - x).min(axis=1), np.linalg.norm(x - np.clip(x, l, h), axis=1)) / DX
    return f


def plane(n, d):
    n = np.asarray(n, np.float64)
    return lambda x: (x @ n[:x.shape[1]] + d) / DX


def placed(f, R, s, t, p):
    """world = t + s R (local - p)"""
    R, t, p = np.asarray(R, np.float64), np.asarray(t, np.float64), np.asarray(p, np.float64)
    return lambda x: s * f((x - t[None, :]) @ R / s + p[None, :])  # (rows: (R^T d)^T = d^T R)


def rot_z(deg):
    a = np.radians(deg)
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def evaluate(tree, x):
    """tree: ("leaf", f) | ("band", f, lo, hi) | ("or", a, b) | ("and", a, b) | ("not", a) -> (phi, [leaf values and band-edge
    differences])"""
    if tree[0] == "leaf":
        v = tree[1](x)
        return v, [v]
    if tree[0] == "band":
        v = tree[1](x)
        return np.maximum(tree[2] - v, v - tree[3]), [v, tree[2] - v, v - tree[3]]
    if tree[0] == "not":
        v, l = evaluate(tree[1], x)
        return -v, l
    a, la = evaluate(tree[1], x)
    b, lb = evaluate(tree[2], x)
    return (np.minimum(a, b) if tree[0] == "or" else np.maximum(a, b)), la + lb


R12, R8, R4 = 12 * DX, 8 * DX, 4 * DX
BOX_LO, BOX_HI = (-6 * DX, -3 * DX, -4 * DX), (6 * DX, 3 * DX, 4 * DX)  # 12 x 6 x 8 dx about the origin


def shape_scenes(tm, dim):
    """name -> (Region, float64 tree)"""
    LS, Region = tm.mpm.LevelSet, tm.mpm.Region
    if dim == 3:
        c = (0.5, 0.5, 0.5)
        ball = lambda r, at=c: Region(LS().add_sphere(at, r))
        cut = Region(LS().add_plane((0, 1, 0), d=-(0.5 + 2 * DX)))
        b0 = Region(LS().add_cuboid(BOX_LO, BOX_HI))
        ground = Region(LS().add_plane((0, 1, 0), d=-0.3))
        crate = Region(LS().add_cuboid((0.25, 0.2, 0.3), (0.75, 0.6, 0.7)))
        z = (0.0, 0.0, 0.0)
        return {
            "clipped_shell": ((ball(R12) - ball(R8)) & cut,
                              ("and", ("and", ("leaf", sphere(c, R12)), ("not", ("leaf", sphere(c, R8)))), ("leaf", plane((0, 1, 0), -(0.5 + 2 * DX))))),
            "placed_boxes": (b0.placed(rotate=((0, 0, 1), 30.0), translate=(0.36, 0.5, 0.5)) | b0.placed(scale=1.5, translate=(0.66, 0.55, 0.47)),
                             ("or", ("leaf", placed(box(BOX_LO, BOX_HI), rot_z(30.0), 1.0, (0.36, 0.5, 0.5), z)),
                              ("leaf", placed(box(BOX_LO, BOX_HI), np.eye(3), 1.5, (0.66, 0.55, 0.47), z)))),
            "ground_band": (ground.band(0.0, 3.0) & crate,
                            ("and", ("band", plane((0, 1, 0), -0.3), 0.0, 3.0), ("leaf", box((0.25, 0.2, 0.3), (0.75, 0.6, 0.7))))),
            "complement": (~ball(R4) & Region(LS().add_cuboid((0.4, 0.4, 0.4), (0.6, 0.6, 0.6))),
                           ("and", ("not", ("leaf", sphere(c, R4))), ("leaf", box((0.4, 0.4, 0.4), (0.6, 0.6, 0.6))))),
        }
    c = (0.5, 0.5)
    disc = lambda r: Region(LS().add_sphere(c + (0.0,), r))
    cut = Region(LS().add_plane((0, 1, 0), d=-(0.5 + 2 * DX)))
    b0 = Region(LS().add_cuboid(BOX_LO, BOX_HI))
    z = (0.0, 0.0)
    return {
        "annulus": ((disc(R12) - disc(R8)) & cut,
                    ("and", ("and", ("leaf", sphere(c, R12)), ("not", ("leaf", sphere(c, R8)))), ("leaf", plane((0, 1), -(0.5 + 2 * DX))))),
        "placed_boxes": (b0.placed(rotate=30.0, translate=(0.36, 0.5)) | b0.placed(scale=1.5, translate=(0.66, 0.55)),
                         ("or", ("leaf", placed(box(BOX_LO[:2], BOX_HI[:2]), rot_z(30.0)[:2, :2], 1.0, (0.36, 0.5), z)),
                          ("leaf", placed(box(BOX_LO[:2], BOX_HI[:2]), np.eye(2), 1.5, (0.66, 0.55), z)))),
    }


def lattice_origin(centre, dim):
    """60 samples per axis at spacing dx / 2, off the grid: as the seeding tests' sampled_sphere builds it"""
    return tuple(np.float32(c - 14.3 * DX + 0.0137 * DX) for c in centre[:dim])


def sampled_ball(tm, centre, r, dim=3):
    c = np.asarray(centre[:dim], np.float64)
    f = lambda x: np.linalg.norm(x - c, axis=1) - r
    if dim == 3:
        return tm.mpm.SampledLevelSet.from_function(f, (60,) * 3, lattice_origin(centre, 3), DX / 2)
    return tm.SampledLevelSet2D.from_function(f, (60,) * 2, lattice_origin(centre, 2), DX / 2)


def sampled_scenes(tm, dim=3):
    """(a) sampled r = 12 dx ball minus sampled r = 8 dx ball on one lattice; (b) the r = 8 dx lattice as two leaves, one plain and
    one placed at (0.70, 0.56, 0.47) about the centre, rotated 30 degrees about z, scale 0.75"""
    Region = tm.mpm.Region
    c = (0.5, 0.5, 0.5)
    s12, s8 = sampled_ball(tm, c, R12, dim), sampled_ball(tm, c, R8, dim)
    rot = ((0, 0, 1), 30.0) if dim == 3 else 30.0
    return {
        "a": Region(s12) - Region(s8),
        "b": Region(s8) | Region(s8).placed(rotate=rot, scale=0.75, translate=(0.70, 0.56, 0.47)[:dim], about=c[:dim]),
    }
