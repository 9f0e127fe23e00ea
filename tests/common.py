"""Shared seeded scene builders for oracle and GPU parity tests."""
import os

import numpy as np

from oracle import oracle as orc


# per-material Config keys used by the seeded scenes (empty = the reference's defaults, src/particles.cpp initialize())
MAT_KW = {}


def lattice_cube(res, lo_cell, hi_cell, dx, jitter=0.0, seed=0):
    """8 particles per cell at the +-0.25*dx lattice of the reference's benchmark generator
    (src/mpm.cpp:164-180), optionally jittered."""
    rng = np.random.default_rng(seed)
    ii, jj, kk = np.meshgrid(np.arange(lo_cell, hi_cell), np.arange(lo_cell, hi_cell),
                             np.arange(lo_cell, hi_cell), indexing="ij")
    cells = np.stack([ii, jj, kk], -1).reshape(-1, 3).astype(np.float64)
    pts = []
    for i in range(8):
        sign = np.array([1.0, 1.0, 1.0])
        if i % 2 == 0:
            sign[0] = -1
        if i // 2 % 2 == 0:
            sign[1] = -1
        if i // 4 % 2 == 0:
            sign[2] = -1
        # Region index get_pos() is the cell centre (ipos + 0.5)
        pts.append((cells + 0.5) * dx + 0.25 * dx * sign)
    x = np.stack(pts, 1).reshape(-1, 3)
    if jitter:
        x = x + rng.uniform(-jitter, jitter, x.shape) * dx
    return x.astype(np.float32)


def make_state(x, type_name, dx, density=400.0, ppc=8, seed=1, vel_scale=1.0, perturb_F=0.05, **mat_kw):
    """random-but-plausible v, B, F around a rotating/shearing field so every term is exercised."""
    rng = np.random.default_rng(seed)
    n = len(x)
    vol = dx ** 3 / ppc
    gp, t = orc.group_params(type_name, vol * density, vol, **mat_kw)
    c = x.mean(0)
    r = (x - c).astype(np.float64)
    omega = np.array([0.3, 1.0, -0.5]) * vel_scale
    v = np.cross(omega, r) * 4.0 + rng.normal(0, 0.05 * vel_scale, (n, 3))
    B = rng.normal(0, 0.02 * vel_scale, (n, 9))
    F = np.tile(np.eye(3).reshape(1, 9), (n, 1)) + rng.normal(0, perturb_F, (n, 9))
    aux = np.full(n, orc.initial_aux(type_name, **mat_kw), np.float32)
    if type_name == "snow":
        aux = (1.0 + rng.normal(0, 0.02, n)).astype(np.float32)
    if type_name == "water":
        aux = (1.0 + rng.normal(0, 0.01, n)).astype(np.float32)
    if type_name == "sand":
        aux = np.abs(rng.normal(0, 0.01, n)).astype(np.float32)
    return orc.State(x, v, B, F, aux, np.zeros(n, np.int32), gp[None, :], np.array([t], np.int32))


def mixed_state(x, mats, dx, seed, **kw):
    """the particles at x dealt out to the materials `mats` by a seeded permutation (equal shares to within one particle), so that
    materials mix inside every cell; one group per material, each seeded like make_state's.  The particles are stored group by
    group: the order in which a simulation that is given the groups in turn numbers them."""
    which = np.random.default_rng(seed).permutation(len(x)) % len(mats)
    parts = [make_state(x[which == g], m, dx, seed=seed + 1 + g, **kw) for g, m in enumerate(mats)]
    return orc.State(*(np.concatenate([getattr(p, f) for p in parts]) for f in ("x", "v", "B", "F", "aux")),
                     np.concatenate([np.full(p.n, g, np.int32) for g, p in enumerate(parts)]),
                     np.stack([p.gparams[0] for p in parts]), np.array([p.gtype[0] for p in parts], np.int32))


def sort_key(x, dx, res=None, v=None, ids=None, clean_boundary=False):
    """the key the device sorts by: Morton(block) << 6 | cell in the block (blocks of 4^3 cells; the cell of a particle is the base
    node of its quadratic stencil).  With `res` (three nodes counts) the slots the device deletes get -1, as particle_key of
    csrc/mpm_common.h decides it in fp32: a non-finite x or v, an id < 0, the 7-cell margin when clean_boundary, X < 0.5, or a
    stencil that leaves the grid (base + 2 > res, per axis)."""
    idx = np.float32(1.0) / np.float32(dx)  # (Params::idx)
    with np.errstate(invalid="ignore", over="ignore"):
        X = x.astype(np.float32) * idx
        if res is None:
            alive = np.ones(len(X), bool)
        else:
            r = np.asarray(res, np.float32)
            alive = np.isfinite(x).all(1)
            if v is not None:
                alive &= np.isfinite(v).all(1)
            if ids is not None:
                alive &= np.asarray(ids) >= 0
            if clean_boundary:
                alive &= ~((X.min(1) < np.float32(7.0)) | ((X - r).max(1) > np.float32(-7.0)))
            alive &= (X >= np.float32(0.5)).all(1)
        base = np.floor(np.where(alive[:, None], X, np.float32(0.5)) - np.float32(0.5)).astype(np.int64)
    if res is not None:
        alive &= (base + 2 <= np.asarray(res, np.int64)).all(1)
        base[~alive] = 0

    def spread(v):
        r = np.zeros_like(v)
        for b in range(10):
            r |= ((v >> b) & 1) << (3 * b)
        return r
    blk = base >> 2
    key = ((spread(blk[:, 0]) << 2 | spread(blk[:, 1]) << 1 | spread(blk[:, 2])) << 6) | ((base[:, 0] & 3) << 4) | \
        ((base[:, 1] & 3) << 2) | (base[:, 2] & 3)
    return np.where(alive, key, -1)


def fewest_kinds_in_a_window(x, kind, dx, window=64):
    """over every run of `window` consecutive particles in key order (a wave of a transfer kernel): the smallest number of
    different values of kind[] in it"""
    k = kind[np.argsort(sort_key(x, dx), kind="stable")]
    present = np.zeros(len(k) - window + 1, np.int64)
    for g in np.unique(kind):
        c = np.concatenate([[0], np.cumsum(k == g)])
        present += (c[window:] - c[:-window]) > 0
    return int(present.min())


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_PART_BYTES = 900_000  # raw bytes per file of a fixture: compressed, every committed file stays under 1 MiB


def save_golden(name, **arrays):
    """tests/golden/<name>.npz, split into <name>.npz, <name>.2.npz, ... of at most GOLDEN_PART_BYTES raw bytes each"""
    parts, size = [{}], 0
    for k, v in arrays.items():
        v = np.asarray(v)
        if parts[-1] and size + v.nbytes > GOLDEN_PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += v.nbytes
    for i, part in enumerate(parts):
        np.savez_compressed(os.path.join(GOLDEN, name + (".npz" if i == 0 else ".%d.npz" % (i + 1))), **part)


def load_golden(name):
    """{key: array} of a fixture written by save_golden (all its parts)"""
    out, i = dict(np.load(os.path.join(GOLDEN, name + ".npz"))), 2
    while os.path.exists(os.path.join(GOLDEN, "%s.%d.npz" % (name, i))):
        out.update(np.load(os.path.join(GOLDEN, "%s.%d.npz" % (name, i))))
        i += 1
    return out
