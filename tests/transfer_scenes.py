"""Seeded scenes for the node-by-node and particle-by-particle tests of the transfer kernels (tests/test_gpu_transfer_edges.py on the
device, tests/test_transfer_model_cpu.py without one): the smallest shapes at which k_p2g, k_grid and k_g2p can go wrong.  Four
geometries come from tests/sort_scenes.py (runs, many_blocks, non_cubic_no_margin, ragged); two are new, on a 16 x 10 x 16 grid
without the boundary margin:

  faces        particles whose X - 0.5 is an integer exactly, and one fp32 ulp either side of it: on cell faces, on block faces and
               at block corners (a stencil over eight grid blocks); X = 0.5 (kept) and an ulp below (deleted); base + 2 == res (kept:
               the last rows of the dense view, and the half-empty top block of the axis of 10) and the next cell up (deleted);
               cells of 1, 2, 3 and 65 particles at the low faces
  lone_blocks  eight particles, each alone in a block none of whose 26 neighbours is active — its block owns all eight candidates of
               the grid pass and every seam is summed from one source — at block coordinate 0 and at the highest one of every axis

A scene is a dict: res, dx, clean_boundary, planes, friction, state (oracle.State, in upload order: group by group) and `edge`, a
function of (transfer_model.Scene, its p2g result) that asserts on the CPU what the scene exists for."""
import numpy as np

from oracle import oracle as orc
from tests import sort_scenes
from tests.common import make_state, mixed_state
from tests.sort_scenes import in_cells

DT = 1e-4
FRICTION = 0.4
MIXED_MATS = ("jelly", "linear", "elastic")
RES2, DX2 = (16, 10, 16), 1.0 / 16

# Planes (n, d): free space n.x + d > 0, the band of boundary nodes is -3 <= phi <= 0 in cells.  The scenes that reach node 0 get a
# plane through the low corner, along the face x = 0 and tilted a little, so that the band's edge crosses the rows of nodes at an angle
# and ends inside the grid: nodes of index 0 (on every axis) are boundary nodes.
# The others keep the floor of the parity tests.  Either way no touched node may lie within 1e-3 cells of phi = -3 or phi = 0, where
# fp32 and float64 could disagree about the band (asserted by band_is_clear): no node is excluded from the comparison.


def corner_plane(dx):
    n = np.array([1.0, 0.037, 0.019])
    n /= np.linalg.norm(n)
    return [tuple(n) + (-1.29 * dx,)]


FLOOR = [(0.0, 1.0, 0.0, -0.3)]


def _ulp(a, k):
    """fp32 a moved by k ulps (k in -1, 0, 1)"""
    a = np.asarray(a, np.float32)
    return a if k == 0 else np.nextafter(a, np.float32(np.inf if k > 0 else -np.inf))


def faces_geometry():
    rng = np.random.default_rng(211)
    res, dx = RES2, DX2
    X = []

    def inner(n):  # positions well inside the grid and inside their cells
        return np.stack([rng.integers(1, r - 3, n) + 0.5 + rng.uniform(0.2, 0.8, n) for r in res], 1)
    # (a) one axis on a face: cell faces (5), block faces (4, 8) and the first one (1); the axis of 10 has no 12
    for a in range(3):
        for face in (1, 4, 5, 8):
            for k in (-1, 0, 1):
                p = inner(6)
                p[:, a] = face + 0.5
                X.append((p, {a: k}))
    # (b) block corners: all three axes on a block face at once, every combination of -1 / 0 / +1 ulp
    for corner in ((4, 4, 4), (8, 4, 12), (12, 8, 4)):
        for kx in (-1, 0, 1):
            for ky in (-1, 0, 1):
                for kz in (-1, 0, 1):
                    X.append((np.array([corner], np.float64) + 0.5, {0: kx, 1: ky, 2: kz}))
    # (c) X = 0.5: kept; one ulp below: deleted
    for a in range(3):
        for k in (-1, 0, 1):
            p = inner(4)
            p[:, a] = 0.5
            X.append((p, {a: k}))
    # (d) the last base the grid holds (base + 2 == res), from its low face to an ulp below its high one; the next cell up is deleted
    for a in range(3):
        for off, k in ((-1.5, 0), (-1.5, 1), (-1.0, 0), (-0.5, -1), (-0.5, 0)):
            p = inner(4)
            p[:, a] = res[a] + off
            X.append((p, {a: k}))
    # all three axes in the last cell at once: the top corner of the dense view
    X.append((np.array([[res[0] - 1.2, res[1] - 1.3, res[2] - 0.9]]), {}))
    pts = []
    for p, moves in X:
        x = (p * dx).astype(np.float32)  # dx = 2^-4: exact
        for a, k in moves.items():
            x[:, a] = _ulp(x[:, a], k)
        pts.append(x)
    # (e) cells of 1, 2, 3 and 65 particles at the low faces
    pts.append(in_cells([(0, 1, 1), (0, 2, 1), (1, 0, 2), (0, 0, 0), (2, 1, 0)], [1, 2, 3, 65, 65], dx, rng))
    return dict(res=res, dx=dx, clean_boundary=False, x=np.concatenate(pts), planes=corner_plane(dx))


def faces_edge(M, raw):
    res = np.asarray(M.res)
    X32 = M.x.astype(np.float32) * np.float32(M.idx)          # live particles
    on = (X32 - np.float32(0.5)) == np.floor(X32 - np.float32(0.5))
    assert on.any(0).all() and (on.sum(1) == 3).sum() >= 3      # faces on every axis, and corners exactly on three
    Xn = np.nextafter(X32, np.float32(np.inf))
    below = (Xn - np.float32(0.5)) == np.floor(Xn - np.float32(0.5))  # one ulp below a face
    spans8 = ((M.base % 4) >= 2).all(1)
    assert np.any(spans8 & below.all(1)), "no stencil over eight grid blocks an ulp below a block corner"
    assert np.any(on & (M.base % 4 == 0)) and np.any(below & (M.base % 4 == 3))
    for a in range(3):
        assert np.any(X32[:, a] == np.float32(0.5)) and np.any(M.base[:, a] + 2 == res[a])
    assert (M.base + 2 == res).all(1).any()                     # the top corner node of the dense view
    n_dead = (~M.live).sum()
    assert n_dead == 3 * 4 + 3 * 4, n_dead                      # (c) an ulp below 0.5, (d) the cell above the last base: nothing else
    assert raw["touched"][0, 0, 0] and raw["touched"][res[0], res[1], res[2]]
    assert M.base[:, 1].max() == 8                              # the half-empty top block of the axis of 10
    cells, cnt = np.unique(M.base, axis=0, return_counts=True)
    for n in (1, 2, 3, 65):
        assert np.any((cnt == n) & (cells.min(1) == 0)), n


def lone_blocks_geometry():
    res, dx = RES2, DX2
    rng = np.random.default_rng(221)
    base = []
    for bx in (0, 3):
        for by in (0, 2):
            for bz in (0, 3):
                hi = [min(4 * b + 3, r - 2) for b, r in zip((bx, by, bz), res)]  # the block's last cell that is a base
                lo = [4 * bx, 4 * by, 4 * bz]
                # the block at the origin keeps cell (0, 0, 0), the last one the last base of the grid; the others a cell whose stencil
                # crosses into the next grid block where the block has one
                base.append(lo if (bx, by, bz) == (0, 0, 0) else hi)
    x = in_cells(base, [1] * len(base), dx, rng)
    return dict(res=res, dx=dx, clean_boundary=False, x=x, planes=corner_plane(dx))


def lone_blocks_edge(M, raw):
    blk = M.base >> 2
    assert M.live.all() and len(np.unique(blk, axis=0)) == len(blk)
    d = np.abs(blk[:, None, :] - blk[None, :, :]).max(2)
    assert np.all(d[~np.eye(len(blk), dtype=bool)] >= 2), "a neighbour block is active"
    top = (np.asarray(M.res) - 2) >> 2
    for a in range(3):
        assert blk[:, a].min() == 0 and blk[:, a].max() == top[a]
    assert (blk == 0).all(1).any() and (blk == top).all(1).any()
    assert (M.base + 2 == np.asarray(M.res)).all(1).any() and (M.base == 0).all(1).any()
    assert raw["count"].max() == 1                               # every node sum has one source
    assert np.any(((M.base % 4) >= 2).sum(1) >= 2)               # a stencil into the seams of its own tile


def _touches_the_low_corner(M, raw):
    t = raw["touched"]
    assert t[0].any() and t[:, 0].any() and t[:, :, 0].any(), "node index 0 is not reached on every axis"


def _from_sort_scene(name, planes):
    def geometry():
        s = sort_scenes.SCENES[name]()
        return dict(res=s["res"], dx=s["dx"], clean_boundary=s["clean_boundary"], x=s["x"], v=s["v"], planes=planes(s["dx"]),
                    sort_edge=s["edge"], sort_scene=s)
    return geometry


def _sort_edge_too(extra=None):
    def edge(M, raw):
        g = GEOMETRY_CACHE[M.name]
        g["sort_edge"](sort_scenes.model_of(g["sort_scene"]))
        if extra:
            extra(M, raw)
    return edge


def _high_faces(M, raw):
    _touches_the_low_corner(M, raw)
    res = np.asarray(M.res)
    for a in range(3):
        assert np.any(M.base[:, a] + 2 == res[a]), "the last row of the dense view is not reached on axis %d" % a


GEOMETRY = {
    "runs": (_from_sort_scene("runs", lambda dx: FLOOR), _sort_edge_too()),
    "ragged": (_from_sort_scene("ragged", lambda dx: FLOOR), _sort_edge_too()),
    "many_blocks": (_from_sort_scene("many_blocks", corner_plane), _sort_edge_too(_touches_the_low_corner)),
    "non_cubic_no_margin": (_from_sort_scene("non_cubic_no_margin", corner_plane), _sort_edge_too(_high_faces)),
    "faces": (faces_geometry, faces_edge),
    "lone_blocks": (lone_blocks_geometry, lone_blocks_edge),
}
SCENES = tuple(GEOMETRY)
CUBIC = ("runs", "ragged", "many_blocks")   # the ones the fp32 CPU oracle (a cubic grid) can express
MIXED_SCENES = ("many_blocks", "faces")
GEOMETRY_CACHE, _CACHE = {}, {}


def geometry(name):
    if name not in GEOMETRY_CACHE:
        GEOMETRY_CACHE[name] = GEOMETRY[name][0]()
    return GEOMETRY_CACHE[name]


def scene(name, mats="jelly", perturb_F=0.0):
    """the scene `name` with one material (a name) or the mixed assignment (mats = "mixed"), F = I + N(0, perturb_F); built once per
    combination and never changed"""
    k = (name, mats, perturb_F)
    if k in _CACHE:
        return _CACHE[k]
    g = geometry(name)
    x = g["x"]
    finite = np.isfinite(x).all(1)
    xs = np.where(finite[:, None], x, np.float32(0.5))  # (make_state centres its velocity field on the mean position)
    seed = 300 + 10 * SCENES.index(name)
    if mats == "mixed":
        assert finite.all()
        st = mixed_state(xs, list(MIXED_MATS), g["dx"], seed, perturb_F=perturb_F)
    else:
        st = make_state(xs, mats, g["dx"], seed=seed, perturb_F=perturb_F)
        st.x[~finite] = x[~finite]
        if "v" in g:  # the slots the sort scene marks dead through v
            bad = ~np.isfinite(g["v"])
            st.v[bad] = g["v"][bad]
    _CACHE[k] = dict(name=name, res=tuple(g["res"]), dx=g["dx"], clean_boundary=g["clean_boundary"], planes=g["planes"],
                     friction=FRICTION, state=st, edge=GEOMETRY[name][1], mats=mats)
    return _CACHE[k]


def model_scene(s):
    """transfer_model.Scene of a scene dict"""
    from tests import transfer_model as tmod
    M = tmod.Scene(s["state"], s["res"], s["dx"], DT, s["clean_boundary"], planes=s["planes"], friction=s["friction"])
    M.name = s["name"]
    return M


def band_is_clear(M, raw):
    from tests import transfer_model as tmod
    margin = tmod.band_margin(M, raw["touched"])
    assert margin > 1e-3, "a touched node lies %.2e cells from an edge of the boundary band" % margin


def oracle_config(s, **kw):
    assert len(set(s["res"])) == 1
    return orc.make_config(s["res"][0], s["dx"], DT, planes=s["planes"], friction=s["friction"], clean_boundary=s["clean_boundary"], **kw)


_MODELLED = {}


def modelled(name, mats="jelly", perturb_F=0.0):
    """(scene, transfer_model.Scene, the model's substep) of a combination, computed once and never changed.  The substep dict also
    holds "g2p_own": G2P from the fp32 copy "grid32" of the model's own grid (what the G2P-alone stage uploads), and "kept": which of
    the live particles the device keeps after G2P (the sort key of the new position), with "kept_margin": the smallest distance of a new
    position from a threshold of that decision, in units of the bound the device's position is held to."""
    from tests import transfer_model as tmod
    from tests.common import sort_key
    k = (name, mats, perturb_F)
    if k not in _MODELLED:
        s = scene(name, mats, perturb_F)
        M = model_scene(s)
        out = tmod.substep(M)
        out["grid32"] = out["grid"]["grid"].astype(np.float32)
        out["g2p_own"] = tmod.g2p(M, out["grid32"].astype(np.float64))
        lo = 7.0 if s["clean_boundary"] else 0.5
        hi = np.asarray(s["res"], np.float64) - lo
        for o in (out, out["g2p_own"]):
            o["kept"] = sort_key(o["x"].astype(np.float32), s["dx"], s["res"], clean_boundary=s["clean_boundary"]) >= 0
            X = o["x"] * M.idx
            o["kept_margin"] = float((np.minimum(np.abs(X - lo), np.abs(X - hi)) / (o["x_bound"] * M.idx)).min())
        _MODELLED[k] = (s, M, out)
    return _MODELLED[k]
