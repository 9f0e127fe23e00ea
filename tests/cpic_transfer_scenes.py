"""Seeded scenes for the per-value tests of the colour-aware transfer kernels k_p2g_rigid / k_g2p_rigid (tests/test_gpu_cpic_transfer_edges.py
on the device, tests/test_cpic_transfer_model_cpu.py without one): the smallest shapes at which the paths of csrc/k_rigid_transfer.h that
the recorded whole-substep runs of tests/test_gpu_cpic.py never reach are taken.

  overflow     a plate through one 4^3 block whose cells beside the plate hold 35 particles each on average: 1120, more than P2GR_LIST = 1024,
               boundary particles (particles with a node on the other side of a body), so the second pass of k_p2g_rigid walks the
               block cell by cell; the blocks around it hold 1 .. 1024
  two_bodies   two plates one cell apart, different velocities and angular velocities, friction0 != friction1 on both: the stencils
               between them hold nodes of the other colour of BOTH bodies (the ImpulseAcc hand-over), particles sit below, between and
               above; the lower plate is moved 0.2 cells up after the particles took their colours, so some of them lie inside the
               penalty window with two bodies in the stencil (the LAST one met receives the penalty's impulse)
  edges        a grid that is not cubic and whose dx is no power of two; one plate reaches into block coordinate 0 of the x axis, another
               into the last block of the z axis
  quiet_shell  the blocks one further in +y than the plate's own are flagged (the reference flags the page of a boundary particle AND its
               neighbours in the positive directions) but hold no coloured node: a flagged block, sparsely filled, none of whose
               particles has a node of the other colour, next to blocks without the flag
  window       the plate is moved 0.45 cells along its normal after the particles took their colours: the particles it swept over have
               negative boundary distances on both sides of both edges of the penalty window (-0.3 dx, -0.05 dx); the plate is smaller
               than the block of particles, so along its rim the fit fails (near == 0) for particles that do have nodes of the other
               colour

THE GRIDS.  A boundary particle of a body is only created 7 cells or more from every wall (add_body of csrc/rigid_setup.h, as
src/mpm_rigid_body.cpp does), so no body can ever have one on a grid with an axis of fewer than 15 cells: `edges` uses 24 x 16 x 20 with
dx = 1/20, the smallest non-cubic shape on which a plate exists at all, and its bodies are MOVED to the ends of the grid after their
creation (`moves`: a velocity for one advect_rigid_bodies(), then the scene's velocities are set).  The moved boundary particles respect
sample_base's [0.5, res - 1.5) rule.

A scene is a dict: res, dx, state (oracle.State in upload order), mat_names (per group), bodies (configs of add_rigid_body plus `velocity`,
`angular_velocity`, `move`), `presweep` (a move of body 1 BETWEEN a first gather_cdf and the stages under test) and `edge`, a function of
(cpic_transfer_model.Cpic, its p2g result, its g2p result) that asserts on the CPU what the scene exists for.  The colour field is an INPUT
of these tests: it is downloaded from whoever ran rasterize_rigid_boundary + gather_cdf (the device, or the compiled reference), so the
run-time assertions of `edge` hold for that field.  The builders and the recorder are in tests/cpic_transfer_runs.py."""
import numpy as np

from tests.common import make_state, mixed_state

DT = 1e-4
GRAVITY = (0.0, -10.0, 0.0)
PENALTY, PUSHING_FORCE = 1e3, 2e4
MIXED_MATS = ("jelly", "linear", "elastic", "sand")
SCENES = ("overflow", "two_bodies", "edges", "quiet_shell", "window")
P2GR_LIST = 1024  # csrc/k_rigid_transfer.h


def plate(hx, hz):
    """a rectangle in the x-z plane (world units), two triangles"""
    return np.array([[[-hx, 0, -hz], [hx, 0, -hz], [hx, 0, hz]], [[-hx, 0, -hz], [hx, 0, hz], [-hx, 0, hz]]], np.float32)


def _box(rng, lo, hi, per_cell):
    """uniformly random positions (cells) in the box [lo, hi), per_cell of them per unit cell"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return rng.uniform(lo, hi, (int(round(np.prod(hi - lo) * per_cell)), 3))


def _body(dx, centre, half, rot, density, f0, f1, vel, omega, move=None):
    return dict(mesh=plate(half[0] * dx, half[1] * dx), codimensional=True, density=density, friction0=f0, friction1=f1,
                initial_position=tuple(float(c) * dx for c in centre), initial_rotation=rot, velocity=vel, angular_velocity=omega,
                move=None if move is None else tuple(float(m) * dx for m in move))


def overflow_geometry():
    rng = np.random.default_rng(401)
    res, dx = (24, 24, 24), 1.0 / 24
    # block (2, 2, 2) = base cells 8 .. 11; the plate lies between the node rows y = 9 and y = 10: the stencils with y base 8 and 9 straddle it
    X = [_box(rng, (8.5, 8.5, 8.5), (12.5, 10.5, 12.5), 35), _box(rng, (8.5, 10.5, 8.5), (12.5, 12.5, 12.5), 4),
         _box(rng, (7.5, 7.5, 7.5), (13.5, 13.5, 8.5), 3), _box(rng, (7.5, 7.5, 12.5), (13.5, 13.5, 13.5), 3),
         _box(rng, (7.5, 7.5, 8.5), (8.5, 13.5, 12.5), 3), _box(rng, (12.5, 7.5, 8.5), (13.5, 13.5, 12.5), 3)]
    # (a heavy plate: the few impulses a broken fallback walk would lose then change its velocity by less than the tolerances of the
    # whole-substep parity tests notice — tests/test_cpic_transfer_model_cpu.py shows both)
    bodies = [_body(dx, (12.02, 9.5, 11.97), (4.8, 4.8), (1.5, 0.0, 1.0), 1600.0, 0.3, 0.1, (0.2, -0.4, 0.1), (0.5, 1.0, -0.7))]
    return dict(res=res, dx=dx, X=np.concatenate(X), bodies=bodies)


def overflow_edge(C, raw, out):
    n = raw["boundary_count"]
    assert n.max() > P2GR_LIST, "no block lists more than %d boundary particles: %d" % (P2GR_LIST, n.max())
    full = np.argwhere(n > P2GR_LIST)
    near = np.abs(np.argwhere((n >= 1) & (n <= P2GR_LIST))[:, None, :] - full[None, :, :]).max(2).min(1)
    assert (near == 1).any(), "no neighbouring flagged block with 1 .. %d boundary particles" % P2GR_LIST
    assert len(C.bodies) == 2 and np.abs(raw["impulse"][1, :3]).min() > 0


def two_bodies_geometry():
    rng = np.random.default_rng(402)
    res, dx = (24, 24, 24), 1.0 / 24
    X = [_box(rng, (7.5, 7.6, 7.5), (13.5, 12.4, 13.5), 7), _box(rng, (7.8, 9.3, 7.8), (13.2, 9.62, 13.2), 30)]
    bodies = [_body(dx, (12.03, 9.35, 11.96), (4.7, 4.7), (1.0, 0.0, 1.5), 2.0, 0.3, 0.05, (0.2, -0.4, 0.1), (0.5, 1.0, -0.7)),
              _body(dx, (11.98, 10.45, 12.05), (4.7, 4.7), (-1.2, 0.0, 0.8), 3.0, 0.1, 0.45, (-0.3, 0.5, 0.2), (-0.8, 0.4, 1.1))]
    # the lower plate moves up 0.2 cells after the particles took their colours (it stays between the node rows 9 and 10): the particles
    # it swept over lie inside the penalty window of a body whose nodes come FIRST in their stencils, the upper body's come last
    return dict(res=res, dx=dx, X=np.concatenate(X), bodies=bodies, presweep=(0.0, 0.2, 0.0))


def two_bodies_edge(C, raw, out):
    pen = out["penalised"] & (out["first_body"] > 0) & (out["first_body"] != out["last_body"])
    assert pen.sum() >= 16, "only %d particles inside the penalty window whose first and last body differ" % pen.sum()
    assert (out["impulse_n"][1:] > 0).all(), "a body receives no penalty impulse: %s" % out["impulse_n"]
    both = (raw["tap_body_count"][:, 1] > 0) & (raw["tap_body_count"][:, 2] > 0)
    assert both.sum() >= 64, "only %d particles whose stencil holds nodes of the other colour of both bodies" % both.sum()
    assert (raw["block_bodies"] >= 2).any(), "no block in which both bodies receive impulses"
    for b in (1, 2):  # particles on both sides of each body: both friction coefficients are used
        assert C.bodies[b]["friction"][0] != C.bodies[b]["friction"][1]
        side = (C.pstate >> (2 * b)) & 1
        used = raw["tap_body_count"][:, b] > 0
        assert (side[used] == 0).any() and (side[used] == 1).any(), "body %d is met from one side only" % b


def edges_geometry():
    rng = np.random.default_rng(403)
    res, dx = (24, 16, 20), 1.0 / 20
    X = [_box(rng, (0.6, 6.2, 7.0), (7.4, 10.3, 13.0), 5), _box(rng, (9.0, 6.2, 12.5), (15.0, 10.3, 18.4), 5)]
    bodies = [_body(dx, (12.03, 8.02, 10.04), (2.4, 2.4), (2.0, 0.0, 1.0), 2.0, 0.3, 0.1, (0.2, -0.4, 0.1), (0.5, 1.0, -0.7), move=(-8.0, 0.3, 0.0)),
              _body(dx, (12.01, 7.97, 9.98), (2.4, 2.4), (-1.0, 0.0, 2.0), 3.0, 0.05, 0.4, (-0.3, 0.5, 0.2), (-0.8, 0.4, 1.1), move=(0.0, 0.2, 5.6))]
    return dict(res=res, dx=dx, X=np.concatenate(X), bodies=bodies)


def edges_edge(C, raw, out):
    """Coloured nodes without a body id: the field under test never holds one — the rasterisation sets a node's tag bits and its
    (distance, body id) word together, on the device (k_cdf_rasterize: atomicMin + atomicOr in one thread) as in the reference (under
    the node's lock) — so the `rid < 0` branches of the kernels cannot be reached from a real field; asserted here, and modelled and
    seeded with a synthetic field in tests/test_cpic_transfer_model_cpu.py."""
    M = C.M
    assert len(set(M.res)) == 3 and 2.0 ** round(np.log2(M.idx)) != M.idx  # not cubic, dx no power of two
    blk = np.argwhere(raw["boundary_count"] > 0)
    top = (np.asarray(M.res) - 2) >> 2
    assert (blk[:, 0] == 0).any(), "no flagged block with boundary particles at block coordinate 0 of x"
    assert (blk[:, 2] == top[2]).any(), "no flagged block with boundary particles in the last block of z"
    tags = C.words & 0xFFFFFF
    assert (tags != 0).sum() > 100 and not np.any((tags != 0) & (C.words >> 24 == 0))


def quiet_shell_geometry():
    rng = np.random.default_rng(404)
    res, dx = (24, 24, 24), 1.0 / 24
    # the plate's own blocks are y block 2 (nodes 8 .. 11); y block 3 (base cells 12 .. 15) is flagged as their +y neighbour, y block 4
    # is not.  One particle in every other cell of x block 2, z block 2, y cells 13 .. 17: the stencils of base 13 stay clear of the
    # coloured nodes (y <= 11), those of base 14, 15 reach into the unflagged block's tile, those of base 16, 17 belong to it
    cells = np.array([(i, j, k) for i in range(8, 12) for j in range(13, 18) for k in range(8, 12) if (i + j + k) % 2 == 0], np.float64)
    X = [cells + 0.5 + rng.uniform(0.1, 0.9, cells.shape), _box(rng, (8.5, 8.0, 8.5), (11.5, 11.0, 11.5), 4)]
    bodies = [_body(dx, (10.03, 9.5, 9.96), (2.9, 2.9), (1.5, 0.0, 1.0), 2.0, 0.3, 0.1, (0.2, -0.4, 0.1), (0.5, 1.0, -0.7))]
    return dict(res=res, dx=dx, X=np.concatenate(X), bodies=bodies)


def quiet_shell_edge(C, raw, out):
    M = C.M
    blk = (2, 3, 2)
    assert C.flagged_block(np.array([blk]))[0] and not C.flagged_block(np.array([(2, 4, 2)]))[0]
    inb = ((M.base >> 2) == np.array(blk)).all(1)
    assert inb.sum() >= 16 and not raw["other"][inb].any(), "a particle of the quiet block has a node of the other colour"
    assert len(np.unique(M.base[inb], axis=0)) < 64, "the quiet block has no empty cell"
    assert (((M.base >> 2) == np.array((2, 4, 2))).all(1)).sum() >= 8
    assert raw["other"].any()  # (the scene has boundary particles elsewhere: the colour-aware kernels do run)


QUIET_BLOCK = (2, 3, 2)


def quiet_tile(M):
    """index arrays of the nodes the particles of quiet_shell's quiet flagged block reach: its own nodes and the halo nodes it shares with
    its neighbours, the unflagged block above among them"""
    mine = ((M.base >> 2) == np.array(QUIET_BLOCK)).all(1)
    reach = np.zeros(tuple(r + 1 for r in M.res), bool)
    for tap, node, ww, d, dw in M.taps():
        reach[tuple(a[mine] for a in node)] = True
    return tuple(np.argwhere(reach).T)


def window_geometry():
    rng = np.random.default_rng(405)
    res, dx = (24, 24, 24), 1.0 / 24
    X = [_box(rng, (7.6, 8.6, 7.6), (15.4, 11.4, 15.4), 3), _box(rng, (8.5, 9.7, 8.5), (14.5, 10.4, 14.5), 25)]
    bodies = [_body(dx, (11.53, 9.8, 11.46), (2.6, 2.6), (1.0, 0.0, 0.7), 2.0, 0.3, 0.1, (0.2, -0.4, 0.1), (0.5, 1.0, -0.7))]
    return dict(res=res, dx=dx, X=np.concatenate(X), bodies=bodies, presweep=(0.0, 0.45, 0.0))


WINDOW_ULPS = 8.0  # distance of every boundary distance from an edge of the window, in fp32 ulps of the edge: the kernel compares fp32 values


def window_edge(C, raw, out):
    M = C.M
    lo, hi = np.float32(-M.dx) * np.float32(0.3), np.float32(-0.05) * np.float32(M.dx)  # as k_g2p_rigid forms them
    d = C.dist[C.near]
    margin = np.minimum(np.abs(d - lo) / np.spacing(np.abs(lo)), np.abs(d - hi) / np.spacing(np.abs(hi))).min()
    assert margin >= WINDOW_ULPS, "a boundary distance lies %.1f ulps from an edge of the penalty window" % margin
    classes = dict(below=d < lo, inside=(d > lo) & (d < hi), above=(d > hi) & (d < 0))
    for k, m in classes.items():
        assert m.sum() >= 32, "%s the window: %d particles" % (k, m.sum())
    assert out["penalised"].sum() == classes["inside"].sum()
    far = ~C.near & raw["other"]
    assert far.sum() >= 32, "near == 0 with a node of the other colour: %d particles" % far.sum()


# (scene, materials, perturbation of F) of the CPU comparison with the reference; FIXTURE_CASES are recorded in
# tests/golden/ref_cpic_transfer.npz (generator: tests/golden/make_golden.py cpic_transfer), all of them run live where the library is
FIXTURE_CASES = [(n, "jelly", 0.02) for n in SCENES] + [("quiet_shell", "sand", 0.0), ("quiet_shell", "mixed", 0.02), ("two_bodies", "mixed", 0.02),
                                                       ("window", "sand", 0.02)]
LIVE_CASES = FIXTURE_CASES + [(n, "jelly", 0.0) for n in SCENES] + [(n, m, 0.02) for n in ("overflow", "two_bodies", "window") for m in ("sand", "mixed")]


def case_id(name, mats, perturb):
    return "%s-%s-%s" % (name, mats, "F=I" if perturb == 0 else "perturbed")


GEOMETRY = {"overflow": (overflow_geometry, overflow_edge), "two_bodies": (two_bodies_geometry, two_bodies_edge),
            "edges": (edges_geometry, edges_edge), "quiet_shell": (quiet_shell_geometry, quiet_shell_edge),
            "window": (window_geometry, window_edge)}
_CACHE = {}


def scene(name, mats="jelly", perturb_F=0.0):
    """the scene `name` with one material (a name) or the mixed assignment (mats = "mixed"); built once per combination, never changed"""
    k = (name, mats, perturb_F)
    if k not in _CACHE:
        g = GEOMETRY[name][0]()
        x = (g["X"] * g["dx"]).astype(np.float32)
        seed = 500 + 10 * SCENES.index(name)
        if mats == "mixed":
            st, names = mixed_state(x, list(MIXED_MATS), g["dx"], seed, perturb_F=perturb_F, vel_scale=0.3), MIXED_MATS
        else:
            st, names = make_state(x, mats, g["dx"], seed=seed, perturb_F=perturb_F, vel_scale=0.3), (mats,)
        _CACHE[k] = dict(name=name, res=g["res"], dx=g["dx"], state=st, mat_names=names, mats=mats, perturb=perturb_F, bodies=g["bodies"],
                         presweep=g.get("presweep"), edge=GEOMETRY[name][1])
    return _CACHE[k]
