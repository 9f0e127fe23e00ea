"""The float64 transfer model (tests/transfer_model.py) and its scenes (tests/transfer_scenes.py), checked without a GPU:
(a) the model against oracle/np_mpm.py — two independent statements of the same maths — and against the conservation identities,
    and every scene's edge();
(b) the bound is not too tight: the fp32 C++ oracle, an independent fp32 implementation with another order of summation, stays
    inside the per-node and per-particle bound on every scene it can express (the cubic grids);
(c) the bound is not too loose: seeded mutants of the float64 result — the faults a subtly wrong kernel would leave — are each
    flagged by the per-node / per-particle check, and the first of them passes the global rel-L2 of the parity tests.
The device is held to the same bounds in tests/test_gpu_transfer_edges.py."""
import numpy as np
import pytest

from oracle import np_mpm
from tests import transfer_model as tmod
from tests import transfer_scenes as ts
from tests.common import rel_l2

model_of = ts.modelled


CASES = [(n, "jelly", 0.0) for n in ts.SCENES] + [(n, "jelly", 0.02) for n in ts.SCENES] + \
        [(n, "mixed", p) for n in ts.MIXED_SCENES for p in (0.0, 0.02)]
IDS = ["%s-%s-%s" % (n, m, "F=I" if p == 0 else "perturbed") for n, m, p in CASES]


@pytest.mark.parametrize("name", ts.SCENES)
def test_scene_reaches_its_edge(name):
    s, M, out = model_of(name)
    s["edge"](M, out["p2g"])
    ts.band_is_clear(M, out["p2g"])
    band = out["grid"]["band"]
    assert band.any(), "no boundary node carries mass"
    if s["planes"] is not ts.FLOOR:
        assert band[0].any() and band[:, 0].any() and band[:, :, 0].any(), "no boundary node of index 0"
    assert 0 < M.n <= 8000
    if name == "faces":
        assert not out["kept"].all() and not out["g2p_own"]["kept"].all()  # particles on the outermost faces leave


@pytest.mark.parametrize("name,mats,perturb", CASES, ids=IDS)
def test_model_matches_np_mpm_and_conserves(name, mats, perturb):
    s, M, out = model_of(name, mats, perturb)
    st = s["state"].select(M.live)
    ref = np_mpm.substep(M.res, 1.0 / M.idx, M.dt, M.g, st.x, st.v, st.B, st.F, st.aux, st.gid, st.gparams, st.gtype,
                         planes=M.planes, friction=M.friction, return_grid=True)

    def close(a, b):
        return np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300)
    raw, grid = out["p2g"]["grid"], out["grid"]["grid"]
    assert close(raw, ref["p2g_grid"]) and close(grid[..., :3], ref["grid"][..., :3]) and close(grid[..., 3], ref["grid"][..., 3])
    for f in ("x", "v", "B", "F"):
        assert close(out[f], ref[f]), f
    assert np.array_equal(out["aux"], ref["aux"])
    # conservation: the weights of a stencil sum to 1 and sum w d = 0, so the affine terms cancel
    mass, mom = M.mass.sum(), (M.mass[:, None] * (M.v + M.g * M.dt)).sum(0)
    assert abs(raw[..., 3].sum() - mass) <= 1e-12 * mass
    scale = np.abs(out["p2g"]["absum"][..., :3]).sum((0, 1, 2))
    assert np.all(np.abs(raw[..., :3].sum((0, 1, 2)) - mom) <= 1e-13 * scale)
    # (a touched node may carry exactly nothing: the third weight of a particle on a face is 0)
    assert not np.any((raw[..., 3] != 0) & ~out["p2g"]["touched"]) and np.all(raw[..., 3] >= 0)
    # which particles the device deletes after G2P must not hang on the last bits of a new position: every new position is at least
    # four times its own bound away from a threshold of particle_key
    for o in (out, out["g2p_own"]):
        assert o["kept_margin"] > 4.0, o["kept_margin"]


def oracle_ratios(orc, name, mats, perturb):
    """largest error / bound of the fp32 CPU oracle per stage: P2G, grid update, G2P from the model's grid (as fp32), whole substep"""
    s, M, out = model_of(name, mats, perturb)
    cfg = ts.oracle_config(s)
    st = s["state"].select(M.live)
    r = {}
    g0 = orc.p2g(cfg, st.copy())
    r["p2g"] = tmod.ratio(g0, out["p2g"]["grid"], out["p2g"]["bound"])
    assert not np.any((g0[..., 3] != 0) & ~out["p2g"]["touched"])
    g1 = orc.grid_update(cfg, g0.copy())
    r["grid"] = tmod.ratio(g1, out["grid"]["grid"], out["grid"]["bound"])
    g32 = out["grid"]["grid"].astype(np.float32)
    want = tmod.g2p(M, g32.astype(np.float64))
    got = st.copy()
    orc.g2p(cfg, got, g32)
    for f in ("x", "v", "B", "F"):
        r["g2p_" + f] = tmod.ratio(getattr(got, f).reshape(want[f].shape), want[f], want[f + "_bound"])
    full = st.copy()
    orc.substep(ts.oracle_config(s), full)
    assert np.array_equal(full.ids, M.ids)
    for f in ("x", "v", "F"):
        r["substep_" + f] = tmod.ratio(getattr(full, f).reshape(out[f].shape), out[f], out[f + "_bound"])
    return r


@pytest.mark.parametrize("name,mats,perturb", [c for c in CASES if c[0] in ts.CUBIC], ids=[i for c, i in zip(CASES, IDS) if c[0] in ts.CUBIC])
def test_fp32_oracle_stays_inside_the_bound(orc, name, mats, perturb):
    """(b): if this fails, K or the position term of tests/transfer_model.py is wrong — not the oracle"""
    r = oracle_ratios(orc, name, mats, perturb)
    msg = "  ".join("%s %.3f" % (k, v[0]) for k, v in r.items())
    print("fp32 oracle, error / bound:", name, mats, perturb, msg)
    assert all(v[0] <= 1.0 for v in r.values()), msg


# ------------------------------------------------------------------------------------------ (c) mutants
def flagged(got, want, bound):
    return tmod.ratio(got, want, bound)[0] > 1.0


def test_a_dropped_corner_contribution_is_flagged_where_the_global_norm_is_blind():
    """one particle's contribution to the corner node (2, 2, 2) of its stencil is lost: the node-by-node check sees it; the rel-L2 over
    the whole grid the parity tests assert (mass 1e-6, momentum 1e-5) does not"""
    s, M, out = model_of("many_blocks")
    w = M.w[:, 2, 0] * M.w[:, 2, 1] * M.w[:, 2, 2]
    # a corner that carries less than 1e-4 of its particle, where it stands out most against the bound of its node
    at = tuple((M.base + 2).T)
    p = int(np.argmax(np.where(w < 1e-4, w * M.mass / out["p2g"]["bound"][..., 3][at], 0.0)))
    assert 1e-7 < w[p] < 1e-4
    print("dropped: %.2e of particle %d, %.1f times the bound of its node" % (w[p], p, w[p] * M.mass[p] / out["p2g"]["bound"][..., 3][at][p]))

    def drop(tap, node, c):
        if tap == (2, 2, 2):
            c = c.copy()
            c[p] = 0.0
        return c, node
    mut = tmod.p2g(M, drop)["grid"]
    good, bound = out["p2g"]["grid"], out["p2g"]["bound"]
    assert flagged(mut[..., 3], good[..., 3], bound[..., 3]) and flagged(mut, good, bound)
    assert rel_l2(mut[..., 3], good[..., 3]) <= 1e-6 and rel_l2(mut[..., :3], good[..., :3]) <= 1e-5
    # and downstream: the normalised velocity of that node, and the particles that gather from it
    mg = tmod.grid_update(M, mut, bound)["grid"]
    assert flagged(mg, out["grid"]["grid"], out["grid"]["bound"])
    # the same fault with a corner of ordinary weight, on every scene
    for name in ts.SCENES:
        s, M, out = model_of(name)
        w = M.w[:, 2, 0] * M.w[:, 2, 1] * M.w[:, 2, 2]
        p = int(np.argmax(w))
        mut = tmod.p2g(M, drop)["grid"]
        assert flagged(mut, out["p2g"]["grid"], out["p2g"]["bound"]), name


@pytest.mark.parametrize("name", ["faces", "many_blocks", "lone_blocks"])
def test_a_base_shifted_by_one_is_flagged(name):
    """one particle's base moves by one node on one axis while fx stays: its whole stencil lands a row off"""
    s, M, out = model_of(name)
    for axis in range(3):
        p = int(np.argmin(M.base[:, axis]))  # (room to move up)

        def shift(tap, node, c):
            node = list(n.copy() for n in node)
            node[axis][p] += 1
            return c, tuple(node)
        mut = tmod.p2g(M, shift)["grid"]
        assert flagged(mut, out["p2g"]["grid"], out["p2g"]["bound"]), axis


@pytest.mark.parametrize("name", ["faces", "runs", "lone_blocks"])
def test_a_lost_tile_seam_is_flagged(name):
    """for one block every contribution to the tile indices 4 and 5 of one axis — the nodes that belong to the next grid block — is lost"""
    s, M, out = model_of(name)
    blk = M.base >> 2
    for axis in range(3):
        cand = np.unique(blk[(M.base[:, axis] & 3) >= 2], axis=0)
        b = cand[len(cand) // 2]
        inb = (blk == b).all(1)

        def seam(tap, node, c):
            lost = inb & (node[axis] - 4 * b[axis] >= 4)
            c = c.copy()
            c[lost] = 0.0
            return c, node
        mut = tmod.p2g(M, seam)["grid"]
        assert flagged(mut, out["p2g"]["grid"], out["p2g"]["bound"]), axis
        assert flagged(mut[..., 3], out["p2g"]["grid"][..., 3], out["p2g"]["bound"][..., 3]), axis


def test_swapped_strides_of_the_dense_view_are_flagged():
    """node (i, j, k) read at (i * nz + j) * ny + k instead of (i * ny + j) * nz + k: invisible on a cubic grid"""
    for name, must in (("non_cubic_no_margin", True), ("faces", True), ("runs", False)):
        s, M, out = model_of(name)
        good = out["p2g"]["grid"]
        nx, ny, nz = good.shape[:3]
        i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
        flat = good.reshape(-1, 4)
        mut = flat[((i * nz + j) * ny + k) % len(flat)]
        assert flagged(mut, good, out["p2g"]["bound"]) == must, name


@pytest.mark.parametrize("name", ["faces", "lone_blocks", "non_cubic_no_margin"])
def test_a_g2p_read_one_row_off_is_flagged(name):
    """one particle gathers one of its 27 nodes from the next row of the grid"""
    s, M, out = model_of(name)
    grid = out["grid"]["grid"]
    want = tmod.g2p(M, grid)
    for axis in range(3):
        p = int(np.argmin(M.base[:, axis]))

        def read(tap, node):
            if tap != (1, 1, 1):
                return node
            node = list(n.copy() for n in node)
            node[axis][p] += 1
            return tuple(node)
        mut = tmod.g2p(M, grid, read=read)
        assert flagged(mut["v"], want["v"], want["v_bound"]) and flagged(mut["B"], want["B"], want["B_bound"]), axis
        assert flagged(mut["x"], want["x"], want["x_bound"]) or np.abs(mut["x"] - want["x"]).max() < 2.0 ** -24 * np.abs(want["x"]).max()
