"""tests/cpic_transfer_model.py without a GPU: the float64 model of the colour-aware transfers reduces to the plain model where nothing
is coloured; the compiled REFERENCE (src/transfer.cpp:367-463, 706-835 — fp32, one impulse added at a time), run stage by stage on the
scenes of tests/cpic_transfer_scenes.py, stays inside the model's bounds node by node, particle by particle and impulse by impulse
(from tests/golden/ref_cpic_transfer.npz on any machine, live as well where oracle/_ref/libmpm_ref.so exists); and seeded faults of the
kind the kernels of csrc/k_rigid_transfer.h could have fall outside them — the first of which passes the tolerances the whole-substep
parity tests (tests/test_gpu_cpic.py: check_run) hold a run to.  Every scene asserts on the reference's own colour field what it is for."""
import os

import numpy as np
import pytest

from tests import cpic_transfer_model as cm
from tests import cpic_transfer_runs as ctr
from tests import cpic_transfer_scenes as cts
from tests import transfer_model as tmod

HERE = os.path.dirname(__file__)
IDS = lambda cases: [cts.case_id(*c) for c in cases]  # noqa: E731


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "ref_cpic_transfer.npz"))


def record(gold, name, mats="jelly", perturb=0.02):
    pre = cts.case_id(name, mats, perturb) + "/"
    return {k[len(pre):]: gold[k] for k in gold.files if k.startswith(pre)}


_MODELS = {}


def modelled(gold, name, mats="jelly", perturb=0.02):
    """(scene, record, Cpic, p2g_cpic, g2p_cpic from the reference's own fp32 grid with its bodies after P2G) of a fixture case, once"""
    k = (name, mats, perturb)
    if k not in _MODELS:
        s = cts.scene(name, mats, perturb)
        rec = record(gold, name, mats, perturb)
        _MODELS[k] = (s, rec) + run_model(s, rec)
    return _MODELS[k]


def run_model(s, rec):
    M, C = ctr.model_of(s, rec)
    raw = cm.p2g_cpic(C)
    C1 = ctr.model_of(s, rec, "bodies1")[1]
    out = cm.g2p_cpic(C1, ctr.dense(s, rec["grid_idx"], rec["grid1"]).astype(np.float64))
    return C, raw, C1, out


def impulse_ratios(C, rows_after, res):
    """per body: |measured impulse - model| / bound, six components"""
    out = []
    for b in range(1, len(C.bodies)):
        st = ctr.body_state(rows_after[b - 1])
        got = cm.measured_impulse(C.bodies[b], st["velocity"], st["angular_velocity"])
        bound = cm.measured_bound(C.bodies[b], st["velocity"], st["angular_velocity"], res["impulse_abs"][b], res["impulse_bound"][b])
        out.append(np.abs(got - res["impulse"][b]) / bound)
    return np.array(out)


def check_record(s, rec):
    """every node, every particle field and every body impulse of a stage-by-stage run inside the model's bound; the scene's own edge"""
    C, raw, C1, out = run_model(s, rec)
    M = C.M
    s["edge"](C, raw, out)
    for b in range(1, len(C.bodies)):  # the impulse shows as a velocity change: half an ulp of the velocity, times the mass, is below its bound
        ulp = np.spacing(np.abs(C.bodies[b]["velocity"]).astype(np.float32)).astype(np.float64) / 2
        assert np.all(ulp * C.bodies[b]["mass"] < raw["impulse_bound"][b, :3]), (b, ulp * C.bodies[b]["mass"], raw["impulse_bound"][b, :3])
    ratios = {}
    assert rec["grid0_rest"] == 0
    g0 = ctr.dense(s, rec["grid_idx"], rec["grid0"]).astype(np.float64)
    ratios["p2g"] = tmod.ratio(g0, raw["grid"], raw["bound"])[0]
    assert not np.any((g0[..., 3] != 0) & ~raw["touched"])
    if s["name"] == "quiet_shell":  # the quiet flagged block and its halo: the PLAIN model inside the PLAIN bound
        plain, tile = tmod.p2g(M), cts.quiet_tile(M)
        assert len(tile[0]) >= 64
        ratios["p2g_quiet_plain"] = tmod.ratio(g0[tile], plain["grid"][tile], plain["bound"][tile])[0]
    ratios["p2g_impulse"] = impulse_ratios(C, rec["bodies1"], raw).max()
    upd = tmod.grid_update(M, raw["grid"], raw["bound"])
    ratios["grid"] = tmod.ratio(ctr.dense(s, rec["grid_idx"], rec["grid1"]).astype(np.float64), upd["grid"], upd["bound"])[0]
    for f in ("x", "v", "B", "F", "aux"):
        ratios["g2p_" + f] = tmod.ratio(rec[f].reshape(out[f].shape), out[f], out[f + "_bound"])[0]
    ratios["g2p_impulse"] = impulse_ratios(C1, rec["bodies2"], out).max()
    print("\nerror / bound  %-32s %s" % (cts.case_id(s["name"], s["mats"], s["perturb"]), "  ".join("%s %.3f" % kv for kv in ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- reduction to the plain model
@pytest.mark.parametrize("name", ["two_bodies", "edges"])
def test_without_colours_the_model_is_the_plain_one(gold, name):
    s, rec, C, _, _, _ = modelled(gold, name)
    M = C.M
    Z = cm.Cpic(M, np.zeros_like(C.words), np.zeros_like(C.pstate), C.normal, C.dist, np.zeros(M.n), rec["samples"], C.bodies[1:], cts.PENALTY, cts.PUSHING_FORCE)
    assert Z.flagged.sum() > 100
    a, b = cm.p2g_cpic(Z), tmod.p2g(M)
    np.testing.assert_allclose(a["grid"], b["grid"], rtol=0, atol=1e-12 * np.abs(b["grid"]).max())
    assert np.array_equal(a["count"], b["count"]) and not a["other"].any() and not a["impulse"].any()
    grid = tmod.grid_update(M, b["grid"], b["bound"])["grid"]
    c, d = cm.g2p_cpic(Z, grid), tmod.g2p(M, grid)
    for f in ("x", "v", "B", "F"):
        np.testing.assert_allclose(c[f], d[f], rtol=0, atol=1e-12 * max(np.abs(d[f]).max(), 1.0))
    assert not c["impulse"].any() and not c["penalised"].any()


def bodyless(C):
    """the field with the body id taken off every coloured node: a SYNTHETIC field (a real one never holds such a node,
    tests/cpic_transfer_scenes.py: edges_edge) for the `rid < 0` branches"""
    import copy
    Z = copy.copy(C)
    Z.words = C.words & np.uint32(cm.TAG_MASK)
    return Z


def test_without_body_ids_nobody_receives_an_impulse(gold):
    s, rec, C, raw, C1, out = modelled(gold, "window")
    a = cm.p2g_cpic(bodyless(C))
    assert a["other"].sum() == raw["other"].sum() > 100 and np.array_equal(a["grid"], raw["grid"])  # the nodes are skipped all the same
    assert not a["impulse"].any() and not a["impulse_bound"].any()
    b = cm.g2p_cpic(bodyless(C1), ctr.dense(s, rec["grid_idx"], rec["grid1"]).astype(np.float64))
    assert b["penalised"].sum() == out["penalised"].sum() >= 32 and not b["impulse"].any()
    assert np.abs(b["v"] - out["v"]).max() > 1e-3  # (v_body = 0, friction = 0 in the projection)


# ---------------------------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize("case", cts.FIXTURE_CASES, ids=IDS(cts.FIXTURE_CASES))
def test_recorded_reference_stays_inside_the_bounds(gold, case):
    check_record(cts.scene(*case), record(gold, *case))


@pytest.mark.parametrize("case", cts.LIVE_CASES, ids=IDS(cts.LIVE_CASES))
def test_live_reference_stays_inside_the_bounds(case):
    from oracle import refmpm
    if not refmpm.available():
        pytest.skip("oracle/_ref/libmpm_ref.so is not built here")
    check_record(cts.scene(*case), ctr.record_reference(refmpm, cts.scene(*case)))


def test_fixture_is_what_the_live_reference_records(gold):
    from oracle import refmpm
    if not refmpm.available():
        pytest.skip("oracle/_ref/libmpm_ref.so is not built here")
    rec = ctr.record_reference(refmpm, cts.scene("quiet_shell", "jelly", 0.02))
    old = record(gold, "quiet_shell")
    assert set(rec) == set(old)
    for k in ("cdf_idx", "cdf_words", "pstate", "near", "grid_idx"):
        assert np.array_equal(rec[k], old[k]), k


# ---------------------------------------------------------------------------------------------- seeded faults
# the mutants, as hooks of cpic_transfer_model.p2g_cpic / g2p_cpic
def bodyless_compatible(tap, node, other, rid):
    """a coloured node without a body id treated as compatible"""
    return other & (rid > 0)


def lose_tile_node(M, block, lost):
    """the contributions of `block`'s particles to the node `lost` never reach the grid"""
    def contrib(tap, node, c):
        return c * ~(((M.base >> 2) == np.asarray(block)).all(1) & (np.stack(node, 1) == np.asarray(lost)).all(1))[:, None]
    return contrib


def credit_first(sel, rid, state):
    """a lane that meets a second body goes on adding to the first"""
    fb = state["first_body"][sel]
    return np.where(fb > 0, fb, rid), np.ones(len(sel), bool)


def drop_listed_after(limit):
    """in a block with more than `limit` boundary particles, those past entry `limit` (creation order) hand over nothing"""
    def credit(sel, rid, state):
        if "rank" not in state:
            rank = np.zeros(len(state["other"]), np.int64)
            for b in np.argwhere(state["boundary_count"] > limit):
                m = np.flatnonzero(state["other"] & (state["block"] == b).all(1))
                rank[m] = np.arange(len(m))
            state["rank"] = rank
        return rid, state["rank"][sel] < limit
    return credit


def imp_ratio(C, raw, mutant):
    """a mutant's impulses against the model's, in units of the bound"""
    return (np.abs(mutant["impulse"] - raw["impulse"])[1:] / raw["impulse_bound"][1:]).max()


def old_tolerances_pass(want, got):
    """check_run of tests/test_gpu_cpic.py, with the model's substep in the place of the recorded run"""
    def rel_l2(a, b):
        return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)
    ok = np.abs(got["x"] - want["x"]).max() <= 5e-6 and rel_l2(got["v"], want["v"]) <= 2e-4 and rel_l2(got["F"], want["F"]) <= 1e-4
    for a, b in zip(want["bodies"], got["bodies"]):
        for f in ("velocity", "angular_velocity"):
            ok = ok and np.all(np.abs(a[f] - b[f]) <= 2e-4 * max(np.abs(a[f]).max(), 1e-2))
    return bool(ok)


def test_fault_fallback_walk_drops_the_particles_past_the_list(gold):
    """the gap, demonstrated: a fallback walk that stops at entry 1024 loses the impulses of the particles behind it — far outside the bound, and
    inside every tolerance of the whole-substep comparison"""
    s, rec, C, raw, _, _ = modelled(gold, "overflow")
    assert raw["boundary_count"].max() > cts.P2GR_LIST
    mutant = cm.p2g_cpic(C, hooks=dict(credit=drop_listed_after(cts.P2GR_LIST)))
    assert np.array_equal(mutant["grid"], raw["grid"])
    r = imp_ratio(C, raw, mutant)
    assert r > 1.0, r
    want = cm.substep_cpic(C)
    bodies = cm.apply_impulses(C, mutant["impulse"], mutant["impulse_bound"])
    got = cm.g2p_cpic(C.with_bodies(bodies), want["grid"]["grid"], want["grid"]["bound"])
    got["bodies"] = bodies
    assert np.abs(got["bodies"][0]["velocity"] - want["bodies"][0]["velocity"]).max() > 0
    assert old_tolerances_pass(want, got)
    print("\nfallback walk stops at the list's end: impulse error / bound %.1f, passes the whole-substep tolerances" % r)


def test_fault_second_body_credited_to_the_first(gold):
    s, rec, C, raw, _, _ = modelled(gold, "two_bodies")
    r = imp_ratio(C, raw, cm.p2g_cpic(C, hooks=dict(credit=credit_first)))
    assert r > 1.0, r


@pytest.mark.parametrize("name", ["two_bodies", "window"])
def test_fault_friction_side_swapped(gold, name):
    s, rec, C, raw, C1, out = modelled(gold, name)
    r = imp_ratio(C, raw, cm.p2g_cpic(C, hooks=dict(side=True)))
    assert r > 1.0, r
    mutant = cm.g2p_cpic(C1, ctr.dense(s, rec["grid_idx"], rec["grid1"]).astype(np.float64), hooks=dict(side=True))
    r = tmod.ratio(mutant["v"], out["v"], out["v_bound"])[0]
    assert r > 1.0, r


def test_fault_penalty_impulse_credited_to_the_first_body_met(gold):
    s, rec, C, raw, C1, out = modelled(gold, "two_bodies")
    mutant = cm.g2p_cpic(C1, ctr.dense(s, rec["grid_idx"], rec["grid1"]).astype(np.float64), hooks=dict(penalty_body=lambda first, last: first))
    assert np.array_equal(mutant["v"], out["v"])
    r = (np.abs(mutant["impulse"] - out["impulse"])[1:] / out["impulse_bound"][1:]).max()
    assert r > 1.0, r


def test_fault_bodyless_coloured_node_treated_as_compatible(gold):
    s, rec, C, raw, C1, out = modelled(gold, "edges")
    Z = bodyless(C)
    a, mutant = cm.p2g_cpic(Z), cm.p2g_cpic(Z, hooks=dict(other=bodyless_compatible))
    r = tmod.ratio(mutant["grid"], a["grid"], a["bound"])[0]
    assert r > 1.0, r
    grid = ctr.dense(s, rec["grid_idx"], rec["grid1"]).astype(np.float64)
    b, mutant = cm.g2p_cpic(bodyless(C1), grid), cm.g2p_cpic(bodyless(C1), grid, hooks=dict(other=bodyless_compatible))
    r = tmod.ratio(mutant["v"], b["v"], b["v_bound"])[0]
    assert r > 1.0, r


def test_fault_penalty_window_lower_edge_misplaced(gold):
    s, rec, C, raw, C1, out = modelled(gold, "window")
    mutant = cm.g2p_cpic(C1, ctr.dense(s, rec["grid_idx"], rec["grid1"]).astype(np.float64), hooks=dict(window=lambda lo, hi: (np.float32(-C.M.dx) * np.float32(0.03), hi)))
    assert mutant["penalised"].sum() != out["penalised"].sum()
    r = tmod.ratio(mutant["v"], out["v"], out["v_bound"])[0]
    assert r > 1.0, r
    r = (np.abs(mutant["impulse"] - out["impulse"])[1:] / out["impulse_bound"][1:]).max()
    assert r > 1.0, r


def test_fault_halo_node_of_a_flagged_tile_lost(gold):
    """the quiet flagged block next to a block without the flag: its nodes equal the PLAIN model's inside the plain bound, and one
    tile node lost on the seam does not"""
    s, rec, C, raw, _, _ = modelled(gold, "quiet_shell")
    M = C.M
    plain = tmod.p2g(M)
    blk, nxt = np.array((2, 3, 2)), np.array((2, 4, 2))
    mine, theirs = ((M.base >> 2) == blk).all(1), ((M.base >> 2) == nxt).all(1)
    reach = np.zeros(raw["count"].shape, np.int64)
    for who, bit in ((mine, 1), (theirs, 2)):
        for tap, node, ww, d, dw in M.taps():
            reach[tuple(a[who] for a in node)] |= bit
    seam = np.argwhere(reach == 3)
    assert len(seam) >= 4, "the two blocks share no node"
    tile = np.argwhere(reach & 1 != 0)
    r, _ = tmod.ratio(raw["grid"][tuple(tile.T)], plain["grid"][tuple(tile.T)], plain["bound"][tuple(tile.T)])
    assert r <= 1.0, r
    mutant = cm.p2g_cpic(C, hooks=dict(contrib=lose_tile_node(M, blk, seam[0])))
    r = tmod.ratio(mutant["grid"], raw["grid"], raw["bound"])[0]
    assert r > 1.0, r
