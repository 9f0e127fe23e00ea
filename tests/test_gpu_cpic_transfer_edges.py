"""k_p2g_rigid and k_g2p_rigid (csrc/k_rigid_transfer.h) node by node, particle by particle and body by body against the float64 model of
tests/cpic_transfer_model.py, on the scenes of tests/cpic_transfer_scenes.py: a block whose boundary list overflows (the cell-by-cell
fallback of the second P2G pass), stencils with nodes of the other colour of two bodies (the ImpulseAcc hand-over in its three forms),
flagged blocks at block coordinate 0 and in the last block of a grid that is not cubic and whose dx is no power of two, a flagged block
without a boundary particle beside unflagged ones, boundary distances on both sides of both edges of the penalty window.  The pattern is
tests/test_gpu_transfer_edges.py's: every device value is held to ITS OWN bound, derived in the model and validated on the CPU
(tests/test_cpic_transfer_model_cpu.py: the compiled reference stays inside it, seeded faults fall outside it; a fallback walk that loses
impulses passes the tolerances of tests/test_gpu_cpic.py).  A ratio error / bound above 1 is a finding about the kernel.

The colour field is an INPUT: it is downloaded from the device after sort + rasterize_rigid_boundary + gather_cdf (held to the reference
entry by entry in tests/test_gpu_cpic.py) and handed to the model, and the scene's assertions (that the list overflows, that both bodies
are met in one stencil, ...) are made on that very field.  Stages of a case: P2G (get_grid(0); the bodies' impulses as mass * dv and
I_world * domega from get_rigid_state before and after), the grid update, G2P from the model's own grid (particles, impulses again), and
a whole substep() on a fresh ctx with the bounds composed (particles, and the bodies' velocities; the poses are not modelled).  With `pytest -s`
every case prints its largest ratio per stage (the table of DESIGN.md)."""
import numpy as np
import pytest

from tests import cpic_transfer_model as cm
from tests import cpic_transfer_runs as ctr
from tests import cpic_transfer_scenes as cts
from tests import kernel_forms as kf
from tests import transfer_model as tmod

pytestmark = pytest.mark.gpu

FORMS = {"default": {}, "deterministic": {"deterministic": True}, "keep_apic_b": {"keep_apic_b": True}}
HARD = ("overflow", "two_bodies")  # every form and material set sees these; every scene sees the default and the deterministic form
CASES = [(n, "jelly", 0.02, f) for n in cts.SCENES for f in ("default", "deterministic")] + \
        [(n, "jelly", 0.0, "default") for n in cts.SCENES] + \
        [(n, "jelly", 0.02, "keep_apic_b") for n in HARD] + \
        [(n, "sand", 0.02, "default") for n in HARD] + \
        [(n, "mixed", 0.02, f) for n in HARD for f in FORMS]
IDS = ["%s-%s" % (cts.case_id(n, m, p), f) for n, m, p, f in CASES]


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


def expected_forms(mats, form):
    keep, det = form == "keep_apic_b", form == "deterministic"
    one = mats != "mixed"
    g2p = kf.g2p(mats if one and not keep else "NO_VISCO", store_b=keep, rigid=True)
    return (g2p,) + kf.beside_a_body("ALL_DET" if det else (mats if one else "ALL"))


def bodies_of(sim, rids):
    return np.stack([ctr.body_row(sim.get_rigid_state(r)) for r in rids])


def colour_field(sim, rids):
    """the record of the device's colour field after sort + rasterize_rigid_boundary + gather_cdf, particles in creation order"""
    p = sim.get_particles(sort_by_id=False)
    o = np.argsort(p["id"], kind="stable")
    b = sim.download_boundary()
    words = sim.download_cdf()[0].reshape(-1)
    nz = np.flatnonzero(words)
    return dict(cdf_idx=nz, cdf_words=words[nz], pstate=p["states"][o].astype(np.uint32), normal=b["normal"][o], dist=b["distance"][o],
                near=b["near"][o], samples=sim.get_rigid_samples(-1)["pos"], bodies0=bodies_of(sim, rids))


def impulses(tag, C, rows_after, res, ratios, bad):
    for b in range(1, len(C.bodies)):
        st = ctr.body_state(rows_after[b - 1])
        got = cm.measured_impulse(C.bodies[b], st["velocity"], st["angular_velocity"])
        bound = cm.measured_bound(C.bodies[b], st["velocity"], st["angular_velocity"], res["impulse_abs"][b], res["impulse_bound"][b])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(got == res["impulse"][b], 0.0, np.abs(got - res["impulse"][b]) / bound)
        ratios[tag] = max(ratios.get(tag, 0.0), float(r.max()))
        if not r.max() <= 1.0:
            bad.append((tag, b, r, got, res["impulse"][b], bound))


def particles(tag, got, M, want, keep_b, ratios, bad):
    assert len(got["x"]) == M.n and np.array_equal(got["gid"], M.gid), tag  # (every particle is kept: creation order)
    for f in ("x", "v", "B", "F", "aux"):
        bound = want[f + "_bound"]
        if f == "B" and not keep_b:
            bound = bound + tmod.folded_B_bound(M, want)
        r, at = tmod.ratio(got[f].reshape(want[f].shape), want[f], bound)
        ratios[tag + "_" + f] = r
        if not r <= 1.0:
            bad.append((tag, f, r, at))


def staged(tm, s, cfg, forms):
    """a ctx of the scene after sort + rasterize_rigid_boundary + gather_cdf, with the model of its colour field"""
    sim, rids = ctr.build_device(tm, s, **cfg)
    kf.assert_runs(sim, *forms)
    sim.sort_particles_and_populate_grid()
    sim.rasterize_rigid_boundary()
    sim.gather_cdf()
    rec = colour_field(sim, rids)
    return sim, rids, rec


@pytest.mark.parametrize("name,mats,perturb,form", CASES, ids=IDS)
def test_colour_aware_transfers_value_by_value(tm, name, mats, perturb, form):
    s = cts.scene(name, mats, perturb)
    cfg, forms = FORMS[form], expected_forms(mats, form)
    keep_b = form == "keep_apic_b"
    ratios, bad = {}, []

    sim, rids, rec = staged(tm, s, cfg, forms)
    M, C = ctr.model_of(s, rec)
    want = cm.substep_cpic(C)
    raw, upd = want["p2g"], want["grid"]
    s["edge"](C, raw, want)  # the run-time input assertions: the device's field takes the path the scene exists for
    X = want["x"] * M.idx
    assert float((np.minimum(X - 0.5, np.asarray(M.res) - 1.5 - X) / (want["x_bound"] * M.idx)).min()) > 4.0  # nobody leaves the grid
    for b in range(1, len(C.bodies)):
        ulp = np.spacing(np.abs(C.bodies[b]["velocity"]).astype(np.float32)).astype(np.float64) / 2
        assert np.all(ulp * C.bodies[b]["mass"] < raw["impulse_bound"][b, :3])
    sim.rasterize_optimized()
    g0 = sim.get_grid(0).astype(np.float64)
    rec["bodies1"] = bodies_of(sim, rids)
    r, at = tmod.ratio(g0, raw["grid"], raw["bound"])
    ratios["p2g"] = r
    if not r <= 1.0:
        bad.append(("p2g", r, at, g0[at[:3]], raw["grid"][at[:3]], raw["bound"][at[:3]]))
    nz = g0[..., 3] != 0
    assert not np.any(nz & ~raw["touched"]), "mass on a node outside every compatible stencil"
    assert np.all(nz[raw["grid"][..., 3] > raw["bound"][..., 3]]), "a node the model gives mass has none"
    if name == "quiet_shell":  # the quiet flagged block and the halo it shares with unflagged blocks: the PLAIN model, the PLAIN bound
        plain, tile = tmod.p2g(M), cts.quiet_tile(M)
        assert len(tile[0]) >= 64
        r, at = tmod.ratio(g0[tile], plain["grid"][tile], plain["bound"][tile])
        ratios["p2g_quiet_plain"] = r
        if not r <= 1.0:
            bad.append(("p2g_quiet_plain", r, at))
    impulses("p2g_impulse", C, rec["bodies1"], raw, ratios, bad)
    sim.normalize_grid_and_apply_boundary_conditions()
    g1 = sim.get_grid(1).astype(np.float64)
    r, at = tmod.ratio(g1, upd["grid"], upd["bound"])
    ratios["grid"] = r
    if not r <= 1.0:
        bad.append(("grid", r, at, g1[at[:3]], upd["grid"][at[:3]], upd["bound"][at[:3]]))
    # G2P alone: from the model's own grid, with the bodies as the device has them after P2G
    grid32 = upd["grid"].astype(np.float32)
    C1 = ctr.model_of(s, rec, "bodies1")[1]
    own = cm.g2p_cpic(C1, grid32.astype(np.float64))
    sim.set_grid(grid32)
    sim.resample_optimized()
    kf.assert_runs(sim, *forms)
    particles("g2p", sim.get_particles(), M, own, keep_b, ratios, bad)
    impulses("g2p_impulse", C1, bodies_of(sim, rids), own, ratios, bad)
    sim.close()

    sim, rids = ctr.build_device(tm, s, **cfg)
    kf.assert_runs(sim, *forms)
    sim.substep()
    sim.synchronize()
    particles("substep", sim.get_particles(), M, want, keep_b, ratios, bad)
    for rid, B in zip(rids, want["bodies_after"]):  # the bodies' velocities through the composed path (P2G, G2P, advect's gravity)
        st = sim.get_rigid_state(rid)
        for f in ("velocity", "angular_velocity"):
            r, _ = tmod.ratio(st[f], B[f], B[f + "_bound"])
            ratios["substep_body"] = max(ratios.get("substep_body", 0.0), r)
            if not r <= 1.0:
                bad.append(("substep_body", rid, f, r, st[f], B[f], B[f + "_bound"]))
    sim.close()
    print("\nerror / bound  %-44s %s" % (IDS[CASES.index((name, mats, perturb, form))], "  ".join("%s %.3f" % (k, v) for k, v in ratios.items())))
    assert not bad, bad


@pytest.mark.parametrize("mats", ["jelly", "mixed"])
def test_deterministic_fallback_walk_gives_the_same_bits_twice(tm, mats):
    """P2G of the overflowing block on two fresh contexts in the deterministic mode: bit-equal bodies (and grids)"""
    s = cts.scene("overflow", mats, 0.02)
    forms = expected_forms(mats, "deterministic")
    runs = []
    for _ in range(2):
        sim, rids, rec = staged(tm, s, FORMS["deterministic"], forms)
        M, C = ctr.model_of(s, rec)
        assert cm.p2g_cpic(C)["boundary_count"].max() > cts.P2GR_LIST
        sim.rasterize_optimized()
        runs.append((bodies_of(sim, rids), sim.get_grid(0)))
        sim.close()
    assert np.any(runs[0][0][:, 7:13] != rec["bodies0"][:, 7:13])  # the bodies did receive impulses
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
