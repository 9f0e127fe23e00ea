"""k_p2g, the grid pass (k_grid.h) and k_g2p / k_g2p_packed node by node and particle by particle against the float64 model of
tests/transfer_model.py, on the scenes of tests/transfer_scenes.py: grids that are not cubic and whose dx is no power of two, blocks
at coordinate 0 and at the last one, stencils that reach node 0 and node res, particles on cell and block faces to the ulp, blocks
with no active neighbour.  Every device value is held to ITS OWN bound — the roundings of its chain of operations times the sum of the
absolute contributions behind it, derived in the model and validated on the CPU (tests/test_transfer_model_cpu.py: the fp32 oracle
stays inside it, seeded faults fall outside it) — where the parity tests hold a rel-L2 over the whole grid, under which a lost corner
contribution disappears.  A ratio error / bound above 1 is a finding about the kernel, not about K.

Stages of a case: P2G (get_grid(0)), grid update (get_grid(1)), G2P from the model's own grid, and a whole substep() with the bounds
composed.  With `pytest -s` every case prints its largest ratio per stage (the table of DESIGN.md)."""
import ctypes as C

import numpy as np
import pytest

from tests import kernel_forms as kf
from tests import transfer_model as tmod
from tests import transfer_scenes as ts

pytestmark = pytest.mark.gpu

FORMS = {  # name: (config keys, environment)
    "default": ({}, {}),
    "deterministic": ({"deterministic": True}, {}),
    "walk0": ({}, {"MPMHIP_GRID_WALK": "0"}),
    "walk2": ({}, {"MPMHIP_GRID_WALK": "2"}),
    "packed0": ({}, {"MPMHIP_G2P_PACKED": "0"}),
    "packed1": ({}, {"MPMHIP_G2P_PACKED": "1"}),
    "keep_apic_b": ({"keep_apic_b": True}, {}),
}
EDGE_SCENES = ("faces", "lone_blocks", "non_cubic_no_margin")  # every form sees these; every scene sees the default form
CASES = [(n, "jelly", p, "default") for n in ts.SCENES for p in (0.0, 0.02)] + \
        [(n, "mixed", p, "default") for n in ts.MIXED_SCENES for p in (0.0, 0.02)] + \
        [(n, "jelly", 0.02, f) for f in FORMS if f != "default" for n in EDGE_SCENES] + \
        [("faces", "mixed", 0.02, "keep_apic_b"), ("faces", "mixed", 0.02, "deterministic")]
IDS = ["%s-%s-%s-%s" % (n, m, "F=I" if p == 0 else "perturbed", f) for n, m, p, f in CASES]


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


def make_sim(tm, s, **cfg):
    """a ctx holding the scene's state in upload order, group by group (past the Python layer's near-boundary filter: the device has
    its own, and it is under test)"""
    sim = tm.create_simulation3("mpm").initialize(dict(res=s["res"], delta_x=s["dx"], base_delta_t=ts.DT, clean_boundary=s["clean_boundary"],
                                                       **cfg))
    ls = tm.mpm.LevelSet(friction=s["friction"])
    for p in s["planes"]:
        ls.add_plane(p[:3], d=p[3])
    sim.set_levelset(ls)
    st = s["state"]
    sim._ensure_ctx(extra=st.n)
    for gi in range(len(st.gtype)):
        params = np.ascontiguousarray(st.gparams[gi], np.float32)
        sim._groups.append((int(st.gtype[gi]), params))
        sim._check(sim._L.mpmhip_add_group(sim._ctx, int(st.gtype[gi]), params.ctypes.data_as(C.POINTER(C.c_float))))
        m = st.gid == gi
        sim._upload_new(gi, st.x[m], st.v[m], st.F[m], st.B[m], st.aux[m])
    sim._n_added = st.n
    return sim


def expected_form(mats, form):
    keep = form == "keep_apic_b"
    mset = "NO_VISCO" if (mats == "mixed" or keep) else mats  # (the one-material kernels exist only without apic_b)
    return kf.packed(mset) if form == "packed1" else kf.g2p(mset, store_b=keep)


def check_particles(tag, got, M, want, keep_b, ratios, bad):
    """the device's particles against the model's, one by one: the same ids kept, every field inside its bound"""
    kept = want["kept"]
    assert np.array_equal(got["id"], M.ids[kept]), (tag, len(got["id"]), int(kept.sum()))
    assert np.array_equal(got["gid"], M.gid[kept]) and np.array_equal(got["aux"], M.aux[kept].astype(np.float32))
    for f in ("x", "v", "B", "F"):
        bound = want[f + "_bound"]
        if f == "B" and not keep_b:
            bound = bound + tmod.folded_B_bound(M, want)
        r, at = tmod.ratio(got[f].reshape((-1,) + want[f].shape[1:]), want[f][kept], bound[kept])
        ratios[tag + "_" + f] = r
        if not r <= 1.0:
            bad.append((tag, f, r, at))


@pytest.mark.parametrize("name,mats,perturb,form", CASES, ids=IDS)
def test_transfers_node_by_node_and_particle_by_particle(tm, monkeypatch, name, mats, perturb, form):
    s, M, want = ts.modelled(name, mats, perturb)
    assert want["kept_margin"] > 4.0 and want["g2p_own"]["kept_margin"] > 4.0
    cfg, env = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    keep_b = bool(cfg.get("keep_apic_b"))
    ratios, bad = {}, []
    raw, upd = want["p2g"], want["grid"]

    sim = make_sim(tm, s, **cfg)
    kf.assert_runs(sim, expected_form(mats, form))
    sim.sort_particles_and_populate_grid()
    sim.rasterize_optimized()
    g0 = sim.get_grid(0).astype(np.float64)
    r, at = tmod.ratio(g0, raw["grid"], raw["bound"])
    ratios["p2g"] = r
    if not r <= 1.0:
        bad.append(("p2g", r, at, g0[at[:3]], raw["grid"][at[:3]], raw["bound"][at[:3]]))
    nz = g0[..., 3] != 0
    assert not np.any(nz & ~raw["touched"]), "mass on a node outside every live stencil"
    assert np.all(nz[raw["grid"][..., 3] > raw["bound"][..., 3]]), "a node the model gives mass has none"
    # totals against the particles: sum of the nodes' bounds (the affine terms cancel: sum w d = 0)
    total = np.concatenate([(M.mass[:, None] * (M.v + M.g * M.dt)).sum(0), [M.mass.sum()]])
    r_tot = float((np.abs(g0.sum((0, 1, 2)) - total) / raw["bound"].sum((0, 1, 2))).max())
    ratios["p2g_total"] = r_tot
    if not r_tot <= 1.0:
        bad.append(("p2g_total", r_tot))
    sim.normalize_grid_and_apply_boundary_conditions()
    g1 = sim.get_grid(1).astype(np.float64)
    r, at = tmod.ratio(g1, upd["grid"], upd["bound"])
    ratios["grid"] = r
    if not r <= 1.0:
        bad.append(("grid", r, at, g1[at[:3]], upd["grid"][at[:3]], upd["bound"][at[:3]]))
    # G2P alone, from the model's own grid (tests/test_gpu_parity.py: g2p_from; the tile / owner structure is the one just built)
    sim.set_grid(want["grid32"])
    sim.resample_optimized()
    kf.assert_runs(sim, expected_form(mats, form))  # (also with what the sort has reported by now)
    check_particles("g2p", sim.get_particles(), M, want["g2p_own"], keep_b, ratios, bad)
    sim.close()

    sim = make_sim(tm, s, **cfg)
    kf.assert_runs(sim, expected_form(mats, form))
    sim.substep()
    sim.synchronize()
    check_particles("substep", sim.get_particles(), M, want, keep_b, ratios, bad)
    sim.close()
    print("\nerror / bound  %-58s %s" % ("-".join((name, mats, "F=I" if perturb == 0 else "perturbed", form)),
                                        "  ".join("%s %.3f" % (k, v) for k, v in ratios.items())))
    assert not bad, bad
