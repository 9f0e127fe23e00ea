"""GPU parity tests against the REFERENCE's own arithmetic (run with -m gpu on an MI355X).

Two sources of truth, both produced by the reference's solver compiled from its sources where they lie
(oracle/_ref/libmpm_ref.so, see oracle/Makefile: ref_mpm and oracle/taichi_shim/taichi/common/util.h):
  * the committed fixtures tests/golden/{ref_materials,ref_shapes}.npz (+ substep_*.npz in tests/test_gpu_parity.py),
  * the library itself, run LIVE on the GPU box's host cores on the BASELINE configurations at full size — C2 (128^3 /
    1 M jelly, jittered + stirred + perturbed F), C3 (256^3 / 8 M sand), the C3 scene AFTER it hit the floor (the
    state bench.py's `evolved` line times), and a two-cluster reduction of C5 on the 512^3 grid.
The HIP library is called through the C ABI (ctypes, taichi_mpm_amd/mpm.py).

Tolerances (fp32): after one P2G grid m rel-L2 <= 1e-6, m v <= 1e-5; after one G2P / one substep:
x abs <= 2e-7 (L = 1), v, F rel-L2 <= 2e-5 (return-mapped materials 1e-4); apic_b rel-L2 <= 1e-5 stored, 3e-4 recovered.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests.common import lattice_cube, load_golden, make_state, rel_l2

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(__file__)
MATS = ["jelly", "snow", "sand", "water", "linear", "elastic", "von_mises", "visco"]
F_TOL = {"snow": 1e-4, "sand": 1e-4, "von_mises": 1e-4, "visco": 1e-4}


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


@pytest.fixture(scope="module")
def ref():
    from oracle import refmpm
    if not refmpm.available():
        pytest.skip("oracle/_ref/libmpm_ref.so did not travel to this box")
    refmpm.set_threads(min(64, os.cpu_count() or 1))
    return refmpm


def hip_sim(tm, res, dx, dt, levelset=None, **cfg):
    sim = tm.create_simulation3("mpm").initialize(dict(res=(res,) * 3, delta_x=dx, base_delta_t=dt, **cfg))
    if levelset is not None:
        sim.set_levelset(levelset)
    return sim


def add_state(sim, tm, s):
    names = {v: k for k, v in tm.MATERIAL_IDS.items()}
    for gi in range(len(s.gtype)):
        m = s.gid == gi
        sim.add_particles(dict(type=names[int(s.gtype[gi])], positions=s.x[m], velocities=s.v[m], F=s.F[m], B=s.B[m],
                               aux=s.aux[m], params=s.gparams[gi]))


def levelset_of(tm, rows, friction):
    ls = tm.mpm.LevelSet(friction=friction)
    for r in rows:
        t, io, p = int(r[0]), bool(r[1]), list(r[2:]) + [0.0] * (8 - len(r))
        if t == 0:
            ls.add_plane(p[0:3], d=p[3])
        elif t == 1:
            ls.add_sphere(p[0:3], p[3], io)
        else:
            ls.add_cuboid(p[0:3], p[3:6], io)
    return ls


# ------------------------------------------------------------------------------------------ fixtures of the reference
@pytest.mark.parametrize("mat", MATS)
def test_device_materials_match_the_reference(tm, mat):
    """mpmhip_debug_force / mpmhip_debug_plasticity (the device's calculate_force, plasticity and the fused
    plasticity + next stress) against MPMParticle::calculate_force / plasticity of src/particles.cpp"""
    g = np.load(os.path.join(HERE, "golden", "ref_materials.npz"))
    gp, t = np.ascontiguousarray(g[mat + "_gp"], np.float32), int(g[mat + "_type"])
    F, cdg, aux = (np.ascontiguousarray(g[mat + k], np.float32) for k in ("_F", "_cdg", "_aux"))
    n = len(F)
    sim = hip_sim(tm, 32, 1 / 32, 1e-4)
    sim.add_particles(dict(type="jelly", positions=lattice_cube(32, 10, 12, 1 / 32)))
    sim._ensure_ctx()
    fp = C.POINTER(C.c_float)
    out = np.zeros((n, 9), np.float32)
    sim._check(sim._L.mpmhip_debug_force(sim._ctx, t, gp.ctypes.data_as(fp), n, F.ctypes.data_as(fp), aux.ctypes.data_as(fp),
                                         out.ctypes.data_as(fp)))
    want = g[mat + "_force"]
    ok = np.isfinite(want).all(1)
    atol = 2 * gp[2] * gp[1] * 4e-6 if mat != "water" else 0.0  # F - R cancellation: absolute error ~ 2 mu vol eps
    assert np.abs(out[ok] - want[ok]).max() <= 3e-5 * np.abs(want[ok]).max() + atol, mat
    Fd, auxd, nf = F.copy(), aux.copy(), np.zeros((n, 9), np.float32)
    sim._check(sim._L.mpmhip_debug_plasticity(sim._ctx, t, gp.ctypes.data_as(fp), n, cdg.ctypes.data_as(fp), Fd.ctypes.data_as(fp),
                                              auxd.ctypes.data_as(fp), nf.ctypes.data_as(fp)))
    F2, aux2, f2 = g[mat + "_F2"], g[mat + "_aux2"], g[mat + "_force2"]
    ok = np.isfinite(F2).all(1) & np.isfinite(f2).all(1)
    if mat == "water":
        Fd = F  # water never updates dg_e (src/particles.cpp:469-478); the kernel does not store it either
    assert np.abs(Fd[ok] - F2[ok]).max() <= 2e-5, mat
    assert np.abs(auxd[ok] - aux2[ok]).max() <= 2e-5 * max(1.0, np.abs(aux2[ok]).max()), mat
    assert np.abs(nf[ok] - f2[ok]).max() <= 3e-5 * np.abs(f2[ok]).max() + atol, mat
    sim.close()


def _shape_cases():
    g = load_golden("ref_shapes")
    return g, json.loads(str(g["cases"]))


SHAPE_CASES = ["static_shapes", "slip_sphere", "particle_collision", "grid_gravity", "moving_plane", "moving_sphere",
               "shrinking_box", "apic_damping_only", "both_dampings"]


@pytest.mark.parametrize("mat", ["jelly", "sand"])
@pytest.mark.parametrize("case", SHAPE_CASES)
def test_level_sets_moving_level_sets_and_config_variants_match_the_reference(tm, case, mat):
    """three substeps with planes / spheres / cuboid containers, DynamicLevelSet key frames (boundary velocity
    -dphi/dt n dx, src/mpm.cpp:323-342), particle_collision, grid-side gravity and APIC/RPIC damping.  For the damping
    cases the reference's GENERIC path is the yardstick (its optimised path has the block-index quirk,
    src/transfer.cpp:925-926 — SURVEY quirk 3)."""
    g, cases = _shape_cases()
    c = cases[case]
    res, dx, dt = int(g["res"]), float(g["dx"]), float(g["dt"])
    a = g["in_" + mat]
    sim = hip_sim(tm, res, dx, dt, **c["cfg"])
    if c.get("shapes1") is not None:
        sim.set_levelset(tm.mpm.DynamicLevelSet().initialize(0.0, c["t1"], levelset_of(tm, c["shapes"], c["friction"]),
                                                             levelset_of(tm, c["shapes1"], c["friction"])))
    else:
        sim.set_levelset(levelset_of(tm, c["shapes"], c["friction"]))
    sim.add_particles(dict(type=mat, positions=a[:, 0:3], velocities=a[:, 3:6], B=a[:, 6:15], F=a[:, 15:24], aux=a[:, 24],
                           params=g["gp_" + mat]))
    for _ in range(3):
        sim.substep()
    got = sim.get_particles()
    key = "%s_%s_%s" % (case, mat, "gen" if "damping" in case else "opt")
    if key not in g:
        pytest.skip("fixture holds this case for jelly only")
    want = g[key]
    assert np.array_equal(got["id"], g[key + "_ids"])
    assert np.abs(got["x"] - want[:, 0:3]).max() <= 5e-7
    assert rel_l2(got["v"], want[:, 3:6]) <= 5e-5 and rel_l2(got["F"], want[:, 6:15]) <= 2e-4
    sim.close()


# ------------------------------------------------------------------------------------------ live reference, full size
def _compare_one_substep_phase_by_phase(tm, ref, s, res, mat, shapes, friction, tol_F, label):
    """HIP vs reference on the same state: grid after P2G, grid after the update, particles after G2P; then one full
    substep of both from the same input"""
    dx, dt = 1.0 / res, 1e-4
    gp = s.gparams[0]
    r = ref.Sim(res, dx, dt, shapes=shapes, friction=friction)
    r.add_particles(mat, gp[0], gp[1], s.x, s.v, s.F, s.B, s.aux)
    r.sort(); r.p2g(True)
    g_ref = r.download_grid()
    sim = hip_sim(tm, res, dx, dt, levelset=levelset_of(tm, shapes, friction), keep_apic_b=True)
    add_state(sim, tm, s)
    sim.sort_particles_and_populate_grid()
    sim.rasterize_optimized()
    g_hip = sim.get_grid(0)
    nz = g_ref[..., 3] != 0
    assert np.array_equal(nz, g_hip[..., 3] != 0), label
    assert rel_l2(g_hip[nz][:, 3], g_ref[nz][:, 3]) <= 1e-6, label
    assert rel_l2(g_hip[nz][:, :3], g_ref[nz][:, :3]) <= 1e-5, label
    r.grid_update()
    sim.normalize_grid_and_apply_boundary_conditions()
    g_ref1, g_hip1 = r.download_grid(), sim.get_grid(1)
    assert rel_l2(g_hip1[nz][:, :3], g_ref1[nz][:, :3]) <= 1e-5, label
    del g_ref, g_hip, g_hip1
    sim.set_grid(g_ref1)  # identical grid on both sides for the G2P comparison
    del g_ref1
    r.g2p(True)
    sim.resample_optimized()
    a, b = sim.get_particles(), r.download()
    assert np.array_equal(a["id"], b["id"]), label
    assert np.abs(a["x"] - b["x"]).max() <= 2e-7, label
    assert rel_l2(a["v"], b["v"]) <= 1e-5 and rel_l2(a["B"], b["B"]) <= 1e-5, label
    assert rel_l2(a["F"], b["F"]) <= tol_F, label
    assert np.abs(a["aux"] - b["aux"]).max() <= 2e-5 * max(1.0, np.abs(b["aux"]).max()), label
    sim.close(); r.close()
    # one whole substep (default ctx mode: apic_b folded into the P2G affine matrix)
    r = ref.Sim(res, dx, dt, shapes=shapes, friction=friction)
    r.add_particles(mat, gp[0], gp[1], s.x, s.v, s.F, s.B, s.aux)
    r.substep(1)
    sim = hip_sim(tm, res, dx, dt, levelset=levelset_of(tm, shapes, friction))
    add_state(sim, tm, s)
    sim.substep()
    a, b = sim.get_particles(), r.download()
    sim.close(); r.close()
    assert np.array_equal(a["id"], b["id"]), label
    assert np.abs(a["x"] - b["x"]).max() <= 2e-7, label
    assert rel_l2(a["v"], b["v"]) <= 2e-5 and rel_l2(a["F"], b["F"]) <= max(tol_F, 2e-5), label
    assert rel_l2(a["B"], b["B"]) <= 3e-4, label  # recovered from A (include/mpmhip.h: discard_apic_b)


def test_c2_full_size_against_the_live_reference(tm, ref):
    """BASELINE configs[1]: 128^3 grid, 50^3 cells x 8 = 1 000 000 fixed-corotated jelly particles — jittered,
    stirred (rotating + shearing velocity field, random apic_b) and with perturbed F, sticky floor"""
    res = 128
    lo = res // 2 - 25
    x = lattice_cube(res, lo, lo + 50, 1.0 / res, jitter=0.2, seed=31)
    s = make_state(x, "jelly", 1.0 / res, perturb_F=0.03, seed=32, vel_scale=1.5)
    assert s.n == 1_000_000
    _compare_one_substep_phase_by_phase(tm, ref, s, res, "jelly", [(0, 0, 0, 1, 0, -0.1)], -1.0, 1e-5, "C2")


def test_c3_full_size_against_the_live_reference(tm, ref):
    """BASELINE configs[2]: 256^3 grid, 100^3 cells x 8 = 8 000 000 Drucker-Prager sand particles (jittered, stirred,
    perturbed F so that the return map is active), sticky floor"""
    res = 256
    lo = res // 2 - 50
    x = lattice_cube(res, lo, lo + 100, 1.0 / res, jitter=0.2, seed=41)
    s = make_state(x, "sand", 1.0 / res, perturb_F=0.02, seed=42, vel_scale=1.0)
    assert s.n == 8_000_000
    _compare_one_substep_phase_by_phase(tm, ref, s, res, "sand", [(0, 0, 0, 1, 0, -0.1)], -1.0, 1e-4, "C3")


def test_c3_after_floor_impact_one_further_substep_matches_the_live_reference(tm, ref):
    """the state bench.py times as `evolved`: the C3 block dropped onto the floor and run for >= 300 substeps after the
    impact on the DEVICE (uneven cells, decayed slot order, both k_rank paths, active Drucker-Prager return map, F far
    from the identity); the state is downloaded and ONE further substep is compared with the reference from the same
    state"""
    from bench import CONFIGS, build_sim, evolve_to_impact
    cfg = CONFIGS["c3"]
    sim = build_sim(tm, dict(cfg, keep_apic_b=True), 0)
    n_sub = evolve_to_impact(sim, cfg)
    assert n_sub >= 300
    st = sim.get_particles()
    n = len(st["x"])
    assert 7_000_000 < n <= 8_000_000
    # the evolved state is really evolved
    assert np.abs(st["F"] - np.eye(3, dtype=np.float32).reshape(1, 9)).max() > 0.05
    assert st["x"][:, 1].min() < 0.1 + 4.0 / 256
    gp, _ = tm.materials.group_params("sand", 400.0 * (1 / 256) ** 3 / 8, (1 / 256) ** 3 / 8)
    r = ref.Sim(256, 1 / 256, 1e-4, shapes=[(0, 0, 0, 1, 0, -0.1)], friction=-1.0)
    r.add_particles("sand", gp[0], gp[1], st["x"], st["v"], st["F"], st["B"], st["aux"])
    r.set_time(sim.get_current_time())
    r.substep(1)
    sim.substep()
    a, b = sim.get_particles(), r.download()
    sim.close(); r.close()
    ids = st["id"]  # the reference numbered the uploaded particles 0..n-1 in the order of st (ascending device id)
    assert len(a["x"]) == len(b["x"])
    keep = np.isin(ids, a["id"])  # (particles deleted near the walls by this substep drop out on both sides)
    assert keep.sum() == len(a["x"]) and np.array_equal(np.nonzero(keep)[0], b["id"])
    assert np.abs(a["x"] - b["x"]).max() <= 2e-7
    assert rel_l2(a["v"], b["v"]) <= 2e-5
    assert rel_l2(a["F"], b["F"]) <= 1e-4
    assert np.abs(a["aux"] - b["aux"]).max() <= 5e-5


def test_c5_two_cluster_reduction_against_the_live_reference(tm, ref):
    """BASELINE configs[4] reduced to two clusters on the full 512^3 grid (Morton keys beyond 2^24, >64 blocks per
    axis): one water and one Hencky-elastic cube of 64^3 cells x 8 at opposite corners of the cluster arrangement"""
    res = 512
    dx = 1.0 / res
    vol = dx ** 3 / 8
    from oracle import oracle as orc
    states = []
    for k, (mat, lo) in enumerate((("water", (78, 78, 78)), ("elastic", (370, 370, 370)))):
        x = lattice_cube(res, 0, 64, dx, jitter=0.2, seed=50 + k) + (np.asarray(lo) * dx).astype(np.float32)
        states.append(make_state(x, mat, dx, perturb_F=0.02, seed=60 + k))
    s = orc.State(np.concatenate([a.x for a in states]), np.concatenate([a.v for a in states]), np.concatenate([a.B for a in states]),
                  np.concatenate([a.F for a in states]), np.concatenate([a.aux for a in states]),
                  np.concatenate([np.full(a.n, i, np.int32) for i, a in enumerate(states)]),
                  np.stack([a.gparams[0] for a in states]), np.array([a.gtype[0] for a in states], np.int32))
    shapes = [(0, 0, 0, 1, 0, -0.1)]
    r = ref.Sim(res, dx, 1e-4, shapes=shapes, friction=-1.0)
    for i, a in enumerate(states):
        r.add_particles(("water", "elastic")[i], a.gparams[0][0], a.gparams[0][1], a.x, a.v, a.F, a.B, a.aux)
    r.substep(1)
    sim = hip_sim(tm, res, dx, 1e-4, levelset=levelset_of(tm, shapes, -1.0))
    add_state(sim, tm, s)
    sim.substep()
    a, b = sim.get_particles(), r.download()
    sim.close(); r.close()
    assert np.array_equal(a["id"], b["id"]) and len(a["x"]) == s.n
    assert np.abs(a["x"] - b["x"]).max() <= 2e-7
    assert rel_l2(a["v"], b["v"]) <= 2e-5
    el = a["gid"] == 1
    assert rel_l2(a["F"][el], b["F"][el]) <= 2e-5
    assert np.abs(a["aux"] - b["aux"]).max() <= 2e-5 * max(1.0, np.abs(b["aux"]).max())
