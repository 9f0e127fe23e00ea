"""Sampled signed-distance level sets on the GPU (include/mpmhip.h: mpmhip_set_levelset_sdf; run with -m gpu on an MI355X):
the device sampler against its numpy model (tests/sdf_model.py), baked planes and spheres against the REFERENCE's fixture
(tests/golden/ref_shapes.npz), a baked container against the analytic one, a torus — a shape no mpmhip_shape expresses —, and the
bitwise guarantees of the deterministic mode with a sampled set installed."""
import json

import numpy as np
import pytest

from tests.common import lattice_cube, load_golden, make_state, rel_l2
from tests.sdf_model import SdfModel, sampler_points, well_conditioned

pytestmark = pytest.mark.gpu
FIELDS = ("x", "v", "F", "aux")


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


def _sim(tm, res, dx, dt, **cfg):
    return tm.create_simulation3("mpm").initialize(dict(res=(res,) * 3, delta_x=dx, base_delta_t=dt, **cfg))


def _torus(c, R, r):
    """closed-form SDF of a torus around the y axis through c: major radius R, tube radius r"""
    c = np.asarray(c, np.float64)

    def f(x):
        d = x - c
        return np.hypot(np.hypot(d[:, 0], d[:, 2]) - R, d[:, 1]) - r
    return f


# ------------------------------------------------------------------------------------------ 5: the sampler against the model
DX5 = 1.0 / 32
RES5, ORG5, H5 = (40, 36, 33), (-0.1, 0.02, -0.05), 0.03


def _fields():
    plane = lambda n, d: (lambda x: x @ np.asarray(n, np.float64) + d)
    sphere = lambda c, r: (lambda x: np.linalg.norm(x - np.asarray(c, np.float64), axis=1) - r)
    return {"plane": (plane((0.6, 0.8, 0.0), -0.4), plane((0.6, 0.8, 0.0), -0.43)),
            "sphere": (sphere((0.4, 0.5, 0.4), 0.3), sphere((0.42, 0.5, 0.39), 0.33)),
            "torus": (_torus((0.45, 0.5, 0.4), 0.3, 0.12), _torus((0.45, 0.52, 0.4), 0.31, 0.13))}


@pytest.mark.parametrize("shape", ["plane", "sphere", "torus"])
def test_device_sampler_matches_the_model(tm, shape):
    """mpmhip_debug_levelset_sample at 10^5 points (inside cells, on cell faces, on samples, outside, a NaN), static and at three
    times between two key frames.

    Both sides evaluate the same expressions in fp32 in the same order, every operation rounded on its own (tests/sdf_model.py; the
    device's sampler forbids the contraction of a multiply and an add, csrc/mpm_math.h: SDF_NO_CONTRACT, and its division and square
    root are correctly rounded).  So `hit`, phi and dphidt are equal bit for bit at every point, and the normal wherever it is well
    conditioned.  The bounds a sampler that did contract would meet stay asserted beside that; they say how far a failure is off:
      phi     a fused interpolation (1 - f) a + f b removes ONE rounding of at most half an ulp of the largest magnitude involved,
              and nothing is amplified on the way up (convex combinations).  7 interpolations per frame: <= 7 * 2^-24 M, M = max |phi|
              over the cell's samples; two frames and their blend: <= 15 * 2^-24 M.  Asserted: 2^-20 M = 16 * 2^-24 M.
      dphidt  (phi1 - phi0) / (t1 - t0) of two values that are each within 7 * 2^-24 M: 2^-20 M / (t1 - t0).
      normal  the eight samples' gradients are differences and products.  7 interpolations: the raw gradient within 7 * 2^-24 G per
              component, G = the largest component among the cell's samples; its squared length 2^-24 relative.  A unit vector
              g / |g| moves by at most (component error + length error) / |g| = 15 * 2^-24 G / |g|; where G / |g| <= 2 that is
              30 * 2^-24.  Two frames: the blend of two such normals normalised again, at most (2 * 30 + 2) / |blend| * 2^-24 with
              |blend| >= 0.97 here: 2^-18 = 64 * 2^-24, asserted for both.  Where G / |g| > 2 (the centre line of a tube, the centre
              of a sphere) the direction is ill-conditioned: there the normal must be a unit vector or zero."""
    f0, f1 = _fields()[shape]
    s0 = tm.SampledLevelSet.from_function(f0, RES5, ORG5, H5, friction=0.3)
    s1 = tm.SampledLevelSet.from_function(f1, RES5, ORG5, H5, friction=0.3)
    x = sampler_points(np.random.default_rng(11), 100000, RES5, ORG5, H5)
    sim = _sim(tm, 32, DX5, 1e-4)
    t0, t1 = 0.5, 2.0
    for times in ((None,), (0.7, 1.25, 1.9)):
        if times[0] is None:
            sim.set_levelset(s0)
            model = SdfModel(s0.phi, ORG5, H5, DX5)
        else:
            sim.set_levelset(tm.DynamicLevelSet().initialize(t0, t1, s0, s1))
            model = SdfModel(s0.phi, ORG5, H5, DX5, s1.phi, t0, t1)
        hit_m, c, f = model.locate(x)
        M = model.cell_max_abs(c)
        for t in times:
            phi, g, dphidt, hit = sim.sample_levelset(x, 0.0 if t is None else t)
            mphi, mg, mdphidt, _ = model.sample(x, 0.0 if t is None else t)
            assert np.array_equal(hit, hit_m) and 0.4 < hit.mean() < 0.97
            assert not phi[~hit].any() and not g[~hit].any() and not dphidt[~hit].any()
            h = hit
            worst = (np.abs(phi - mphi)[h] / (2.0 ** -20 * M[h])).max()
            print("%s t=%s: |dphi| / (2^-20 M) <= %.3f, %d of %d hits differ in a bit" % (shape, t, worst, (phi != mphi)[h].sum(), h.sum()))
            assert worst <= 1.0
            if t is None:
                assert not dphidt.any()
            else:
                assert np.all(np.abs(dphidt - mdphidt)[h] <= 2.0 ** -20 * M[h] / (t1 - t0))
            _, well = well_conditioned(model, x, t)
            assert well.sum() > 0.9 * h.sum()
            worst = np.abs(g - mg)[well].max() / 2.0 ** -18
            print("%s t=%s: |dn| / 2^-18 <= %.3f over %d of %d points" % (shape, t, worst, well.sum(), h.sum()))
            assert worst <= 1.0
            ln = np.linalg.norm(g[h], axis=1)
            assert np.all((np.abs(ln - 1) < 1e-5) | (ln == 0))
            assert np.array_equal(phi[h], mphi[h]) and np.array_equal(dphidt[h], mdphidt[h])  # the bits
            assert np.array_equal(g[well], mg[well])
    # the same entry evaluates analytic shapes
    sim.set_levelset(tm.LevelSet(friction=0.3).add_sphere((0.4, 0.5, 0.4), 0.3))
    phi, g, _, hit = sim.sample_levelset(x[:1000])
    ok = np.isfinite(x[:1000]).all(1)
    assert hit[ok].all()
    d = np.linalg.norm(x[:1000].astype(np.float64) - (0.4, 0.5, 0.4), axis=1)
    assert np.abs(phi - (d - 0.3) / DX5)[ok].max() < 1e-4
    sim.close()


def test_argument_checks(tm):
    import ctypes as C
    from taichi_mpm_amd import _lib
    sim = _sim(tm, 32, DX5, 1e-4)
    sim._ensure_ctx()
    L, fp = sim._L, C.POINTER(C.c_float)
    phi = np.zeros((4, 4, 4), np.float32)
    p = phi.ctypes.data_as(fp)

    def desc(res=(4, 4, 4), origin=(0, 0, 0), spacing=0.1):
        d = _lib.SdfDesc()
        d.res[:] = res
        d.origin[:] = origin
        d.spacing = spacing
        return C.byref(d)
    EINVAL = L.mpmhip_set_levelset_sdf(sim._ctx, None, p, None, 0, 1, 0.0)
    assert EINVAL < 0
    for bad in (desc(res=(4, 1, 4)), desc(spacing=0.0), desc(spacing=-1.0), desc(origin=(0, float("inf"), 0)), desc(spacing=float("nan"))):
        assert L.mpmhip_set_levelset_sdf(sim._ctx, bad, p, None, 0, 1, 0.0) == EINVAL
        assert len(L.mpmhip_last_error(sim._ctx)) > 0
    assert L.mpmhip_set_levelset_sdf(sim._ctx, desc(), p, p, 1.0, 1.0, 0.0) == EINVAL
    assert L.mpmhip_set_levelset_sdf(sim._ctx, desc(), None, None, 0, 1, 0.0) == EINVAL
    assert L.mpmhip_set_levelset_sdf(sim._ctx, desc(), p, p, 0.0, 1.0, 0.0) == 0
    # rigid_body_levelset_collision and a sampled set: refused, naming the combination
    assert L.mpmhip_set_rigid_levelset_collision(sim._ctx, 1) == EINVAL
    assert b"sampled" in L.mpmhip_last_error(sim._ctx)
    sim.set_levelset(tm.LevelSet().add_plane((0, 1, 0), d=-0.3))
    assert L.mpmhip_set_rigid_levelset_collision(sim._ctx, 1) == 0
    assert L.mpmhip_set_levelset_sdf(sim._ctx, desc(), p, None, 0, 1, 0.0) == EINVAL
    assert b"sampled" in L.mpmhip_last_error(sim._ctx)
    sim.close()


# ------------------------------------------------------------------------------------------ 6, 7: against the reference's fixture
def _levelset_of(tm, rows, friction, dx):
    from tests.test_gpu_ref import levelset_of
    ls = levelset_of(tm, rows, friction)
    ls.delta_x = dx
    return ls


def _run_case(tm, case, res_l, origin, spacing):
    """test_gpu_ref.py's level-set cases with the shapes baked into a sampled set; returns (got, want, ids)"""
    g = load_golden("ref_shapes")
    c = json.loads(str(g["cases"]))[case]
    res, dx, dt = int(g["res"]), float(g["dx"]), float(g["dt"])
    a = g["in_jelly"]
    sim = _sim(tm, res, dx, dt, **c["cfg"])
    bake = lambda rows: tm.SampledLevelSet.from_levelset(_levelset_of(tm, rows, c["friction"], dx), (res_l,) * 3, origin, spacing)
    if c.get("shapes1") is not None:
        sim.set_levelset(tm.DynamicLevelSet().initialize(0.0, c["t1"], bake(c["shapes"]), bake(c["shapes1"])))
    else:
        sim.set_levelset(bake(c["shapes"]))
    sim.add_particles(dict(type="jelly", positions=a[:, 0:3], velocities=a[:, 3:6], B=a[:, 6:15], F=a[:, 15:24], aux=a[:, 24],
                           params=g["gp_jelly"]))
    for _ in range(3):
        sim.substep()
    got = sim.get_particles()
    sim.close()
    key = "%s_jelly_%s" % (case, "gen" if "damping" in case else "opt")
    return got, g[key], g[key + "_ids"]


@pytest.mark.parametrize("case,lattice", [("moving_plane", "grid"), ("grid_gravity", "grid"), ("apic_damping_only", "grid"),
                                          ("moving_plane", "fine")])
def test_baked_planes_meet_the_reference_fixture(tm, case, lattice):
    """a plane's phi is linear, so the sampled set reproduces it: the reference's fixture must be met with the tolerances of the analytic
    path (tests/test_gpu_ref.py).  'grid': 33^3 samples on the simulation's own nodes (the one-load path of the grid pass); 'fine':
    spacing dx / 2 and a shifted origin (the interpolating path)."""
    dx = 1.0 / 32
    got, want, ids = _run_case(tm, case, 33, (0, 0, 0), dx) if lattice == "grid" else \
        _run_case(tm, case, 70, (-0.011, -0.007, -0.013), dx / 2)
    assert np.array_equal(got["id"], ids)
    ex, ev, eF = np.abs(got["x"] - want[:, 0:3]).max(), rel_l2(got["v"], want[:, 3:6]), rel_l2(got["F"], want[:, 6:15])
    print("%s / %s: max |dx| %.3g, rel-L2 v %.3g, F %.3g" % (case, lattice, ex, ev, eF))
    assert ex <= 5e-7
    assert ev <= 5e-5 and eF <= 2e-4


@pytest.mark.parametrize("case", ["slip_sphere", "particle_collision"])
def test_baked_sphere_converges_to_the_reference_fixture(tm, case):
    """the sphere (and plane) baked at spacing dx, dx / 2, dx / 4: the error against the reference's fixture falls from each spacing
    to the next until it is inside the fixture's own tolerance, and stays inside from there on.  The three errors per case are
    recorded in DESIGN.md."""
    dx = 1.0 / 32
    errs = []
    for k in (1, 2, 4):
        got, want, ids = _run_case(tm, case, 32 * k + 1, (0, 0, 0), dx / k)
        assert np.array_equal(got["id"], ids)
        errs.append((rel_l2(got["v"], want[:, 3:6]), float(np.abs(got["x"] - want[:, 0:3]).max())))
        print("%s spacing dx/%d: rel-L2 v %.3g, max |dx| %.3g" % (case, k, errs[-1][0], errs[-1][1]))
    for m, tol in ((0, 5e-5), (1, 5e-7)):
        e = [q[m] for q in errs]
        for i in range(2):
            if e[i] <= tol:
                assert e[i + 1] <= tol, (case, m, e)
            else:
                assert e[i + 1] < e[i], (case, m, e)


# ------------------------------------------------------------------------------------------ 8: container
def test_sampled_container_keeps_particles_like_the_analytic_one(tm):
    """the scene of tests/test_levelset_cpu.py (water block thrown into the corner of a slip container, particle_collision) in the
    analytic box and in the same box baked at spacing dx.  The sampled run's largest excursion beyond the true box is bounded by the
    analytic run's own plus the largest one-step projection residual of this array (tests/sdf_model.py: projection_residual); the
    interpolated phi of a container never exceeds the true one (tests/test_sdf_cpu.py), so no interpolation term is added."""
    res, dx = 32, 1.0 / 32
    x = lattice_cube(res, 10, 16, dx, jitter=0.2, seed=3)
    s = make_state(x, "water", dx, vel_scale=0.0)
    s.v[:] = (3.0, -2.0, 0.0)
    box = tm.LevelSet(friction=-2.0, delta_x=dx).add_cuboid((0.3,) * 3, (0.6,) * 3, True)
    baked = tm.SampledLevelSet.from_levelset(box, (33,) * 3)
    exc = {}
    for name, ls in (("analytic", box), ("sampled", baked)):
        sim = _sim(tm, res, dx, 2e-4, particle_collision=True)
        sim.set_levelset(ls)
        sim.add_particles(dict(type="water", positions=s.x, velocities=s.v, F=s.F, B=s.B, aux=s.aux, params=s.gparams[0]))
        worst = 0.0
        for _ in range(40):
            sim.substep()
            p = sim.get_particles()
            assert len(p["x"]) == len(x) and np.isfinite(p["x"]).all(), name
            worst = max(worst, float(max(0.3 - p["x"].min(), p["x"].max() - 0.6, 0.0)))
        exc[name] = worst
        sim.close()
    model = SdfModel(baked.phi, baked.origin, baked.spacing, dx)
    probe = np.random.default_rng(8).uniform(0.26, 0.64, (400000, 3)).astype(np.float32)
    residual = model.projection_residual(probe, dx) * dx
    print("container: excursion analytic %.3g, sampled %.3g, one-step projection residual %.3g (world units)" % (exc["analytic"], exc["sampled"], residual))
    assert exc["sampled"] <= exc["analytic"] + residual


# ------------------------------------------------------------------------------------------ 9, 10, 11: a torus
RES9, DX9, DT9 = 64, 1.0 / 64, 1e-4
TORUS_C, TORUS_R, TUBE_R = (0.5, 0.4, 0.5), 0.18, 0.07  # tube radius 4.5 cells


def _torus_set(tm, friction=0.4):
    return tm.SampledLevelSet.from_function(_torus(TORUS_C, TORUS_R, TUBE_R), (RES9 + 1,) * 3, (0, 0, 0), DX9, friction)


def _sand(seed=0):
    """12^3 cells of sand whose lowest layer starts one cell above the tube's top, moving down at 2 m/s"""
    x = lattice_cube(RES9, 0, 12, DX9, jitter=0.2, seed=91)
    x += (np.array([TORUS_C[0] + TORUS_R, TORUS_C[1] + TUBE_R + DX9, TORUS_C[2]]) - (6 * DX9, 0, 6 * DX9)).astype(np.float32)
    s = make_state(x, "sand", DX9, perturb_F=0.0, seed=92, vel_scale=0.0)
    s.v[:] = (0.0, -2.0, 0.0)
    return s


def _drop(tm, s, ls, steps, order=None, ids=None, **cfg):
    from taichi_mpm_amd.mpm import F_ID
    sim = _sim(tm, RES9, DX9, DT9, particle_collision=True, **cfg)
    sim.set_levelset(ls)
    o = np.arange(s.n) if order is None else order
    sim.add_particles(dict(type="sand", positions=s.x[o], velocities=s.v[o], F=s.F[o], B=s.B[o], aux=s.aux[o], params=s.gparams[0]))
    if order is not None:
        sim.upload(F_ID, o.astype(np.int32))
    sim.run_substeps(steps)
    return sim


def test_sand_on_a_torus(tm):
    """sand dropped on a torus given as a closed-form SDF through from_function: nothing is lost, nothing is NaN, and the device-sampled
    phi at every final position is >= -0.5 cells — a cap on gross failure (tunnelling through a 9-cell solid shows as phi << -0.5), not
    an accuracy claim.  The analytic analogue, a sphere of the tube's radius under the same block, is run beside it and held to the
    same cap (its figure is printed, and recorded in DESIGN.md)."""
    s = _sand()
    sim = _drop(tm, s, _torus_set(tm), 300)
    p = sim.get_particles()
    assert len(p["x"]) == s.n
    for f in FIELDS:
        assert np.isfinite(p[f]).all(), f
    phi, _, _, hit = sim.sample_levelset(p["x"])
    sim.close()
    assert hit.all()
    assert (phi < 1.0).sum() > 100  # the sand did reach the torus
    ball_c = (TORUS_C[0] + TORUS_R, TORUS_C[1], TORUS_C[2])
    sim = _drop(tm, s, tm.LevelSet(friction=0.4).add_sphere(ball_c, TUBE_R), 300)
    q = sim.get_particles()
    sim.close()
    phi_ball = (np.linalg.norm(q["x"].astype(np.float64) - ball_c, axis=1) - TUBE_R) / DX9
    print("lowest phi after 300 substeps: torus (sampled) %.4f cells, sphere analogue (analytic) %.4f cells" % (phi.min(), phi_ball.min()))
    assert len(q["x"]) == s.n and phi_ball.min() >= -0.5
    assert phi.min() >= -0.5


def _same(a, b, what):
    assert np.array_equal(a["id"], b["id"]), what
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), (what, f, float(np.abs(a[f] - b[f]).max()))


def test_deterministic_mode_is_bitwise_with_a_sampled_set(tm, monkeypatch):
    """two runs, a shuffled upload, and the two walks of the grid pass agree bit for bit on every particle field; and
    delete_particles_inside_level_set removes exactly the particles whose device-sampled phi is negative"""
    s, ls = _sand(), _torus_set(tm)

    def run(order=None):
        sim = _drop(tm, s, ls, 120, order=order, deterministic=True)
        out = sim.get_particles()
        sim.close()
        return out
    ref = run()
    assert np.abs(ref["v"][:, 1] - (-2.0 - 10.0 * 120 * DT9)).max() > 0.05  # not free fall any more: the torus acts on the sand
    _same(run(), ref, "second run")
    _same(run(np.random.default_rng(5).permutation(s.n)), ref, "shuffled upload")
    for walk in ("0", "2"):
        monkeypatch.setenv("MPMHIP_GRID_WALK", walk)
        _same(run(), ref, "MPMHIP_GRID_WALK=" + walk)
    monkeypatch.delenv("MPMHIP_GRID_WALK")
    # delete_particles_inside_level_set: move the torus up into the sand, then delete
    sim = _drop(tm, s, ls, 20, deterministic=True)
    up = tm.SampledLevelSet.from_function(_torus((TORUS_C[0], TORUS_C[1] + 4 * DX9, TORUS_C[2]), TORUS_R, TUBE_R), (RES9 + 1,) * 3,
                                          (0, 0, 0), DX9, 0.4)
    sim.set_levelset(up)
    before = sim.get_particles()
    phi, _, _, hit = sim.sample_levelset(before["x"])
    inside = hit & (phi < 0)
    assert 100 < inside.sum() < s.n
    import ctypes as C
    n_del = C.c_int64(0)
    sim._check(sim._L.mpmhip_delete_particles_inside_level_set(sim._ctx, C.byref(n_del)))
    after = sim.get_particles()
    assert n_del.value == inside.sum()
    assert np.array_equal(after["id"], before["id"][~inside])
    sim.run_substeps(3)
    assert len(sim.get_particles()["x"]) == len(after["id"])
    sim.close()


def test_replacing_a_sampled_set_by_shapes_and_back_leaves_nothing_behind(tm):
    """sampled -> shapes -> sampled on one ctx: each run equals the run of a fresh ctx with that level set, bit for bit"""
    s = _sand()
    torus = _torus_set(tm)
    ball = tm.LevelSet(friction=0.4).add_sphere((TORUS_C[0] + TORUS_R, TORUS_C[1], TORUS_C[2]), TUBE_R)

    def fresh(ls):
        sim = _drop(tm, s, ls, 60, deterministic=True)
        out = sim.get_particles()
        sim.close()
        return out
    want = {"torus": fresh(torus), "ball": fresh(ball)}
    assert not np.array_equal(want["torus"]["x"], want["ball"]["x"])
    from taichi_mpm_amd.mpm import F_AUX, F_B, F_F, F_V, F_X
    sim = _drop(tm, s, torus, 60, deterministic=True)
    _same(sim.get_particles(), want["torus"], "first")
    for name, ls in (("ball", ball), ("torus", torus), ("ball", ball)):
        sim.set_levelset(ls)
        slots = sim.get_particles(sort_by_id=False)["id"]  # (uploads go by slot; the ids are the rows of the initial state)
        for fld, arr in ((F_X, s.x), (F_V, s.v), (F_F, s.F), (F_B, s.B), (F_AUX, s.aux)):
            sim.upload(fld, arr[slots])
        sim.run_substeps(60)
        _same(sim.get_particles(), want[name], "after switching to the " + name)
    sim.close()
