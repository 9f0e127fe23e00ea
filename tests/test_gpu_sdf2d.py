"""Sampled signed-distance level sets as boundaries of the 2D solver (include/mpmhip.h: mpmhip2d_set_levelset_sdf; run with -m gpu on
an MI355X): the device sampler against its numpy model (tests/sdf_model.py at D = 2) and against the seeding's sampled region
(tests/seed2d_model.py), baked floors and a baked disc against the REFERENCE's 2D fixture (tests/golden/ref_mpm2d.npz) and against
the analytic path of this library, a baked container, a polygon hopper — a boundary no mpmhip_shape expresses —, the deterministic
mode, the asynchronous stepper and the CPIC coupling over a sampled floor, replacement, deletion, the refusals and the C++ layer.
Unless a test says otherwise the size is the fixture's: res 64, dx 1/64, dt 1e-4, its 1 600 particles, 3 substeps."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests.common import load_golden, rel_l2
from tests.sdf2d_model import H1, ORG1, RES1, T0, T1, TIMES, Sdf2DModel, sampler_fields
from tests.sdf_model import sampler_points, well_conditioned
from tests.seed2d_model import SampledRegion2D, ShapeRegion2D

pytestmark = pytest.mark.gpu
F = np.float32
RES, DX, DT = 64, 1.0 / 64, 1e-4
EINVAL = -1
PFIELDS = ("id", "x", "v", "F", "B", "aux")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP_SRC = os.path.join(ROOT, "tests", "cpp", "sdf2d_host_layer.cpp")
CPP_OUT = os.path.join(ROOT, "tests", "cpp", "_build", "sdf2d_host_layer")


def build_cpp():
    """tests/cpp/sdf2d_host_layer.cpp against include/mpm_amd/mpm2d.h and the library (__graft_entry__.build() calls this too)"""
    from taichi_mpm_amd import _lib
    lib = _lib.build()
    os.makedirs(os.path.dirname(CPP_OUT), exist_ok=True)
    inc = os.path.join(ROOT, "include")
    deps = [CPP_SRC, os.path.join(inc, "mpm_amd", "mpm2d.h"), os.path.join(inc, "mpm_amd", "mpm.h"), os.path.join(inc, "mpmhip.h"), lib]
    if not os.path.exists(CPP_OUT) or any(os.path.getmtime(d) > os.path.getmtime(CPP_OUT) for d in deps):
        libdir = os.path.dirname(lib)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", inc, CPP_SRC, "-o", CPP_OUT,
                               "-L", libdir, "-lmpmhip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib",
                               "-Wl,--allow-shlib-undefined"])
    return CPP_OUT


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


@pytest.fixture(scope="module")
def gold():
    g = load_golden("ref_mpm2d")
    return g, json.loads(str(g["cases"]))


def make_sim(tm, kind="mpm", **cfg):
    return tm.create_simulation2(kind).initialize(dict(dict(res=(RES, RES), delta_x=DX, base_delta_t=DT), **cfg))


def plane_set(tm, d, friction):
    return tm.LevelSet(friction=friction, delta_x=DX).add_plane((0, 1, 0), d=d)


GRID_LATTICE = ((RES + 1, RES + 1), (0.0, 0.0), DX)          # the grid's own nodes
FINE_LATTICE = ((133, 133), (-0.011, -0.007), DX / 2)        # spacing dx / 2, a shifted origin; covers [0, 1]^2


def bake(tm, ls, lattice=GRID_LATTICE):
    return tm.SampledLevelSet2D.from_levelset(ls, *lattice).as_boundary(ls.friction)


def add_fixture_particles(sim, g, mat):
    aux0 = {"snow": 1.0, "water": 1.0, "visco": 1000.0}.get(mat, 0.0)
    sim.add_particles(dict(type=mat, positions=g["x"], velocities=g["v"], F=g["F"], B=g["B"], aux=np.full(len(g["x"]), aux0, F),
                           params=g["gp_" + mat]))


def meets(got, want_x, want_v, want_F, want_B, want_aux, mat, what):
    """the tolerances of tests/test_gpu_mpm2d.py::test_mpm2d_matches_the_reference_fixture"""
    ex, ev = float(np.abs(got["x"] - want_x).max()), rel_l2(got["v"], want_v)
    eF, eB = rel_l2(got["F"], want_F), rel_l2(got["B"], want_B)
    ea = float(np.abs(got["aux"] - want_aux).max())
    print("%s: max |dx| %.3g, rel-L2 v %.3g F %.3g B %.3g, max |daux| %.3g" % (what, ex, ev, eF, eB, ea))
    assert ex <= 5e-7, what
    assert ev <= 5e-5, what
    if mat != "water":
        assert eF <= 1e-4, what
    assert eB <= 2e-4, what
    assert ea <= 5e-5 * max(1.0, np.abs(want_aux).max()), what
    return ex, ev


def meets_fixture(got, want, ids, mat, what):
    assert np.array_equal(got["id"], ids), what
    return meets(got, want[:, 0:2], want[:, 2:4], want[:, 4:8], want[:, 8:12], want[:, 12], mat, what)


def meets_run(got, ref, mat, what):
    assert np.array_equal(got["id"], ref["id"]), what
    return meets(got, ref["x"], ref["v"], ref["F"], ref["B"], ref["aux"], mat, what)


# ------------------------------------------------------------------------------------------ 1: the sampler against the model
@pytest.mark.parametrize("shape", ["line", "disc", "ring"])
def test_device_sampler_matches_the_model(tm, shape):
    """mpmhip2d_debug_levelset_sample at 20 000 points (inside cells, on lattice lines, on samples, outside, a NaN) on a lattice with a
    shifted origin and spacing != dx, static and at three times between two key frames.

    Both sides evaluate the same expressions in fp32 in the same order (tests/sdf_model.py); the cell and the weights come from a
    subtraction and a multiplication that cannot be fused, so they — and `hit` — are identical.  The sampler forbids every fusion
    (csrc/mpm_math.h: SDF_NO_CONTRACT), so phi and dphidt are equal bit for bit at every hit and the normal wherever it is well
    conditioned.  Beside that the bound of tests/test_gpu_sdf.py::test_device_sampler_matches_the_model with the 2D counts stays
    asserted, which says how far a failure is off: a fused interpolation (1 - f) a + f b removes ONE rounding of at most half an ulp
    of the largest magnitude involved; nothing is amplified on the way up (convex combinations).
      phi     3 interpolations per frame: <= 3 * 2^-24 M, M = max |phi| over the cell's samples; two frames and their blend
              (one more fusable add): <= 7 * 2^-24 M.  Asserted: 2^-21 M = 8 * 2^-24 M.
      dphidt  (phi1 - phi0) / (t1 - t0) of two values that are each within 3 * 2^-24 M: 2^-21 M / (t1 - t0).
      normal  the four samples' gradients are differences and products: identical.  3 interpolations: the raw gradient is within
              3 * 2^-24 G per component, G = the largest component among the cell's samples.  Its squared length may fuse one add
              (2^-24 relative on the length).  A unit vector g / |g| moves by at most (component error + length error) / |g|
              = 7 * 2^-24 G / |g|; where G / |g| <= 2 that is 14 * 2^-24.  Two frames: the blend of two such normals (one more fused
              add each way, 2 * 2^-24) normalised again, at most (2 * 14 + 2) / |blend| * 2^-24 with |blend| >= 0.97 here: under
              2^-19 = 32 * 2^-24, asserted for both.  Where G / |g| > 2 (the centre of a disc, the centre line of a ring) the
              direction is ill-conditioned on both sides alike: there the normal must be a unit vector or zero.  Those points are at
              most 10 % of the hits (checked on the CPU: tests/test_sdf2d_cpu.py::test_the_sampler_tests_fields_are_well_conditioned)."""
    f0, f1 = sampler_fields()[shape]
    s0 = tm.SampledLevelSet2D.from_function(f0, RES1, ORG1, H1).as_boundary(0.3)
    s1 = tm.SampledLevelSet2D.from_function(f1, RES1, ORG1, H1).as_boundary(0.3)
    x = sampler_points(np.random.default_rng(11), 20000, RES1, ORG1, H1)
    sim = make_sim(tm)
    for times in ((None,), TIMES):
        if times[0] is None:
            sim.set_levelset(s0)
            model = Sdf2DModel(s0.phi, ORG1, H1, DX)
        else:
            sim.set_levelset(tm.DynamicLevelSet().initialize(T0, T1, s0, s1))
            model = Sdf2DModel(s0.phi, ORG1, H1, DX, s1.phi, T0, T1)
        hit_m, c, f = model.locate(x)
        M = model.cell_max_abs(c)
        for t in times:
            phi, g, dphidt, hit = sim.sample_levelset(x, 0.0 if t is None else t)
            mphi, mg, mdphidt, _ = model.sample(x, 0.0 if t is None else t)
            assert np.array_equal(hit, hit_m) and 0.4 < hit.mean() < 0.97
            assert not phi[~hit].any() and not g[~hit].any() and not dphidt[~hit].any()
            h = hit
            worst = (np.abs(phi - mphi)[h] / (2.0 ** -21 * M[h])).max()
            print("%s t=%s: |dphi| / (2^-21 M) <= %.3f" % (shape, t, worst))
            assert worst <= 1.0
            if t is None:
                assert not dphidt.any()
            else:
                assert np.all(np.abs(dphidt - mdphidt)[h] <= 2.0 ** -21 * M[h] / (T1 - T0))
            _, well = well_conditioned(model, x, t)
            assert h.sum() - well.sum() <= 0.1 * h.sum()
            worst = np.abs(g - mg)[well].max() / 2.0 ** -19
            print("%s t=%s: |dn| / 2^-19 <= %.3f over %d of %d points" % (shape, t, worst, well.sum(), h.sum()))
            assert worst <= 1.0
            ln = np.linalg.norm(g[h], axis=1)
            assert np.all((np.abs(ln - 1) < 1e-5) | (ln == 0))
            assert np.array_equal(phi[h], mphi[h]) and np.array_equal(dphidt[h], mdphidt[h])  # the bits
            assert np.array_equal(g[well], mg[well])
    # the same entry evaluates analytic shapes, read in the plane
    sim.set_levelset(tm.LevelSet(friction=0.3).add_sphere((0.4, 0.5, 0.0), 0.3))
    phi, g, _, hit = sim.sample_levelset(x[:1000])
    ok = np.isfinite(x[:1000]).all(1)
    assert hit[ok].all()
    d = np.linalg.norm(x[:1000].astype(np.float64) - (0.4, 0.5), axis=1)
    assert np.abs(phi - (d - 0.3) / DX)[ok].max() < 1e-4
    sim.close()


# ------------------------------------------------------------------------------------------ 2: one sampler, two users
HOPPER = [(0.14, 0.30), (0.46, 0.30), (0.46, 0.36), (0.20, 0.70), (0.20, 0.84), (0.80, 0.84), (0.80, 0.70), (0.54, 0.36), (0.54, 0.30),
          (0.86, 0.30), (0.86, 0.88), (0.14, 0.88)]  # an arch: two wedges joined above the sand; the outlet is 5 cells wide


def hopper(tm, lattice=GRID_LATTICE):
    return tm.SampledLevelSet2D.from_polygon(HOPPER, *lattice)


def test_boundary_and_seeding_decide_alike(tm):
    """for one array, `phi < 0` of the installed boundary (the device's sampler) equals the seeding model's `inside` at 20 000 points,
    exactly; a polygon region seeded on the device and then deleted with the same field as the boundary leaves no particle, and with
    the field negated leaves all of them"""
    reg = hopper(tm, FINE_LATTICE)
    sim = make_sim(tm)
    sim.set_levelset(reg.as_boundary(0.3))
    rng = np.random.default_rng(3)
    x = rng.uniform(-0.05, 1.05, (20000, 2)).astype(F)
    pts = tm.SampledLevelSet2D.lattice_points(*FINE_LATTICE)  # (points exactly on samples and on lattice lines among them)
    x[:2000] = pts[rng.integers(0, len(pts), 2000)].astype(F)
    x[2000:4000, 0] = pts[rng.integers(0, len(pts), 2000), 0].astype(F)
    phi, _, _, hit = sim.sample_levelset(x)
    want = SampledRegion2D(reg.phi, reg.origin, reg.spacing, DX).inside(x)
    assert np.array_equal(hit & (phi < 0), want) and 0.1 < want.mean() < 0.9
    sim.add_particles(dict(type="sand", region=reg, ppc=4))
    n = sim.get_num_particles()
    assert n > 3000
    neg = tm.SampledBoundary2D(-reg.phi, reg.origin, reg.spacing, 0.3)
    sim.set_levelset(neg)
    assert sim.general_action(dict(action="delete_particles_inside_level_set")) == ""
    assert sim.get_num_particles() == n
    sim.set_levelset(reg.as_boundary(0.3))
    assert sim.general_action(dict(action="delete_particles_inside_level_set")) == ""
    assert sim.get_num_particles() == 0
    sim.close()


# ------------------------------------------------------------------------------------------ 3: linear fields are exact
def _floor_run(tm, g, mat, levelset, deterministic, steps=3):
    sim = make_sim(tm, deterministic=deterministic)
    sim.set_levelset(levelset)
    add_fixture_particles(sim, g, mat)
    sim.run_substeps(steps)
    got, grid = sim.get_particles(), sim.get_grid()
    sim.close()
    return got, grid


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("lattice", ["grid", "fine"])
@pytest.mark.parametrize("mat", ["jelly", "sand", "water"])
def test_baked_floor_meets_the_reference_fixture(tm, gold, mat, lattice, deterministic):
    """a floor's phi is linear, so the sampled set reproduces it.  (a) the fixture's `floor` case with the floor baked meets the
    REFERENCE's fixture with the tolerances of the analytic path, on the grid's own nodes (65^2, spacing dx, origin 0) and at spacing
    dx / 2 with a shifted origin.  The fixture's floor (y = 0.37) lies under the particles' lowest node, so (b) the same with the floor
    raised to y = 0.40, where nodes inside the band carry mass, against the analytic floor on this library — the yardstick the fixture
    checks — with the same tolerances."""
    g, cases = gold
    c = cases["floor"]
    lat = GRID_LATTICE if lattice == "grid" else FINE_LATTICE
    got, _ = _floor_run(tm, g, mat, bake(tm, plane_set(tm, -0.37, c["friction"]), lat), deterministic)
    meets_fixture(got, g["floor_" + mat], g["floor_%s_ids" % mat], mat, "floor 0.37 / %s / %s" % (mat, lattice))
    ls = plane_set(tm, -0.40, c["friction"])
    ref, grid = _floor_run(tm, g, mat, ls, deterministic)
    band = grid[:, :26, 2] > 0  # nodes at y <= 25 dx = 0.39: below the floor and within 3 cells of it
    assert band.sum() > 20
    got, _ = _floor_run(tm, g, mat, bake(tm, ls, lat), deterministic)
    meets_run(got, ref, mat, "floor 0.40 / %s / %s" % (mat, lattice))
    free, _ = _floor_run(tm, g, mat, plane_set(tm, -0.2, c["friction"]), deterministic)
    assert rel_l2(free["v"], ref["v"]) > 1e-3  # the raised floor does act on the particles


def _pc_floor_run(tm, g, mat, levelset, deterministic):
    sim = make_sim(tm, deterministic=deterministic, particle_collision=True)
    sim.set_levelset(levelset)
    add_fixture_particles(sim, g, mat)
    x0 = sim.get_particles()["x"]
    sim.run_substeps(3)
    got = sim.get_particles()
    sim.close()
    return got, x0


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("mat", ["jelly", "sand"])
def test_particle_collision_against_a_baked_floor_is_the_inline_push(tm, gold, mat, deterministic):
    """k2_sdf_collide, the pass behind G2P, against the push g2p_particle carries for shapes: the fixture's particles over a floor at
    y = 0.40 — the lowest row, 40 of them, starts below it — with particle_collision on, baked (both lattices) against analytic, with the
    fixture's tolerances.  Not bitwise: the analytic phi of a plane and the interpolated one differ in the last place, and the push
    moves a particle by phi.  A pass that reflected the normal velocity instead of removing it, or pushed the wrong way, is off by the
    velocity itself (0.7 m/s) or by the depth (0.4 cells)."""
    g, cases = gold
    ls = plane_set(tm, -0.40, cases["floor"]["friction"])
    ref, x0 = _pc_floor_run(tm, g, mat, ls, deterministic)
    below = x0[:, 1] < 0.40
    assert below.sum() >= 40 and ref["x"][:, 1].min() >= 0.40 - 1e-6  # the push did act, and lifted every one of them
    off, _ = _floor_run(tm, g, mat, ls, deterministic)
    assert np.abs(off["x"] - ref["x"]).max() > 1e-3  # (without particle_collision they stay below)
    for name, lat in (("grid", GRID_LATTICE), ("fine", FINE_LATTICE)):
        got, _ = _pc_floor_run(tm, g, mat, bake(tm, ls, lat), deterministic)
        meets_run(got, ref, mat, "particle_collision floor 0.40 / %s / %s" % (mat, name))


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
def test_particle_collision_with_a_cpic_body_over_a_baked_floor(tm, deterministic):
    """the same with a rigid body in the scene, where G2P is k_g2p with the colour test (default) or k2d_g2p (deterministic mode):
    box_sand of tests/cpic_scenes.py over a floor at y = 0.36, which the block's lowest row starts below, particle_collision on, baked
    against analytic with the tolerances tests/test_gpu_cpic.py gives that scene"""
    from tests import cpic_scenes as cs
    name, body, material, n, cfg = [c for c in cs.CASES2 if c[0] == "box_sand"][0]
    floor = tm.LevelSet(friction=0.4, delta_x=cs.DX2).add_plane((0, 1, 0), d=-0.36)
    out = {}
    for which, ls in (("analytic", floor), ("baked", bake(tm, floor))):
        sim, rid = cs.build_device2(tm, body, material, particle_collision=True, deterministic=deterministic, **cfg)
        sim.set_levelset(ls)
        below = int((sim.get_particles()["x"][:, 1] < 0.36).sum())
        sim.run_substeps(n)
        out[which] = (sim.get_particles(), sim.get_rigid_state(rid))
        sim.close()
    (h, b), (r, a) = out["baked"], out["analytic"]
    assert below > 20 and r["x"][:, 1].min() >= 0.36 - 1e-6
    assert np.array_equal(h["id"], r["id"])
    ex, ev, eF = float(np.abs(h["x"] - r["x"]).max()), rel_l2(h["v"], r["v"]), rel_l2(h["F"], r["F"])
    print("cpic box_sand, particle_collision, baked floor (%s): max |dx| %.3g, rel-L2 v %.3g F %.3g" % ("det" if deterministic else "default", ex, ev, eF))
    assert ex <= 5e-6 and ev <= 2e-4 and eF <= 1e-4
    np.testing.assert_allclose(b[0:3], a[0:3], rtol=0, atol=2e-6)
    np.testing.assert_allclose(b[3:5], a[3:5], rtol=0, atol=2e-4 * max(np.abs(a[3:5]).max(), 1e-2))


# ------------------------------------------------------------------------------------------ 4: a moving linear field
@pytest.mark.parametrize("d0", [-0.37, -0.40])
@pytest.mark.parametrize("mat", ["jelly", "sand"])
def test_moving_baked_floor_matches_the_analytic_key_frames(tm, gold, mat, d0):
    """a floor rising from y = 0.37 to 0.375 over 0.01 s (and, so that nodes in the band carry mass, from 0.40 to 0.405) as two baked
    frames against a DynamicLevelSet of planes on this library, with the fixture's tolerances; sticky, so the boundary velocity
    formed from d phi / dt is what the nodes take"""
    g, _ = gold

    def run(l0, l1):
        sim = make_sim(tm)
        sim.set_levelset(tm.DynamicLevelSet().initialize(0.0, 0.01, l0, l1))
        add_fixture_particles(sim, g, mat)
        sim.run_substeps(3)
        out = sim.get_particles()
        sim.close()
        return out
    p0, p1 = plane_set(tm, d0, -1.0), plane_set(tm, d0 - 0.005, -1.0)
    ref = run(p0, p1)
    for name, lat in (("grid", GRID_LATTICE), ("fine", FINE_LATTICE)):
        meets_run(run(bake(tm, p0, lat), bake(tm, p1, lat)), ref, mat, "rising floor %.2f / %s / %s" % (-d0, mat, name))
    if d0 == -0.40:
        still = run(p0, p0)
        assert rel_l2(still["v"], ref["v"]) > 1e-4  # the floor's velocity reaches the particles


# ------------------------------------------------------------------------------------------ 5: a curved field converges
@pytest.mark.parametrize("mat", ["jelly", "sand", "water"])
def test_baked_disc_converges_to_the_reference_fixture(tm, gold, mat):
    """the fixture's disc+rising_floor baked at spacing dx, dx / 2, dx / 4: the error against the REFERENCE's fixture falls from each
    spacing to the next until it is inside the fixture's own tolerance, and stays inside from there on
    (tests/test_gpu_sdf.py::test_baked_sphere_converges_to_the_reference_fixture).  The three errors are printed and recorded in
    DESIGN.md §9."""
    g, cases = gold
    from tests.test_gpu_mpm2d import _levelset
    c = cases["disc+rising_floor"]
    errs = []
    for k in (1, 2, 4):
        lat = ((RES * k + 1,) * 2, (0.0, 0.0), DX / k)
        frames = []
        for rows in (c["shapes"], c["shapes1"]):
            ls = _levelset(tm, rows, c["friction"])
            frames.append(bake(tm, ls, lat))
        sim = make_sim(tm, **c["cfg"])
        sim.set_levelset(tm.DynamicLevelSet().initialize(0.0, c["t1"], *frames))
        add_fixture_particles(sim, g, mat)
        sim.run_substeps(3)
        got = sim.get_particles()
        sim.close()
        want = g["disc+rising_floor_" + mat]
        assert np.array_equal(got["id"], g["disc+rising_floor_%s_ids" % mat])
        errs.append((rel_l2(got["v"], want[:, 2:4]), float(np.abs(got["x"] - want[:, 0:2]).max())))
        print("disc+rising_floor %s spacing dx/%d: rel-L2 v %.3g, max |dx| %.3g" % (mat, k, errs[-1][0], errs[-1][1]))
    for m, tol in ((0, 5e-5), (1, 5e-7)):
        e = [q[m] for q in errs]
        for i in range(2):
            if e[i] <= tol:
                assert e[i + 1] <= tol, (mat, m, e)
            else:
                assert e[i + 1] < e[i], (mat, m, e)


# ------------------------------------------------------------------------------------------ 6: container
def test_sampled_container_keeps_particles_like_the_analytic_one(tm):
    """the 2D form of tests/test_gpu_sdf.py's container: a water block thrown into the corner of an inside-out box, friction -2,
    particle_collision, 40 substeps, in the analytic box and in the same box baked at spacing dx.  The sampled run's largest excursion
    beyond the true box is at most the analytic run's own plus the largest one-step projection residual of this array
    (tests/sdf_model.py: projection_residual); the interpolated phi of a container never exceeds the true one (phi is concave
    inside it), so no interpolation term is added."""
    from taichi_mpm_amd.mpm2d import lattice_square
    x = lattice_square(20, 32, DX) + np.array([7 * DX, 0.0], F)  # x in 0.42 .. 0.61 -> the right wall at 0.6 and the floor at 0.3
    x = x[(x[:, 0] < 0.597) & (x[:, 1] > 0.303)]
    v = np.tile(np.array([3.0, -2.0], F), (len(x), 1))
    box = tm.LevelSet(friction=-2.0, delta_x=DX).add_cuboid((0.3, 0.3, 0.0), (0.6, 0.6, 1.0), True)
    baked = bake(tm, box)
    exc = {}
    for name, ls in (("analytic", box), ("sampled", baked)):
        sim = make_sim(tm, particle_collision=True, base_delta_t=2e-4)
        sim.set_levelset(ls)
        sim.add_particles(dict(type="water", positions=x, velocities=v))
        worst = 0.0
        for _ in range(40):
            sim.substep()
            p = sim.get_particles()
            assert len(p["x"]) == len(x) and np.isfinite(p["x"]).all(), name
            worst = max(worst, float(max(0.3 - p["x"].min(), p["x"].max() - 0.6, 0.0)))
        exc[name] = worst
        # the block did run into the right wall, and the wall held it: free flight would have carried its front 0.024 on, past x = 0.6
        assert x[:, 0].max() + 3.0 * 40 * 2e-4 > 0.6 + 5e-3
        assert 0.6 - DX < p["x"][:, 0].max() <= 0.6 + worst + 1e-7, name
        sim.close()
    model = Sdf2DModel(baked.phi, baked.origin, baked.spacing, DX)
    probe = np.random.default_rng(8).uniform(0.26, 0.64, (400000, 2)).astype(F)
    residual = model.projection_residual(probe, DX) * DX
    print("container: excursion analytic %.3g, sampled %.3g, one-step projection residual %.3g (world units)" % (exc["analytic"], exc["sampled"], residual))
    assert exc["sampled"] <= exc["analytic"] + residual


# ------------------------------------------------------------------------------------------ 7, 8: a polygon hopper
def hopper_scene(tm):
    """sand over the funnel's slopes and throat, moving down at 3 m/s: 4 particles per cell where the hopper's phi is > 0.5 cells"""
    from taichi_mpm_amd.mpm2d import lattice_square
    reg = hopper(tm)
    x = lattice_square(14, 50, DX)
    x = x[(x[:, 1] > 0.33) & (x[:, 1] < 0.62)]
    phi, _, _, hit = Sdf2DModel(reg.phi, reg.origin, reg.spacing, DX).sample(x)
    x = x[hit & (phi > 0.5)]
    vol = DX * DX / 4
    gp, _ = tm.group_params("sand", 400.0 * vol, vol)
    v = np.tile(np.array([0.0, -3.0], F), (len(x), 1))
    return reg, dict(type="sand", positions=x, velocities=v, params=gp)


def test_sand_through_a_polygon_hopper(tm):
    """sand with particle_collision falls through a from_polygon funnel for 200 substeps at res 64: no particle is lost (the domain
    rule deletes within 7 cells of a wall; at 3 m/s nothing gets there in 0.02 s) and none is NaN; after every 20th substep every
    particle's device-sampled phi is >= -(the model's one-step projection residual of this array over the band -1 < phi < 0)"""
    reg, group = hopper_scene(tm)
    n = len(group["positions"])
    assert n > 1000
    model = Sdf2DModel(reg.phi, reg.origin, reg.spacing, DX)
    residual = model.projection_residual(np.random.default_rng(2).uniform(0.1, 0.9, (1000000, 2)).astype(F), DX)
    sim = make_sim(tm, particle_collision=True)
    sim.set_levelset(reg.as_boundary(0.4))
    sim.add_particles(group)
    lowest, touched = 0.0, 0
    for k in range(10):
        sim.run_substeps(20)
        p = sim.get_particles()
        assert len(p["x"]) == n
        for f in ("x", "v", "F", "B", "aux"):
            assert np.isfinite(p[f]).all(), f
        phi, _, _, hit = sim.sample_levelset(p["x"])
        assert hit.all()
        lowest = min(lowest, float(phi.min()))
        touched = max(touched, int((phi < 0.25).sum()))
        assert phi.min() >= -residual, (k, float(phi.min()), residual)
    print("hopper: lowest phi %.4g cells, one-step projection residual %.4g cells, %d particles within 0.25 cells of the walls" % (lowest, residual, touched))
    assert touched > 20  # the sand did reach the walls
    assert p["x"][:, 1].min() < 0.33  # and went down the throat
    sim.close()


def test_hopper_in_the_deterministic_mode_is_bitwise(tm):
    """the hopper scene uploaded in two particle orders with the ids re-uploaded, deterministic=True: the states after 50 substeps
    are equal bit for bit"""
    from tests.test_gpu_deterministic_2d import _run, _same
    reg, group = hopper_scene(tm)
    ls = reg.as_boundary(0.4)
    a = _run(tm, 50, RES, [group], cfg=dict(particle_collision=True), levelset=ls)
    assert np.abs(a["v"][:, 1] - (-3.0 - 10.0 * 50 * DT)).max() > 0.05  # not free fall: the hopper acts on the sand
    _same(a, _run(tm, 50, RES, [group], cfg=dict(particle_collision=True), levelset=ls, seed=21))
    _same(a, _run(tm, 50, RES, [group], cfg=dict(particle_collision=True), levelset=ls))


# ------------------------------------------------------------------------------------------ 9: the asynchronous stepper
def test_async_stepper_over_a_baked_floor(tm):
    """AsyncMPM<2> runs the ordinary substep per advance: one frame (2.5e-3 s) of a soft and a stiff square on a floor through their
    lower rows, baked against analytic, with the fixture's tolerances"""
    from tests.golden.make_golden import mpm2d_state
    vol = DX * DX / 4
    groups = []
    for mat, lo, seed in (("elastic", (16, 24), 3), ("sand", (30, 24), 4)):
        x, v, Fm, B = mpm2d_state(RES, lo=lo, cells=12, seed=seed)
        groups.append((mat, tm.group_params(mat, 400 * vol, vol)[0], x, 0.3 * v, Fm, B))
    floor = plane_set(tm, -0.40, 0.4)  # y = 0.40: a cell and a half inside the squares (y from 0.375)
    out = {}
    for name, ls in (("analytic", floor), ("baked", bake(tm, floor))):
        sim = tm.create_simulation2("async_mpm").initialize(dict(res=(RES, RES), delta_x=DX, unit_delta_t=2e-6, max_units=1024))
        sim.set_levelset(ls)
        for mat, gp, x, v, Fm, B in groups:
            sim.add_particles(dict(type=mat, positions=x, velocities=v, F=Fm, B=B, params=gp))
        sim.step(2.5e-3)
        out[name] = sim.get_pool_particles()
        out[name + "_t"] = (sim.current_t_int, sim.update_counter)
        sim.close()
    assert out["analytic_t"] == out["baked_t"]
    a, b = out["baked"], out["analytic"]
    assert np.array_equal(a["block"], b["block"])
    meets_run(a, b, "mixed", "async floor")


# ------------------------------------------------------------------------------------------ 10: CPIC
def test_cpic_box_in_sand_over_a_baked_floor(tm):
    """box_sand of tests/cpic_scenes.py (a box falling into 2D sand, penalty 1e3).  The scene has no level set of its own; a floor at
    y = 0.36 — one cell inside the block's lowest row — is added to both runs, analytic and baked, and the baked run is held to the
    analytic one with the tolerances tests/test_gpu_cpic.py gives that scene against its fixture.  With
    rigid_body_levelset_collision=True the sampled set is refused, in both orders of the two calls."""
    from tests import cpic_scenes as cs
    name, body, material, n, cfg = [c for c in cs.CASES2 if c[0] == "box_sand"][0]
    floor = tm.LevelSet(friction=0.4, delta_x=cs.DX2).add_plane((0, 1, 0), d=-0.36)
    out = {}
    for which, ls in (("analytic", floor), ("baked", bake(tm, floor))):
        sim, rid = cs.build_device2(tm, body, material, **cfg)
        sim.set_levelset(ls)
        sim.run_substeps(n)
        o = np.argsort(sim.get_particles(sort_by_id=False)["id"], kind="stable")
        out[which] = (sim.get_particles(), sim.download_colours()["states"][o], sim.get_rigid_state(rid))
        sim.close()
    (h, st_h, b), (r, st_r, a) = out["baked"], out["analytic"]
    assert np.array_equal(h["id"], r["id"])
    ex, ev, eF = float(np.abs(h["x"] - r["x"]).max()), rel_l2(h["v"], r["v"]), rel_l2(h["F"], r["F"])
    print("cpic box_sand over a baked floor: max |dx| %.3g, rel-L2 v %.3g F %.3g" % (ex, ev, eF))
    assert ex <= 5e-6 and ev <= 2e-4 and eF <= 1e-4
    assert (st_h != st_r).sum() <= 3
    np.testing.assert_allclose(b[0:3], a[0:3], rtol=0, atol=2e-6)
    np.testing.assert_allclose(b[3:5], a[3:5], rtol=0, atol=2e-4 * max(np.abs(a[3:5]).max(), 1e-2))
    np.testing.assert_allclose(b[5], a[5], rtol=0, atol=2e-4 * max(abs(a[5]), 1e-1))
    sim, _ = cs.build_device2(tm, body, material, **cfg)  # the floor does act: without it the lowest row falls freely
    sim.run_substeps(n)
    assert rel_l2(sim.get_particles()["v"], r["v"]) > 1e-3
    sim.close()
    # refusals, at the Python surface and below it
    sim = make_sim(tm, rigid_body_levelset_collision=True)
    with pytest.raises(tm.MPMError, match="rigid_body_levelset_collision is not supported with a sampled level set"):
        sim.set_levelset(bake(tm, floor))
    sim.close()
    sim = tm.create_simulation2("mpm")
    sim.set_levelset(bake(tm, floor))  # (before initialize: the library refuses when the ctx is made)
    sim.initialize(dict(res=(RES, RES), delta_x=DX, rigid_body_levelset_collision=True))
    with pytest.raises(tm.MPMError, match="rigid_body_levelset_collision is not supported with a sampled level set"):
        sim.substep()
    sim.close()
    sim = make_sim(tm)
    sim.set_levelset(bake(tm, floor))
    sim._ensure_ctx()
    assert sim._L.mpmhip2d_set_rigid_levelset_collision(sim._ctx, 1) == EINVAL
    assert b"sampled" in sim._L.mpmhip2d_last_error(sim._ctx)
    sim.close()


# ------------------------------------------------------------------------------------------ 11: replacement
def test_replacement_frees_and_leaves_nothing_behind(tm, gold, tmp_path):
    """sampled -> shapes -> sampled (the same lattice) -> sampled (another lattice): the live-buffer count returns to its level after
    every replacement by shapes and after destroy, a same-size lattice allocates nothing; and in the deterministic mode the run after
    each replacement equals the run of a fresh ctx with that level set bit for bit (the particles are put back by a snapshot, which
    does not hold the level set)"""
    g, _ = gold
    L = tm.load()
    live = L.mpmhip_debug_live_buffers
    floor = plane_set(tm, -0.40, 0.4)
    disc = tm.LevelSet(friction=0.4, delta_x=DX).add_sphere((0.47, 0.40, 0.0), 0.05)
    A, A2, B = bake(tm, floor), bake(tm, disc), bake(tm, disc, FINE_LATTICE)
    base = live()
    sim = make_sim(tm)
    sim._ensure_ctx()
    level = live()
    for ls, extra in ((A, 1), (floor, 0), (A, 1), (A2, 1), (B, 1), (tm.DynamicLevelSet().initialize(0.0, 1.0, B, B), 2), (B, 1), (tm.DynamicLevelSet().initialize(0.0, 1.0, B, B), 2),
                      (disc, 0), (B, 1)):  # (a static set straight after a dynamic one of its size frees the second frame)
        sim.set_levelset(ls)
        assert live() == level + extra, (type(ls).__name__, live(), level, extra)
    sim.close()
    assert live() == base

    def fresh(ls):
        s = make_sim(tm, deterministic=True)
        s.set_levelset(ls)
        add_fixture_particles(s, g, "sand")
        return s

    def state(s):
        p = s.get_particles()
        return {f: p[f] for f in PFIELDS}
    want = {}
    for name, ls in (("A", A), ("floor", floor), ("A2", A2), ("B", B), ("disc", disc)):
        s = fresh(ls)
        if name == "A":
            snap = str(tmp_path / "start.snap")
            s.save_snapshot(snap)
        s.run_substeps(20)
        want[name] = state(s)
        s.close()
    assert not np.array_equal(want["A"]["v"], want["A2"]["v"]) and not np.array_equal(want["B"]["v"], want["floor"]["v"])
    sim = fresh(A)
    sim.run_substeps(20)
    seq = [("floor", floor), ("A", A), ("A2", A2), ("B", B), ("disc", disc), ("B", B)]
    for name, ls in seq:
        sim.set_levelset(ls)
        sim.load_snapshot(snap)
        sim.run_substeps(20)
        got = state(sim)
        for f in PFIELDS:
            assert np.array_equal(got[f], want[name][f]), (name, f)
    sim.close()
    assert live() == base


# ------------------------------------------------------------------------------------------ 12: deletion
def test_delete_particles_inside_level_set_2d(tm, gold):
    """with shapes, against ShapeRegion2D (no particle of the fixture lies within 1e-4 cells of the shapes' zero level, where a fused
    multiply-add of the device could decide otherwise), and with a sampled set, against the model, which is exact: exactly those ids
    go, the count is returned, general_action returns ''"""
    g, _ = gold
    x = g["x"]
    shapes = tm.LevelSet(friction=0.4, delta_x=DX).add_sphere((0.45, 0.5, 0.0), 0.09).add_plane((0.6, -0.8, 0.0), d=0.05)
    ring = tm.SampledLevelSet2D.from_function(lambda p: np.abs(np.linalg.norm(p - (0.47, 0.55), axis=1) - 0.1) - 0.03, *FINE_LATTICE).as_boundary(0.4)
    shape_model, ring_model = ShapeRegion2D(shapes.shapes, DX), Sdf2DModel(ring.phi, ring.origin, ring.spacing, DX)
    in_r = ring_model.inside(x)
    for name, ls in (("shapes", shapes), ("sampled", ring)):
        sim = make_sim(tm)
        sim.set_levelset(ls)
        add_fixture_particles(sim, g, "sand")
        sim.substep()  # (deleting is not only for fresh uploads)
        before = sim.get_particles()
        if name == "shapes":
            phi_s, inside = shape_model.phi(before["x"])
            assert np.abs(phi_s).min() > 1e-4
        else:
            inside = ring_model.inside(before["x"])
        assert 50 < inside.sum() < len(x) - 50, name
        n_del = C.c_int64(-1)
        sim._check(sim._L.mpmhip2d_delete_particles_inside_level_set(sim._ctx, C.byref(n_del)))
        after = sim.get_particles()
        assert n_del.value == inside.sum(), name
        assert np.array_equal(after["id"], before["id"][~inside]), name
        assert sim.general_action(dict(action="delete_particles_inside_level_set")) == ""
        assert sim.get_num_particles() == len(after["id"])  # nothing more to delete
        sim.run_substeps(3)
        assert sim.get_num_particles() == len(after["id"])
        sim.close()
    # the MPM driver's call over a 2D simulation
    drv = tm.MPM(res=(RES, RES), delta_x=DX, base_delta_t=DT)
    drv.set_levelset(ring)
    drv.add_particles(type="sand", positions=x, velocities=g["v"], params=g["gp_sand"])
    drv.delete_particles_inside_level_set()
    assert drv.c.get_num_particles() == len(x) - in_r.sum()
    drv.c.close()


# ------------------------------------------------------------------------------------------ 13: every refusal
def test_every_refusal(tm):
    from taichi_mpm_amd import _lib
    sim = make_sim(tm)
    sim._ensure_ctx()
    L, fp = sim._L, C.POINTER(C.c_float)
    phi = np.zeros((4, 4), F)
    p = phi.ctypes.data_as(fp)

    def desc(res=(4, 4), origin=(0, 0), spacing=0.1):
        d = _lib.SdfDesc2D()
        d.res[:] = res
        d.origin[:] = origin
        d.spacing = spacing
        return C.byref(d)

    def refused(msg, *args):
        assert L.mpmhip2d_set_levelset_sdf(sim._ctx, *args) == EINVAL, msg
        assert msg.encode() in L.mpmhip2d_last_error(sim._ctx), (msg, L.mpmhip2d_last_error(sim._ctx))
    refused("the lattice description and the first key frame are required", None, p, None, 0, 1, 0.0)
    refused("the lattice description and the first key frame are required", desc(), None, None, 0, 1, 0.0)
    refused("res[1] = 1", desc(res=(4, 1)), p, None, 0, 1, 0.0)
    refused("res[0] = 0", desc(res=(0, 4)), p, None, 0, 1, 0.0)
    refused("origin[1] is not finite", desc(origin=(0, float("inf"))), p, None, 0, 1, 0.0)
    refused("origin[0] is not finite", desc(origin=(float("nan"), 0)), p, None, 0, 1, 0.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused("spacing must be a finite number > 0", desc(spacing=bad), p, None, 0, 1, 0.0)
    refused("more than 2^31 samples", desc(res=(65536, 32769)), p, None, 0, 1, 0.0)
    refused("t0 < t1", desc(), p, p, 1.0, 1.0, 0.0)
    refused("t0 < t1", desc(), p, p, 2.0, 1.0, 0.0)
    assert L.mpmhip2d_set_levelset_sdf(None, desc(), p, None, 0, 1, 0.0) == EINVAL
    assert L.mpmhip2d_set_levelset_sdf(sim._ctx, desc(), p, p, 0.0, 1.0, 0.0) == 0
    # rigid_body_levelset_collision and a sampled set, in either order
    assert L.mpmhip2d_set_rigid_levelset_collision(sim._ctx, 1) == EINVAL
    assert b"rigid_body_levelset_collision is not supported with a sampled level set" in L.mpmhip2d_last_error(sim._ctx)
    sim.set_levelset(tm.LevelSet().add_plane((0, 1, 0), d=-0.3))
    assert L.mpmhip2d_set_rigid_levelset_collision(sim._ctx, 1) == 0
    refused("rigid_body_levelset_collision is not supported with a sampled level set", desc(), p, None, 0, 1, 0.0)
    assert L.mpmhip2d_set_rigid_levelset_collision(sim._ctx, 0) == 0
    # the other entry points
    n = C.c_int64(0)
    assert L.mpmhip2d_delete_particles_inside_level_set(sim._ctx, None) == EINVAL
    assert L.mpmhip2d_delete_particles_inside_level_set(None, C.byref(n)) == EINVAL
    assert L.mpmhip2d_delete_particles_inside_level_set(sim._ctx, C.byref(n)) == 0 and n.value == 0  # no particles
    assert L.mpmhip2d_debug_levelset_sample(sim._ctx, 0, p, 0.0, p, p, p, None) == EINVAL
    assert L.mpmhip_abi_version() == 3
    sim.close()
    # the Python surface
    sim = make_sim(tm)
    with pytest.raises(tm.MPMError, match="region for add_particles"):
        sim.set_levelset(tm.SampledLevelSet2D(phi, (0, 0), 0.1))
    sim._ensure_ctx()
    with pytest.raises(tm.MPMError, match="region for add_particles"):
        sim.set_levelset(tm.SampledLevelSet2D(phi, (0, 0), 0.1))
    sim.set_levelset(tm.SampledLevelSet2D(phi + 1).as_boundary(0.2))  # spacing=None: the simulation's delta_x
    _, _, _, hit = sim.sample_levelset(np.array([[2.9 * DX, 2.9 * DX], [3.1 * DX, 1.0 * DX]], F))
    assert hit.tolist() == [True, False]
    sim.close()


# ------------------------------------------------------------------------------------------ 14: the C++ layer
def test_cpp_host_layer_runs_a_baked_floor_and_deletes(tm, tmp_path):
    """MPM<2>::set_levelset_sdf (one and two frames) and the delete_particles_inside_level_set action of include/mpm_amd/mpm2d.h:
    tests/cpp/sdf2d_host_layer.cpp runs a sand square over a baked floor through the C++ layer and through the C ABI directly and
    compares the two bit for bit; the number it deletes is the model's for the positions it had"""
    floor = bake(tm, plane_set(tm, -0.40, 0.4))
    disc = bake(tm, tm.LevelSet(friction=0.4, delta_x=DX).add_sphere((0.47, 0.45, 0.0), 0.06))
    path = tmp_path / "fields.f32"
    np.concatenate([np.array([floor.origin[0], floor.origin[1], floor.spacing], F), floor.phi.reshape(-1), disc.phi.reshape(-1)]).tofile(path)
    out = tmp_path / "before.f32"
    r = subprocess.run([build_cpp(), str(path), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.split()
    n0, deleted, n1, same = int(f[0]), int(f[1]), int(f[2]), int(f[3])
    assert same == 1 and n1 == n0 - deleted and 0 < deleted < n0, r.stdout
    before = np.fromfile(out, F).reshape(-1, 2)
    assert len(before) == n0 == 4 * 16 * 16
    assert deleted == Sdf2DModel(disc.phi, disc.origin, disc.spacing, DX).inside(before).sum()
