"""The 2D sampled level set without a GPU: the numpy model of the sampler (tests/sdf_model.py at D = 2) against closed forms and against
the seeding's sampled region (tests/seed2d_model.py), the Python surface (SampledBoundary2D, from_levelset, the refusals), and the
ctypes mirror of mpmhip2d_sdf_desc.  (The argument checking of mpmhip2d_set_levelset_sdf is exercised through the entry point on
the GPU, tests/test_gpu_sdf2d.py::test_every_refusal.)"""
import ctypes as C

import numpy as np
import pytest

import taichi_mpm_amd as tm
from taichi_mpm_amd import _lib
from taichi_mpm_amd.mpm import DynamicLevelSet, LevelSet, MPMError
from tests.sdf2d_model import H1, ORG1, RES1, T0, T1, TIMES, Sdf2DModel, sampler_fields
from tests.sdf_model import sampler_points, well_conditioned
from tests.seed2d_model import SampledRegion2D, ShapeRegion2D

DX = 1.0 / 64
F = np.float32


@pytest.mark.parametrize("shape", ["line", "disc", "ring"])
def test_the_sampler_tests_fields_are_well_conditioned(shape):
    """what the GPU test excludes from its normal comparison stays under 10 % of the hits, for every field and time it uses"""
    f0, f1 = sampler_fields()[shape]
    p0, p1 = _bake(f0, RES1, ORG1, H1).phi, _bake(f1, RES1, ORG1, H1).phi
    x = sampler_points(np.random.default_rng(11), 20000, RES1, ORG1, H1)
    for model, times in ((Sdf2DModel(p0, ORG1, H1, DX), (None,)), (Sdf2DModel(p0, ORG1, H1, DX, p1, T0, T1), TIMES)):
        for t in times:
            hit, well = well_conditioned(model, x, t)
            assert 0.4 < hit.mean() < 0.97
            print("%s t=%s: %d of %d hits ill-conditioned" % (shape, t, hit.sum() - well.sum(), hit.sum()))
            assert hit.sum() - well.sum() <= 0.1 * hit.sum()


def _bake(f, res, origin, spacing):
    return tm.SampledLevelSet2D.from_function(f, res, origin, spacing)


def test_line_is_reproduced_to_rounding():
    """phi of a line is linear: bilinear interpolation is exact, the gradient is the line's normal"""
    n = np.array([0.6, 0.8])
    s = _bake(lambda x: x @ n - 0.41, (65, 65), (0, 0), DX)
    m = Sdf2DModel(s.phi, s.origin, s.spacing, DX)
    x = np.random.default_rng(1).uniform(0.0, 1.0, (20000, 2)).astype(F)
    phi, g, dphidt, hit = m.sample(x)
    assert hit.all() and not dphidt.any()
    exact = (x.astype(np.float64) @ n - 0.41) / DX
    # the samples are rounded to fp32 (half an ulp of |phi| <= 1), the cell coordinate carries an ulp of u <= 64 (2^-18 of a cell
    # along a unit gradient), the two nested interpolations add at most three roundings each of max |phi| / dx < 64 (2^-18): 8 * 2^-18
    assert np.abs(phi - exact).max() <= 8 * 2.0 ** -18, np.abs(phi - exact).max()
    assert np.abs(g - n[None, :]).max() < 2e-5  # differences of fp32 samples over a spacing: 2^-24 / (1/64) per component
    out = np.array([[1.0001, 0.5], [0.5, -1e-4], [0.5, 2.0], [np.nan, 0.5]], F)
    phi, g, _, hit = m.sample(out)
    assert not hit.any() and not phi.any() and not g.any()
    on = np.array([[0, 0], [1, 1], [0.5, 0.25]], F)  # exactly on samples, the last one included
    phi, _, _, hit = m.sample(on)
    assert hit.all()
    np.testing.assert_allclose(phi, (on.astype(np.float64) @ n - 0.41) / DX, atol=1e-5)


def _disc_errors(res):
    c, r = np.array([0.5, 0.5]), 0.25
    h = 1.0 / (res - 1)
    s = _bake(lambda x: np.linalg.norm(x - c, axis=1) - r, (res, res), (0, 0), h)
    m = Sdf2DModel(s.phi, s.origin, s.spacing, DX)
    rng = np.random.default_rng(res)
    a = rng.uniform(0, 2 * np.pi, 50000)
    d = np.stack([np.cos(a), np.sin(a)], 1)
    x = (c + d * (r - rng.uniform(0.0, 3.0, (len(d), 1)) * h)).astype(F)  # the three cells under the surface
    phi, g, _, hit = m.sample(x)
    assert hit.all()
    xd = x.astype(np.float64)
    dist = np.linalg.norm(xd - c, axis=1)
    # the bilinear bound per cell: h^2 / 8 per axis times the second derivatives of |x - c|, whose sum is 1 / rho in the plane,
    # rho = the smallest distance from the centre over the cell
    lo = np.floor(xd / h) * h
    rho = np.linalg.norm(c - np.clip(c, lo, lo + h), axis=1)
    err_phi = np.abs(phi * DX - (dist - r))
    assert np.all(err_phi <= h * h / (8 * rho) + 1e-7), (err_phi / (h * h / (8 * rho))).max()
    return np.linalg.norm(g - (xd - c) / dist[:, None], axis=1).max(), err_phi.max()


def test_disc_phi_bound_and_second_order_gradient():
    e33, e65, e129 = _disc_errors(33), _disc_errors(65), _disc_errors(129)
    print("disc r = 0.25: gradient error 33^2 %.3g 65^2 %.3g 129^2 %.3g, phi error %.3g %.3g %.3g" % (e33[0], e65[0], e129[0], e33[1], e65[1], e129[1]))
    assert e65[0] <= 0.3 * e33[0], (e33, e65)
    assert e129[0] <= 0.3 * e65[0], (e65, e129)


def test_ring_both_signs_of_curvature_and_two_key_frames():
    """a ring (an annulus: | |x - c| - R | - w): phi within h^2 / (8 rho) + the kink's h of the closed form away from the centre line,
    and two frames blend linearly in time"""
    c, R, w = np.array([0.5, 0.5]), 0.25, 0.06
    ring = lambda R_: (lambda x: np.abs(np.linalg.norm(x - c, axis=1) - R_) - w)
    h = DX / 2
    s0, s1 = _bake(ring(R), (129, 129), (0, 0), h), _bake(ring(R + 0.02), (129, 129), (0, 0), h)
    m = Sdf2DModel(s0.phi, s0.origin, s0.spacing, DX, s1.phi, 1.0, 3.0)
    rng = np.random.default_rng(4)
    a = rng.uniform(0, 2 * np.pi, 20000)
    rad = R + rng.uniform(-0.1, 0.1, len(a))
    x = (c + np.stack([np.cos(a), np.sin(a)], 1) * rad[:, None]).astype(F)
    xd = x.astype(np.float64)
    for t, al in ((1.0, 0.0), (2.0, 0.5), (3.0, 1.0)):
        phi, g, dphidt, hit = m.sample(x, t)
        assert hit.all()
        want0, want1 = ring(R)(xd), ring(R + 0.02)(xd)
        want = (1 - al) * want0 + al * want1
        far = (np.abs(np.linalg.norm(xd - c, axis=1) - R) > 2 * h) & (np.abs(np.linalg.norm(xd - c, axis=1) - R - 0.02) > 2 * h)
        assert np.abs(phi * DX - want)[far].max() <= h * h / (8 * 0.1) + 1e-6
        assert np.abs(phi * DX - want).max() <= h  # across the centre line's kink: first order
        np.testing.assert_allclose(dphidt[far] * DX, ((want1 - want0) / 2.0)[far], atol=2 * h * h / (8 * 0.1) + 1e-5)
        ln = np.linalg.norm(g, axis=1)
        assert np.all((np.abs(ln - 1) < 1e-5) | (ln == 0))


def test_the_sign_is_the_seedings_at_every_point():
    """for one array `phi < 0` of the boundary's sampler and `inside` of the seeding's sampled region decide identically: 10^5 points —
    random ones, points on lattice lines, points exactly on samples, points outside the lattice, near the zero level on purpose"""
    rng = np.random.default_rng(12)
    res, org, h = (53, 47), (-0.013, 0.021), 0.0131
    c = np.array([0.3, 0.33])
    field = lambda x: np.minimum(np.linalg.norm(x - c, axis=1) - 0.17, x @ np.array([0.28, 0.96]) - 0.2)
    s = _bake(field, res, org, h)
    hi = np.array(org) + (np.array(res) - 1) * h
    inside = rng.uniform(org, hi, (40000, 2))
    line = rng.uniform(org, hi, (20000, 2))
    ax = rng.integers(0, 2, len(line))
    line[np.arange(len(line)), ax] = np.array(org)[ax] + rng.integers(0, np.array(res)[ax], len(line)) * h
    on = np.array(org) + np.stack([rng.integers(0, res[k], 10000) for k in range(2)], 1) * h
    a = rng.uniform(0, 2 * np.pi, 20000)  # within 1e-6 of the disc's zero level: where a differing rounding would show
    zero = c + np.stack([np.cos(a), np.sin(a)], 1) * (0.17 + rng.uniform(-1e-6, 1e-6, (len(a), 1)))
    out = rng.uniform(np.array(org) - 0.2, hi + 0.2, (10000, 2))
    x = np.concatenate([inside, line, on, zero, out]).astype(F)
    x[-1] = (np.nan, 0.3)
    assert len(x) == 100000
    for dx in (DX, 1.0 / 3, 7.0):  # (the grid-unit factor must not move the sign)
        got = Sdf2DModel(s.phi, org, h, dx).inside(x)
        want = SampledRegion2D(s.phi, org, h, dx).inside(x)
        assert np.array_equal(got, want)
    assert 0.1 < want.mean() < 0.9
    phi_m = Sdf2DModel(s.phi, org, h, DX).sample(x)
    phi_s, _ = SampledRegion2D(s.phi, org, h, DX).phi(x)
    assert np.array_equal(phi_m[0][phi_m[3]], phi_s[phi_m[3]])  # the same bits, not only the same sign


def test_as_boundary_and_from_levelset():
    reg = tm.SampledLevelSet2D.from_polygon([(0.2, 0.2), (0.8, 0.2), (0.5, 0.7)], (33, 33), (0, 0), 1.0 / 32)
    b = reg.as_boundary(friction=0.3)
    assert isinstance(b, tm.SampledBoundary2D) and b.friction == 0.3
    assert b.phi is reg.phi and b.origin == reg.origin and b.spacing == reg.spacing and b.res == reg.res
    assert reg.as_boundary().friction == -1.0 and b.set_friction(-2.0).friction == -2.0
    assert tm.SampledLevelSet2D(np.zeros((4, 4))).as_boundary(0.1).spacing is None  # resolved when it is installed
    # from_levelset: the shapes read in the plane, baked in float64 — against the fp32 formulas of the device's shapes
    ls = LevelSet(friction=0.4, delta_x=DX)
    ls.add_plane((0, 1, 0), d=-0.37).add_sphere((0.5, 0.33, 0.7), 0.08).add_cuboid((0.2, 0.2, 0.3), (0.8, 0.8, 0.4), True)
    res, org, h = (70, 66), (-0.011, -0.007), DX / 2
    s = tm.SampledLevelSet2D.from_levelset(ls, res, org, h)
    assert s.phi.shape == res and s.spacing == h
    pts = tm.SampledLevelSet2D.lattice_points(res, org, h)
    want = ShapeRegion2D(ls.shapes, 1.0)  # (dx = 1: world units)
    # float64 -> float32 rounding of values up to 0.6 (2^-25 relative) plus the fp32 formulas' own few roundings of the same size
    assert np.abs(s.phi.reshape(-1) - want.phi(pts.astype(F))[0]).max() <= 8 * 2.0 ** -24
    assert tm.SampledLevelSet2D.from_levelset(ls, (65, 65)).spacing == DX  # the LevelSet's own cell size by default
    with pytest.raises(MPMError, match="no shapes"):
        tm.SampledLevelSet2D.from_levelset(LevelSet(), (8, 8), (0, 0), 0.1)


def test_set_levelset_accepts_and_refuses():
    ok = np.zeros((4, 4), F)
    reg = tm.SampledLevelSet2D(ok, (0, 0), 0.1)
    a, analytic = reg.as_boundary(0.2), LevelSet().add_plane((0, 1, 0), d=-0.3)
    sim = tm.create_simulation2("mpm").initialize(dict(res=(64, 64), delta_x=DX))
    with pytest.raises(MPMError, match="region for add_particles"):
        sim.set_levelset(reg)
    sim.set_levelset(a)  # before the ctx exists: kept for its creation
    assert sim._levelset is a and sim._ctx is None
    # two frames: one lattice, one kind
    sim.set_levelset(DynamicLevelSet().initialize(0.0, 1.0, a, tm.SampledBoundary2D(ok + 1, (0, 0), 0.1)))
    for other in (tm.SampledBoundary2D(np.zeros((4, 5), F), (0, 0), 0.1), tm.SampledBoundary2D(ok, (0, 0.1), 0.1),
                  tm.SampledBoundary2D(ok, (0, 0), 0.2)):
        with pytest.raises(MPMError, match="one lattice"):
            DynamicLevelSet().initialize(0.0, 1.0, a, other)
    for l0, l1 in ((a, analytic), (analytic, a)):
        with pytest.raises(MPMError, match="cannot be mixed"):
            DynamicLevelSet().initialize(0.0, 1.0, l0, l1)
    with pytest.raises(MPMError, match="cannot be mixed"):
        DynamicLevelSet().initialize(0.0, 1.0, a, tm.SampledLevelSet(np.zeros((4, 4, 4), F), (0, 0, 0), 0.1))
    d = DynamicLevelSet()
    d.t0, d.t1, d.levelset0, d.levelset1 = 0.0, 1.0, a, analytic  # (set_levelset checks what it is given, however it was built)
    with pytest.raises(MPMError, match="cannot be mixed"):
        sim.set_levelset(d)
    d.levelset1 = reg  # a region is not a key frame
    with pytest.raises(MPMError):
        sim.set_levelset(d)
    sim3 = tm.create_simulation3("mpm").initialize(dict(res=(32,) * 3, delta_x=1.0 / 32))  # a 2D boundary is not for the 3D simulation
    for ls in (a, DynamicLevelSet().initialize(0.0, 1.0, a, tm.SampledBoundary2D(ok + 1, (0, 0), 0.1))):
        with pytest.raises(MPMError, match="bounds the 2D simulation"):
            sim3.set_levelset(ls)
    sim2 = tm.create_simulation2("mpm").initialize(dict(res=(64, 64), delta_x=DX, rigid_body_levelset_collision=True))
    with pytest.raises(MPMError, match="rigid_body_levelset_collision"):
        sim2.set_levelset(a)


def test_ctypes_mirror_and_exports():
    d = _lib.SdfDesc2D()
    assert C.sizeof(d) == 20 and _lib.SdfDesc2D.res.offset == 0 and _lib.SdfDesc2D.origin.offset == 8 and _lib.SdfDesc2D.spacing.offset == 16
    for name in ("mpmhip2d_set_levelset_sdf", "mpmhip2d_delete_particles_inside_level_set", "mpmhip2d_debug_levelset_sample", "mpmhip2d_capacity"):
        assert name in _lib.exported_symbols()
        assert hasattr(tm.load(), name)
    assert "SampledBoundary2D" in tm.__all__
    import re
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpmhip.h")).read()
    assert re.search(r"typedef struct \{\s*int32_t res\[2\];\s*float origin\[2\];\s*float spacing;\s*\} mpmhip2d_sdf_desc;", hdr)
    assert "#define MPMHIP_ABI_VERSION 3" in hdr or tm.load().mpmhip_abi_version() == 3
