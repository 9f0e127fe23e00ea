"""Sampled level set without a GPU: the numpy model of the sampler (tests/sdf_model.py) against closed forms, and the
validation the Python surface does before anything reaches the device."""
import numpy as np
import pytest

from taichi_mpm_amd.mpm import DynamicLevelSet, LevelSet, MPMError, SampledLevelSet, eval_shapes
from tests.sdf_model import SdfModel

DX = 1.0 / 32


def _model(ls, res, spacing, origin=(0, 0, 0), dx=DX):
    s = SampledLevelSet.from_levelset(ls, (res,) * 3, origin, spacing)
    return s, SdfModel(s.phi, s.origin, s.spacing, dx)


def test_plane_is_reproduced_to_rounding():
    """phi of a plane is linear: trilinear interpolation is exact, the gradient is the plane's normal"""
    n = np.array([0.36, 0.8, -0.48])
    ls = LevelSet(delta_x=DX).add_plane(n, d=-0.31)
    s, m = _model(ls, 33, DX)
    x = np.random.default_rng(1).uniform(0.0, 1.0, (20000, 3)).astype(np.float32)
    phi, g, dphidt, hit = m.sample(x)
    assert hit.all() and not dphidt.any()
    exact = (x.astype(np.float64) @ n - 0.31) / DX
    # the samples are rounded to fp32 (half an ulp of |phi| <= 1.3), the cell coordinate carries an ulp of u <= 32 (2^-19 of a cell
    # along a unit gradient), the three nested interpolations add at most three ulps of max |phi| / dx < 64: 2^-19 + 4 * 2^-18
    assert np.abs(phi - exact).max() <= 2.0 ** -19 + 4 * 2.0 ** -18, np.abs(phi - exact).max()
    assert np.abs(g - n[None, :]).max() < 2e-5  # differences of fp32 samples over a spacing: 2^-24 * 1.3 / (1/32) per component
    # outside the lattice on any axis: no level set
    out = np.array([[1.0001, 0.5, 0.5], [0.5, -1e-4, 0.5], [0.5, 0.5, 2.0], [np.nan, 0.5, 0.5]], np.float32)
    phi, g, _, hit = m.sample(out)
    assert not hit.any() and not phi.any() and not g.any()
    # exactly on samples, last one included
    on = np.array([[0, 0, 0], [1, 1, 1], [0.5, 1.0, 0.25]], np.float32)
    phi, _, _, hit = m.sample(on)
    assert hit.all()
    np.testing.assert_allclose(phi, (on.astype(np.float64) @ n - 0.31) / DX, atol=1e-5)


def _sphere_errors(res):
    c, r = np.array([0.5, 0.5, 0.5]), 0.25  # radius 8 samples on the 33^3 lattice
    h = 1.0 / (res - 1)
    ls = LevelSet(delta_x=DX).add_sphere(c, r)
    s, m = _model(ls, res, h)
    rng = np.random.default_rng(res)
    d = rng.normal(size=(100000, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    x = (c + d * (r - rng.uniform(0.0, 3.0, (len(d), 1)) * h)).astype(np.float32)  # the three cells under the surface
    phi, g, _, hit = m.sample(x)
    assert hit.all()
    xd = x.astype(np.float64)
    dist = np.linalg.norm(xd - c, axis=1)
    # the trilinear bound per cell: h^2 / 8 per axis times the second derivatives of |x - c|, whose sum is 2 / rho,
    # rho = the smallest distance from the centre over the cell
    lo = np.floor(xd / h) * h
    rho = np.linalg.norm(c - np.clip(c, lo, lo + h), axis=1)
    err_phi = np.abs(phi * DX - (dist - r))
    assert np.all(err_phi <= h * h / (4 * rho) + 1e-7), (err_phi / (h * h / (4 * rho))).max()
    return np.linalg.norm(g - (xd - c) / dist[:, None], axis=1).max(), err_phi.max()


def test_sphere_phi_bound_and_second_order_gradient():
    e33, e65, e129 = _sphere_errors(33), _sphere_errors(65), _sphere_errors(129)
    print("sphere r = 0.25: gradient error 33^3 %.3g 65^3 %.3g 129^3 %.3g, phi error %.3g %.3g %.3g" % (e33[0], e65[0], e129[0], e33[1], e65[1], e129[1]))
    assert e65[0] <= 0.3 * e33[0], (e33, e65)
    assert e129[0] <= 0.3 * e65[0], (e65, e129)


def test_sampled_container_is_conservative():
    """inside a container phi is concave (a minimum of linear functions), so its trilinear interpolant lies below it:
    interpolated phi >= -eps implies true phi >= -eps"""
    ls = LevelSet(delta_x=DX).add_cuboid((0.3,) * 3, (0.6,) * 3, True)
    s, m = _model(ls, 33, DX)
    x = np.random.default_rng(3).uniform(0.3, 0.6, (200000, 3)).astype(np.float32)
    phi, _, _, hit = m.sample(x)
    true = eval_shapes(ls.shapes, x) / DX
    assert hit.all()
    gap = true - phi
    print("container 0.3..0.6 on 33^3: true - interpolated phi in [%.3g, %.3g] cells" % (gap.min(), gap.max()))
    assert gap.min() >= -1e-4  # rounding of fp32 samples and interpolation weights, phi up to 5 cells
    assert gap.max() < 1.0


def test_key_frames_blend():
    l0 = LevelSet(delta_x=DX).add_plane((0, 1, 0), d=-0.3)
    l1 = LevelSet(delta_x=DX).add_plane((0, 1, 0), d=-0.4)
    s0 = SampledLevelSet.from_levelset(l0, (33,) * 3)
    s1 = SampledLevelSet.from_levelset(l1, (33,) * 3)
    m = SdfModel(s0.phi, s0.origin, s0.spacing, DX, s1.phi, 1.0, 3.0)
    x = np.random.default_rng(5).uniform(0.05, 0.95, (1000, 3)).astype(np.float32)
    phi, g, dphidt, hit = m.sample(x, 1.5)
    assert hit.all()
    np.testing.assert_allclose(phi, (x[:, 1] - 0.325) / DX, atol=2e-5)
    np.testing.assert_allclose(dphidt, np.full(len(x), -0.1 / DX / 2.0), rtol=1e-4)
    np.testing.assert_allclose(g, np.tile([0, 1, 0], (len(x), 1)), atol=1e-5)


def test_python_validation():
    ok = np.zeros((4, 4, 4), np.float32)
    with pytest.raises(MPMError):
        SampledLevelSet(np.zeros((4, 4)))
    with pytest.raises(MPMError):
        SampledLevelSet(np.zeros((4, 4, 4, 1)))
    with pytest.raises(MPMError):
        SampledLevelSet(np.zeros((4, 1, 4)))
    bad = ok.copy()
    bad[1, 2, 3] = np.nan
    with pytest.raises(MPMError):
        SampledLevelSet(bad)
    bad[1, 2, 3] = np.inf
    with pytest.raises(MPMError):
        SampledLevelSet(bad)
    with pytest.raises(MPMError):
        SampledLevelSet(ok, spacing=0.0)
    with pytest.raises(MPMError):
        SampledLevelSet(ok, spacing=-1.0)
    with pytest.raises(MPMError):
        SampledLevelSet(ok, origin=(0.0, np.inf, 0.0))
    with pytest.raises(MPMError):
        SampledLevelSet(ok, origin=(0.0, 0.0))
    with pytest.raises(MPMError):
        SampledLevelSet(ok).get_delta_x()
    with pytest.raises(MPMError):
        SampledLevelSet.from_function(lambda x: x[:, 0], (4, 4, 4), spacing=None)
    with pytest.raises(MPMError):
        SampledLevelSet.from_function(lambda x: x[:, 0], (4, 4), spacing=0.1)
    a = SampledLevelSet(ok, (0, 0, 0), 0.1)
    assert a.get_delta_x() == 0.1 and a.set_friction(0.3).friction == 0.3
    analytic = LevelSet().add_plane((0, 1, 0), d=-0.3)
    # two frames: one lattice, one kind
    DynamicLevelSet().initialize(0.0, 1.0, a, SampledLevelSet(ok + 1, (0, 0, 0), 0.1))
    for other in (SampledLevelSet(np.zeros((4, 4, 5), np.float32), (0, 0, 0), 0.1), SampledLevelSet(ok, (0, 0.1, 0), 0.1),
                  SampledLevelSet(ok, (0, 0, 0), 0.2), analytic):
        with pytest.raises(MPMError):
            DynamicLevelSet().initialize(0.0, 1.0, a, other)
    with pytest.raises(MPMError):
        DynamicLevelSet().initialize(0.0, 1.0, analytic, a)
    with pytest.raises(MPMError):
        DynamicLevelSet().initialize(1.0, 1.0, a, a)


def test_from_function_layout():
    """sample (i, j, k) sits at origin + (i, j, k) spacing; the array is C-ordered with k fastest"""
    s = SampledLevelSet.from_function(lambda x: x[:, 0] * 100 + x[:, 1] * 10 + x[:, 2], (3, 4, 5), (1.0, 2.0, 3.0), 0.5)
    assert s.phi.shape == (3, 4, 5) and s.phi.flags["C_CONTIGUOUS"]
    assert s.phi[2, 3, 4] == np.float32((1 + 1.0) * 100 + (2 + 1.5) * 10 + 3 + 2.0)
