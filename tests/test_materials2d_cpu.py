"""The 2D constitutive math the device runs (taichi_mpm_amd/csrc/mpm2d_math.h: eig_FFt, signed_sigma, calculate_force,
plasticity of all eight particle types) compiled for the HOST by g++ (tests/cpp/mpm2d_math_host.cpp) and held to the reference's
dim = 2 particles (src/particles.cpp with MPMParticle<2>) — no GPU needed.  The fixtures are output of the reference's own code
(tests/golden/make_golden.py: materials2d_fixture, illcond2d_fixture):
  ref_materials2d.npz   384 states per material, strains up to 0.2, every branch of every return map (asserted by the generator)
  ref_illcond2d.npz     F = R(a) diag(sigma) R(b)^T with cond(F) from 1 to 1e4, det F < 0, repeated singular values, scaled
                        rotations (the fallback of eig_FFt), symmetric / diagonal F, sand's 1e-4 clamp
tests/test_gpu_materials2d.py runs the SAME assertions (tests/materials2d_common.py) through the device's test entries
mpmhip2d_debug_force / _plasticity / _svd2; the bounds are those of the 3D tests (tests/test_gpu_ref.py, tests/test_gpu_illcond.py).

Not reached, on purpose: visco's step-halving loop (taken while det(I + S + S^2 / 2) <= 0, S = cdg - I).  The eigenvalues of that
matrix are p(l) = 1 + l + l^2 / 2 = ((l + 1)^2 + 1) / 2 of the eigenvalues l of S: positive for real l, and for a complex pair the
determinant is |p(l)|^2 >= 0, zero only at l = -1 +- i (a cdg with eigenvalues +- i: a quarter turn per substep).  So in 2D the
loop's condition holds on no state a simulation produces, and no fixture row takes it."""
import pytest

from tests import materials2d_common as m2c

MATS = m2c.MATS


@pytest.fixture(scope="module")
def host():
    return m2c.HostBackend()


@pytest.mark.parametrize("mat", MATS)
def test_host_build_of_the_2d_materials_matches_the_reference(host, mat):
    m2c.check_materials2d(host, mat)


@pytest.mark.parametrize("mat", MATS)
def test_host_build_of_the_2d_materials_on_ill_conditioned_deformation_gradients(host, mat):
    m2c.check_illcond2d(host, mat)


@pytest.mark.parametrize("mat", MATS)
def test_host_build_keeps_every_output_finite_where_the_reference_is(host, mat):
    m2c.check_finite2d(host, mat)


def test_host_build_singular_values_keep_their_relative_accuracy(host):
    m2c.check_svd2(host)


def test_plasticity_alone_equals_the_fused_form(host):
    """force_out = NULL runs plasticity alone: the same F and aux as with the next force"""
    import numpy as np
    g = m2c.illcond2d()
    F, cdg = (np.ascontiguousarray(g[k], np.float32) for k in ("F", "cdg"))
    for mat in MATS:
        gp, t, aux = np.ascontiguousarray(g[mat + "_gp"], np.float32), int(g[mat + "_type"]), np.ascontiguousarray(g[mat + "_aux"], np.float32)
        a, b = host.plasticity(t, gp, cdg, F, aux, fused=True), host.plasticity(t, gp, cdg, F, aux, fused=False)
        assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)
