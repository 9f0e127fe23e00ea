"""The constitutive path on ILL-CONDITIONED deformation gradients, against the reference's own particles.cpp
(tests/golden/ref_illcond.npz: output of oracle/_ref/libmpm_ref.so, generator tests/golden/make_golden.py: illcond_fixture).

The reference calls svd(F) / polar_decomp(F) (src/particles.cpp:207-242, 391-416, 599-647, 701-732, 786-812); the device
takes U and sigma^2 from a Jacobi eigen-solve of F F^T in fp32 (csrc/mpm_math.h: sym_eig3_FFt), which alone would lose
sigma_min like eps cond(F)^2, and measures the singular values again on F itself when the wave holds a matrix with
cond(F) > 8 (sym_eig3_refine: eps cond(F)).  F = U diag(sigma) V^T with cond in {1, 10, 1e2, 1e3, 1e4} in four patterns,
repeated / nearly repeated singular values, singular values at sand's 1e-4 clamp, det F < 0 for the non-Hencky models.
The tolerances of tests/test_gpu_ref.py::test_device_materials_match_the_reference must hold up to cond 1e2 (asserted:
they hold to 1e3); the measured error per condition number is printed (pytest -s) and recorded in DESIGN.md section 2."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.common import lattice_cube
from tests.materials2d_common import assert_illcond_bounds, cond_classes, errors, print_illcond_table  # shared with the 2D tests

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
MATS = ["jelly", "snow", "sand", "water", "linear", "elastic", "von_mises", "visco"]
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


@pytest.fixture(scope="module")
def ctx_sim(tm):
    sim = tm.create_simulation3("mpm")
    sim.initialize(dict(res=(32, 32, 32), delta_x=1 / 32, base_delta_t=1e-4))
    sim.add_particles(dict(type="jelly", positions=lattice_cube(32, 10, 12, 1 / 32)))
    sim._ensure_ctx()
    yield sim
    sim.close()


def device_outputs(sim, g, mat):
    gp, t = np.ascontiguousarray(g[mat + "_gp"], np.float32), int(g[mat + "_type"])
    F, cdg, aux = (np.ascontiguousarray(a, np.float32) for a in (g["F"], g["cdg"], g[mat + "_aux"]))
    n = len(F)
    force = np.zeros((n, 9), np.float32)
    sim._check(sim._L.mpmhip_debug_force(sim._ctx, t, gp.ctypes.data_as(FP), n, F.ctypes.data_as(FP), aux.ctypes.data_as(FP),
                                         force.ctypes.data_as(FP)))
    F2, aux2, force2 = F.copy(), aux.copy(), np.zeros((n, 9), np.float32)
    sim._check(sim._L.mpmhip_debug_plasticity(sim._ctx, t, gp.ctypes.data_as(FP), n, cdg.ctypes.data_as(FP), F2.ctypes.data_as(FP),
                                              aux2.ctypes.data_as(FP), force2.ctypes.data_as(FP)))
    if mat == "water":
        F2 = F.copy()  # water never updates dg_e (src/particles.cpp:469-478)
    return force, F2, aux2, force2


@pytest.mark.parametrize("mat", MATS)
def test_device_materials_on_ill_conditioned_deformation_gradients(ctx_sim, mat):
    g = np.load(os.path.join(HERE, "golden", "ref_illcond.npz"))
    rows = errors(g, mat, device_outputs(ctx_sim, g, mat))
    print_illcond_table(mat, rows)
    # the tolerances of the well-conditioned fixture (3e-5 stress, 2e-5 F) hold up to cond 1e2 — and, with the singular values
    # measured on F, an order further; beyond that the error grows like eps cond.  Measured at cond 1e3:
    # F_new <= 1.7e-4, stress <= 5e-5 — but 1.3e-3 / 3.3e-3 for the NEXT stress of von Mises / visco.
    assert_illcond_bounds(mat, rows)


def test_device_singular_values_keep_their_relative_accuracy(ctx_sim):
    """mpmhip_debug_svd3 against the singular values of the same float32 matrices in double precision: RELATIVE error of every
    sigma, per condition number"""
    g = np.load(os.path.join(HERE, "golden", "ref_illcond.npz"))
    F = np.ascontiguousarray(g["F"], np.float32)
    n = len(F)
    U = np.zeros((n, 9), np.float32); S = np.zeros((n, 3), np.float32); V = np.zeros((n, 9), np.float32)
    sim = ctx_sim
    sim._check(sim._L.mpmhip_debug_svd3(sim._ctx, n, F.ctypes.data_as(FP), U.ctypes.data_as(FP), S.ctypes.data_as(FP), V.ctypes.data_as(FP)))
    want = g["sigma"]  # descending, sign on the last
    have = np.sort(np.abs(S.astype(np.float64)), 1)[:, ::-1]
    rel = np.abs(have - np.abs(want)) / np.abs(want)
    assert np.all(np.sign(np.prod(S, 1)) == np.sign(want[:, 2]))  # the sign of det F goes on one sigma
    Um = U.reshape(n, 3, 3).astype(np.float64)
    assert np.abs(np.einsum("nji,njk->nik", Um, Um) - np.eye(3)).max() < 2e-5
    print("\ncond     rows   max relative error of sigma_max / sigma_mid / sigma_min")
    for c, sel in cond_classes(g["cond"]):
        r = rel[sel].max(0)
        print("%-7g  %4d   %.2e  %.2e  %.2e" % (c, sel.sum(), r[0], r[1], r[2]))
        assert r.max() <= 4e-7 * max(c, 8.0), (c, r)  # eps cond(F), against eps cond(F)^2 of sqrt(eig(F F^T))
