"""The 2D constitutive path ON THE DEVICE (csrc/mpm2d_math.h through the test entries mpmhip2d_debug_force / _plasticity / _svd2,
csrc/k_debug2d.h) against the reference's dim = 2 particles: large strains and every branch of the return maps
(tests/golden/ref_materials2d.npz), ill-conditioned F up to cond 1e4, det F < 0, scaled rotations, sand's clamp
(ref_illcond2d.npz) — the same assertions tests/test_materials2d_cpu.py runs through the host build of the same header
(tests/materials2d_common.py), with the bounds of the 3D tests — and ONE substep of the transfer kernels (k_p2g, k_g2p, the
deterministic stage / gather) from strongly stretched particles against the reference's MPM<2> (ref_mpm2d_stretch.npz).
Every per-row test is one launch of a few hundred rows.

Not reached, on purpose: visco's step-halving loop — in 2D det(I + S + S^2 / 2) cannot be negative (tests/test_materials2d_cpu.py
has the argument), so no state takes it."""
import numpy as np
import pytest

from tests import materials2d_common as m2c
from tests.common import load_golden, rel_l2
from tests.materials2d_common import fptr

pytestmark = pytest.mark.gpu
MATS = m2c.MATS
EINVAL = -1


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


class DeviceBackend:
    """the three test entries on one 2D ctx"""

    def __init__(self, sim):
        self.sim, self.L, self.ctx = sim, sim._L, sim._ctx

    def force(self, t, gp, F, aux):
        out = np.zeros_like(F)
        self.sim._check(self.L.mpmhip2d_debug_force(self.ctx, t, fptr(gp), len(F), fptr(F), fptr(aux), fptr(out)))
        return out

    def plasticity(self, t, gp, cdg, F, aux, fused=True):
        F2, aux2, nf = F.copy(), aux.copy(), np.zeros_like(F)
        self.sim._check(self.L.mpmhip2d_debug_plasticity(self.ctx, t, fptr(gp), len(F), fptr(cdg), fptr(F2), fptr(aux2),
                                                         fptr(nf) if fused else None))
        return F2, aux2, nf

    def svd2(self, F):
        n = len(F)
        cu, su, S = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 2), np.float32)
        self.sim._check(self.L.mpmhip2d_debug_svd2(self.ctx, n, fptr(F), fptr(cu), fptr(su), fptr(S)))
        return cu, su, S


@pytest.fixture(scope="module")
def device(tm):
    sim = tm.create_simulation2("mpm").initialize(dict(res=(32, 32), delta_x=1 / 32, base_delta_t=1e-4))
    sim.add_particles(dict(type="jelly", positions=np.array([[0.4, 0.5], [0.5, 0.5], [0.6, 0.5], [0.5, 0.6]], np.float32)))
    sim._ensure_ctx()
    yield DeviceBackend(sim)
    sim.close()


@pytest.mark.parametrize("mat", MATS)
def test_device_2d_materials_match_the_reference(device, mat):
    m2c.check_materials2d(device, mat)


@pytest.mark.parametrize("mat", MATS)
def test_device_2d_materials_on_ill_conditioned_deformation_gradients(device, mat):
    m2c.check_illcond2d(device, mat)


@pytest.mark.parametrize("mat", MATS)
def test_device_2d_outputs_stay_finite_where_the_reference_is(device, mat):
    m2c.check_finite2d(device, mat)


def test_device_2d_singular_values_keep_their_relative_accuracy(device):
    m2c.check_svd2(device)


def test_device_2d_plasticity_alone_equals_the_fused_form_and_rows_beyond_one_grid_are_reached(device):
    """force_out = NULL; and more rows than one launch's lanes (1024 workgroups of 256), which the grid-stride loop must reach"""
    g = m2c.illcond2d()
    F, cdg = (np.ascontiguousarray(g[k], np.float32) for k in ("F", "cdg"))
    gp, t, aux = np.ascontiguousarray(g["snow_gp"], np.float32), int(g["snow_type"]), np.ascontiguousarray(g["snow_aux"], np.float32)
    a, b = device.plasticity(t, gp, cdg, F, aux, fused=True), device.plasticity(t, gp, cdg, F, aux, fused=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    reps = 1024 * 256 // len(F) + 2  # > 262144 rows
    big = device.force(t, gp, np.tile(F, (reps, 1)), np.tile(aux, reps))
    assert np.array_equal(big.reshape(reps, len(F), 4), np.broadcast_to(device.force(t, gp, F, aux), (reps, len(F), 4)))


def test_2d_debug_entries_check_their_arguments(device):
    L, ctx = device.L, device.ctx
    F = np.eye(2, dtype=np.float32).reshape(1, 4).repeat(3, 0)
    aux, out, gp = np.zeros(3, np.float32), np.full((3, 4), 7.0, np.float32), np.zeros(16, np.float32)
    gp[1:4] = 1.0
    cu, S = np.zeros(3, np.float32), np.zeros((3, 2), np.float32)
    jelly = 4
    assert L.mpmhip2d_debug_force(None, jelly, fptr(gp), 3, fptr(F), fptr(aux), fptr(out)) == EINVAL
    assert L.mpmhip2d_debug_force(ctx, jelly, None, 3, fptr(F), fptr(aux), fptr(out)) == EINVAL
    assert L.mpmhip2d_debug_force(ctx, jelly, fptr(gp), 3, None, fptr(aux), fptr(out)) == EINVAL
    assert L.mpmhip2d_debug_force(ctx, jelly, fptr(gp), 3, fptr(F), None, fptr(out)) == EINVAL
    assert L.mpmhip2d_debug_force(ctx, jelly, fptr(gp), 3, fptr(F), fptr(aux), None) == EINVAL
    assert L.mpmhip2d_debug_force(ctx, jelly, fptr(gp), -1, fptr(F), fptr(aux), fptr(out)) == EINVAL
    for bad in (0, 9, -3):
        assert L.mpmhip2d_debug_force(ctx, bad, fptr(gp), 3, fptr(F), fptr(aux), fptr(out)) == EINVAL
        assert L.mpmhip2d_debug_plasticity(ctx, bad, fptr(gp), 3, fptr(F), fptr(F), fptr(aux), None) == EINVAL
    assert L.mpmhip2d_debug_plasticity(None, jelly, fptr(gp), 3, fptr(F), fptr(F), fptr(aux), None) == EINVAL
    assert L.mpmhip2d_debug_plasticity(ctx, jelly, None, 3, fptr(F), fptr(F), fptr(aux), None) == EINVAL
    assert L.mpmhip2d_debug_plasticity(ctx, jelly, fptr(gp), 3, None, fptr(F), fptr(aux), None) == EINVAL
    assert L.mpmhip2d_debug_plasticity(ctx, jelly, fptr(gp), 3, fptr(F), None, fptr(aux), None) == EINVAL
    assert L.mpmhip2d_debug_plasticity(ctx, jelly, fptr(gp), 3, fptr(F), fptr(F), None, None) == EINVAL
    assert L.mpmhip2d_debug_plasticity(ctx, jelly, fptr(gp), -1, fptr(F), fptr(F), fptr(aux), None) == EINVAL
    assert L.mpmhip2d_debug_svd2(None, 3, fptr(F), fptr(cu), fptr(cu), fptr(S)) == EINVAL
    assert L.mpmhip2d_debug_svd2(ctx, 3, None, fptr(cu), fptr(cu), fptr(S)) == EINVAL
    assert L.mpmhip2d_debug_svd2(ctx, 3, fptr(F), None, fptr(cu), fptr(S)) == EINVAL
    assert L.mpmhip2d_debug_svd2(ctx, 3, fptr(F), fptr(cu), None, fptr(S)) == EINVAL
    assert L.mpmhip2d_debug_svd2(ctx, 3, fptr(F), fptr(cu), fptr(cu), None) == EINVAL
    assert L.mpmhip2d_debug_svd2(ctx, -1, fptr(F), fptr(cu), fptr(cu), fptr(S)) == EINVAL
    assert np.all(out == 7.0)  # nothing was written by a refused call
    # n == 0: success, nothing launched, nothing written
    assert L.mpmhip2d_debug_force(ctx, jelly, fptr(gp), 0, fptr(F), fptr(aux), fptr(out)) == 0
    assert L.mpmhip2d_debug_plasticity(ctx, jelly, fptr(gp), 0, fptr(F), fptr(F), fptr(aux), None) == 0
    assert L.mpmhip2d_debug_svd2(ctx, 0, fptr(F), fptr(cu), fptr(cu), fptr(S)) == 0
    assert np.all(out == 7.0) and np.array_equal(F, np.eye(2, dtype=np.float32).reshape(1, 4).repeat(3, 0))


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("mat", ["jelly", "elastic"])
def test_one_substep_from_strongly_stretched_particles_matches_the_reference(tm, mat, deterministic):
    """cond(F) = 30 and 100 (R diag(sqrt c, 1 / sqrt c) R^T, det F = 1) through k_p2g + k_g2p, and through the stage / gather P2G of
    the deterministic mode; the bounds of tests/test_gpu_mpm2d.py::test_mpm2d_matches_the_reference_fixture"""
    from tests.test_gpu_mpm2d import _levelset
    g = load_golden("ref_mpm2d_stretch")
    res, dx, dt = int(g["res"]), float(g["dx"]), float(g["dt"])
    sim = tm.create_simulation2("mpm").initialize(dict(res=(res, res), delta_x=dx, base_delta_t=dt, deterministic=deterministic))
    sim.set_levelset(_levelset(tm, [(0, 0, 0, 1, 0, -0.37)], 0.4))
    sim.add_particles(dict(type=mat, positions=g["x"], velocities=g["v"], F=g["F"], B=g["B"], aux=np.zeros(len(g["x"]), np.float32),
                           params=g["gp_" + mat]))
    sim.substep()
    got = sim.get_particles()
    sim.close()
    want = g["floor_" + mat]
    assert np.array_equal(got["id"], g["floor_%s_ids" % mat])
    ex, ev = np.abs(got["x"] - want[:, 0:2]).max(), rel_l2(got["v"], want[:, 2:4])
    eF, eB = rel_l2(got["F"], want[:, 4:8]), rel_l2(got["B"], want[:, 8:12])
    ea = np.abs(got["aux"] - want[:, 12]).max() / max(1.0, np.abs(want[:, 12]).max())
    print("\nstretch %-8s %-13s x %.2e  v %.2e  F %.2e  B %.2e  aux %.2e" % (mat, "deterministic" if deterministic else "default", ex, ev, eF, eB, ea))
    assert ex <= 5e-7 and ev <= 5e-5 and eF <= 1e-4 and eB <= 2e-4 and ea <= 5e-5
