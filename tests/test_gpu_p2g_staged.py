"""k_p2g reads each window of a block's particle records through LDS (csrc/k_p2g.h: p2g_cell_staged): a window is two particles
per cell, the block's fullest cell sets the number of windows.  These scenes exercise what the lattice does not: cells with many
more particles than a window and odd counts, blocks with one particle in a few cells, and an evolved state whose records no
longer sit in sort order.  The P2G grid is held to the parity tolerances of tests/test_gpu_parity.py (mass rel-L2 <= 1e-6,
momentum <= 1e-5); in the deterministic mode (every cell in creation-id order) the grid may not depend on where the records lie,
so a shuffled copy of the input gives the same bits."""
import numpy as np
import pytest

from tests.common import lattice_cube, make_state, rel_l2
from tests.test_gpu_parity import DX, make_sim, ocfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


def _p2g_grid(sim):
    sim.sort_particles_and_populate_grid()
    sim.rasterize_optimized()
    return sim.get_grid(0)


def _check_against_oracle(orc, g0, s):
    ref = orc.p2g(ocfg(orc), s.copy())
    assert rel_l2(g0[..., 3], ref[..., 3]) <= 1e-6
    assert rel_l2(g0[..., :3], ref[..., :3]) <= 1e-5
    assert np.array_equal(g0[..., 3] != 0, ref[..., 3] != 0)


def _crowded(seed):
    """the lattice (8 per cell) plus clumps of 1..40 particles in single cells: counts far beyond a window, odd and even"""
    rng = np.random.default_rng(seed)
    x = [lattice_cube(32, 10, 16, DX, jitter=0.2, seed=seed)]
    for k, cell in enumerate(rng.integers(10, 16, (12, 3))):
        m = 1 + (7 * k) % 40
        x.append(((cell + rng.uniform(0.05, 0.95, (m, 3))) * DX).astype(np.float32))
    return np.concatenate(x).astype(np.float32)


@pytest.mark.parametrize("mat", ["jelly", "sand"])
def test_crowded_cells_match_oracle(tm, orc, mat):
    s = make_state(_crowded(31), mat, DX, perturb_F=0.02, seed=32)
    sim = make_sim(tm, s)
    _check_against_oracle(orc, _p2g_grid(sim), s)
    sim.close()


def test_sparse_blocks_match_oracle(tm, orc):
    """a few hundred particles scattered over 16^3 cells: most blocks hold one to three particles, most cells none"""
    rng = np.random.default_rng(41)
    x = rng.uniform(9 * DX, 25 * DX, (300, 3)).astype(np.float32)
    s = make_state(x, "jelly", DX, perturb_F=0.02, seed=42)
    sim = make_sim(tm, s)
    _check_against_oracle(orc, _p2g_grid(sim), s)
    sim.close()


def test_evolved_state_matches_oracle(tm, orc):
    """after 20 substeps of a spinning, crowded scene the records lie where the last G2P put them and the sort's permutation is
    no longer the identity; the oracle rasterises the state the device holds (apic_b stored exactly)"""
    s = make_state(_crowded(51), "jelly", DX, perturb_F=0.02, seed=52, vel_scale=3.0)
    sim = make_sim(tm, s, keep_apic_b=True)
    for _ in range(20):
        sim.substep()
    got = sim.get_particles()
    assert len(got["id"]) == s.n
    ev = s.copy()
    ev.x[:], ev.v[:], ev.B[:], ev.F[:], ev.aux[:] = got["x"], got["v"], got["B"], got["F"], got["aux"]
    _check_against_oracle(orc, _p2g_grid(sim), ev)
    sim.close()


def test_deterministic_grid_does_not_depend_on_record_order(tm, monkeypatch):
    """the same particles added in lattice order and shuffled: in the deterministic mode each cell is summed in creation-id
    order, so the staged loads must deliver the same records in the same order from near-identity and scattered permutations"""
    monkeypatch.setenv("MPMHIP_DETERMINISTIC", "1")
    x = _crowded(61)
    s = make_state(x, "sand", DX, perturb_F=0.02, seed=62)
    order = np.random.default_rng(63).permutation(s.n)
    grids = []
    for perm in (np.arange(s.n), order):
        t = s.copy()
        t.x[:], t.v[:], t.B[:], t.F[:], t.aux[:] = s.x[perm], s.v[perm], s.B[perm], s.F[perm], s.aux[perm]
        sim = make_sim(tm, t)
        sim.substep()
        grids.append(_p2g_grid(sim))
        sim.close()
    assert grids[0].tobytes() != bytes(grids[0].nbytes)
    # creation ids follow the order of addition, so the two runs sum each cell in different particle orders: the grids agree to
    # rounding, and each run repeats itself to the bit
    assert rel_l2(grids[1][..., 3], grids[0][..., 3]) <= 1e-6
    sim = make_sim(tm, s)
    sim.substep()
    again = _p2g_grid(sim)
    sim.close()
    assert np.array_equal(again, grids[0])
