"""An emitter on a 2D simulation created without max_particles (run with -m gpu on an MI355X): add_particles(region=..., pd_source=True)
before every frame makes the ctx grow more than once.  mpmhip2d_reserve may give more room than it was asked for; Simulation2D has to
record the capacity the library has (mpmhip2d_capacity), not the one it asked for — with the smaller figure the next call but one
stopped with "2D particle capacity exceeded" although the library had room (examples/jet_2d.py stopped at frame 14 of 40)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RES, DX, DT = 64, 1.0 / 64, 1e-4


def test_an_emitter_grows_the_ctx_more_than_once():
    import taichi_mpm_amd as tm
    sim = tm.create_simulation2("mpm").initialize(dict(res=(RES, RES), delta_x=DX, base_delta_t=DT, gravity=(0, -10)))
    nozzle = tm.LevelSet().add_cuboid((0.2, 0.80, 0.0), (0.8, 0.86, 0.0))
    L = sim._L
    seeded, caps = [], []
    for frame in range(12):
        before = sim._n_added
        sim.add_particles(dict(type="water", region=nozzle, ppc=4, pd_source=True, initial_velocity=(0, -4), delta_t=0.01))
        seeded.append(sim._n_added - before)
        caps.append(int(L.mpmhip2d_capacity(sim._ctx)))
        assert sim._capacity == caps[-1]  # what Python records is what the library has
        sim.step(0.01)
    grown = int(np.count_nonzero(np.diff(caps))) + (caps[0] > 1024)
    print("seeded per call %s, capacities %s" % (seeded, sorted(set(caps))))
    assert min(seeded) > 100 and grown >= 2
    assert int(L.mpmhip2d_num_slots(sim._ctx)) == sum(seeded) <= caps[-1]
    assert sim.get_num_particles() == sum(seeded)  # (0.12 s from y = 0.8 at 4 m/s: y > 0.24, far from the 7 cells of the domain rule)
    # minus the deleted ones: a disc in the jet's path
    x = sim.get_particles()["x"]
    c = np.array([0.5, float(np.median(x[:, 1]))])
    sim.set_levelset(tm.SampledLevelSet2D.from_function(lambda p: np.linalg.norm(p - c, axis=1) - 0.1, (65, 65), (0, 0), DX).as_boundary(0.2))
    n_del = C.c_int64(0)
    sim._check(L.mpmhip2d_delete_particles_inside_level_set(sim._ctx, C.byref(n_del)))
    assert 0 < n_del.value < sum(seeded)
    assert sim.get_num_particles() == sum(seeded) - n_del.value
    sim.step(0.01)
    assert sim.get_num_particles() == sum(seeded) - n_del.value and np.isfinite(sim.get_particles()["x"]).all()
    sim.close()
