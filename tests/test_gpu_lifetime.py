"""Every object of the library gives back the device and pinned arrays it took: mpmhip_debug_live_buffers() (the counter of
taichi_mpm_amd/csrc/host_mem.h, arrays not bytes — free device memory is moved by other people's jobs) is read, one create ... close
cycle through the Python layer visits the allocating paths of one kind of object, and the counter must be above the first reading
while the object lives and back AT it after close().  No case asks for an allocation meant to fail: tests/test_host_mem_cpu.py
covers those paths.

Shapes: the smallest at which the path in question allocates.  Particles nearer than 7 cells to a wall are dropped at creation, so a
16^3 / 16^2 grid holds particles in its two middle cells per axis.  Two cases need more: the auto-sized block table of a 3D ctx only
grows where the block space (8^kbits) exceeds particles / 48 + 4096, i.e. from 64 nodes per axis on (case a), and the CPIC scenes
come from tests/cpic_scenes.py at their own 32^3 / 64^2 (cases b, e)."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests import cpic_scenes as cs
from tests.common import lattice_cube, make_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


def _live(tm):
    gc.collect()  # (a simulation object some earlier test dropped without close() destroys its ctx in __del__)
    return int(tm.load().mpmhip_debug_live_buffers())


def _middle(res, n, dim, seed):
    """n positions in the two middle cells per axis of a res^dim grid with dx = 1 / res (7 cells off every wall on a 16-grid)"""
    rng = np.random.default_rng(seed)
    return ((res / 2 - 0.9 + 1.8 * rng.random((n, dim))) / res).astype(np.float32)


def test_a_3d_ctx_with_reserve_level_sets_frames_snapshot_and_energy(tm, tmp_path):
    base = _live(tm)
    res, dx = 64, 1.0 / 64
    sim = tm.create_simulation3("mpm").initialize(dict(res=(res,) * 3, delta_x=dx, base_delta_t=1e-4, max_particles=600))
    s = make_state(lattice_cube(res, 28, 32, dx, jitter=0.2, seed=1), "jelly", dx, perturb_F=0.02)
    sim.add_particles(dict(type="jelly", positions=s.x, velocities=s.v, F=s.F, B=s.B, aux=s.aux, params=s.gparams[0]))
    sim.run_substeps(2)
    assert _live(tm) > base
    sim.set_deterministic(True)
    sim.substep()
    # 512 more particles: past the capacity of 600 -> mpmhip_reserve(1280); 1280 / 48 + 4096 > 600 / 48 + 4096: the block table grows too
    blocks = lambda cap: cap // 48 + 4096
    s2 = make_state(lattice_cube(res, 34, 38, dx, jitter=0.2, seed=2), "jelly", dx, perturb_F=0.02)
    sim.add_particles(dict(type="jelly", positions=s2.x, velocities=s2.v, F=s2.F, B=s2.B, aux=s2.aux, params=s2.gparams[0]))
    cap = int(sim._L.mpmhip_capacity(sim._ctx))
    assert cap >= 1024 and blocks(cap) > blocks(600) and blocks(cap) < 8 ** 5
    sim.substep()
    floor = tm.LevelSet(friction=0.4).add_plane((0, 1, 0), d=-0.3)
    sim.set_levelset(tm.SampledLevelSet.from_levelset(floor, (9,) * 3, (0.2, 0.2, 0.2), 0.075))
    sim.substep()
    sim.set_levelset(tm.SampledLevelSet.from_levelset(floor, (12,) * 3, (0.2, 0.2, 0.2), 0.05))  # another lattice: new arrays
    sim.substep()
    sim.set_levelset(floor)  # analytic shapes replace the sampled set
    sim.substep()
    mesh = cs.box() + np.float32([0.5037, 0.4971, 0.5013])  # (off the lattice planes)
    sim.set_levelset(tm.MeshLevelSet(mesh, (17,) * 3, (0.3, 0.3, 0.3), 0.025, band=0.1))
    assert np.isfinite(sim.download_levelset_sdf()[0]).all()
    assert len(sim.bgeo_bytes(verbose=False)) < len(sim.bgeo_bytes(verbose=True))
    path = str(tmp_path / "a.snapshot")
    sim.save_snapshot(path)
    sim.load_snapshot(path)
    assert sim.get_num_particles() == s.n + s2.n
    kin, pot = sim.calculate_energy()
    assert np.isfinite(kin) and np.isfinite(pot)
    assert _live(tm) > base
    sim.close()
    assert _live(tm) == base


def test_b_cpic_ctx_with_a_second_body_samples_and_the_distance_field(tm):
    base = _live(tm)
    sim, rid = cs.build_device(tm, "box", "jelly", penalty=1e3, deterministic=True, rigid_body_levelset_collision=True)
    sim.set_levelset(tm.LevelSet(friction=0.3).add_plane((0, 1, 0), d=-0.3).add_plane((-1, 0, 0), d=0.66))
    sim.substep()
    assert _live(tm) > base
    plate = dict(cs.BODIES["plate"], initial_position=(0.503, 0.72, 0.501))  # (cuts the top of the block, clear of the box)
    rid2 = int(sim.add_particles(dict(type="rigid", **plate)))  # the samples of both bodies are uploaded again
    assert rid2 == rid + 1
    sim.run_substeps(2)
    smp = sim.get_rigid_samples()
    assert len(np.unique(smp["body"])) == 2 and np.isfinite(smp["pos"]).all()
    states, dist = sim.download_cdf()
    assert states.shape == dist.shape == (cs.RES + 1,) * 3 and np.isfinite(dist).all()
    assert _live(tm) > base
    sim.close()
    assert _live(tm) == base


def test_c_resident_async_stepper_begun_twice(tm):
    base = _live(tm)
    res, dx = 16, 1.0 / 16
    kw = dict(unit_delta_t=2e-6, max_units=1024)
    sim = tm.create_simulation3("async_mpm").initialize(dict(res=(res,) * 3, delta_x=dx, **kw))
    sim._ensure_ctx()  # mpmhip_async_begin ...
    from taichi_mpm_amd import _lib
    again = _lib.AsyncConfig(kw["unit_delta_t"], kw["max_units"], 1.0, 1.0, 0)
    sim._check(sim._L.mpmhip_async_begin(sim._ctx, C.byref(again)))  # ... and once more: the tables of the first go
    assert _live(tm) > base
    x = _middle(res, 300, 3, seed=3)
    sim.add_particles(dict(type="elastic", positions=x, velocities=np.zeros_like(x)))
    for _ in range(3):
        sim.step(1e-3)
    pools = sim.get_pool_particles()  # mpmhip_async_download_pools
    assert set(np.unique(pools["id"])) == set(range(len(x)))
    assert _live(tm) > base
    sim.close()
    assert _live(tm) == base


def test_c_resident_async_stepper_begun_again_after_use(tm):
    """mpmhip_async_begin on a ctx whose store has been used starts from an EMPTY store (AsyncStore::reset): the containers, tags and
    pending counters of the first session are gone, so the pools of the second session hold the second session's particles alone.
    The store's size is bounded by what the second session can have appended: its pooled particles plus one container per particle
    update (state[1], which begin resets), whether or not a compaction ran."""
    base = _live(tm)
    res, dx = 16, 1.0 / 16
    kw = dict(unit_delta_t=2e-6, max_units=1024)
    sim = tm.create_simulation3("async_mpm").initialize(dict(res=(res,) * 3, delta_x=dx, **kw))
    x = _middle(res, 300, 3, seed=3)
    x[:, 0] = (res / 2 - 0.9 + 0.85 * (x[:, 0] * res - (res / 2 - 0.9)) / 1.8) / res  # the lower of the two middle cells along x
    sim.add_particles(dict(type="elastic", positions=x, velocities=np.zeros_like(x)))
    for _ in range(3):
        sim.step(1e-3)
    assert set(np.unique(sim.get_pool_particles()["id"])) == set(range(len(x)))
    from taichi_mpm_amd import _lib
    again = _lib.AsyncConfig(kw["unit_delta_t"], kw["max_units"], 1.0, 1.0, 0)
    sim._check(sim._L.mpmhip_async_begin(sim._ctx, C.byref(again)))
    x2 = _middle(res, 100, 3, seed=4)
    x2[:, 0] = (res / 2 + 0.05 + 0.85 * (x2[:, 0] * res - (res / 2 - 0.9)) / 1.8) / res  # the upper one
    sim.add_particles(dict(type="elastic", positions=x2, velocities=np.zeros_like(x2)))
    for _ in range(3):
        sim.step(1e-3)
    ids = set(np.unique(sim.get_pool_particles()["id"]).tolist())
    st = sim._state()
    print("second session: ids %d..%d (%d), state %s" % (min(ids), max(ids), len(ids), st))
    assert ids and ids <= set(range(len(x), len(x) + len(x2))), sorted(ids)[:8]
    assert st[4] <= st[5] <= len(x2) + st[1], st
    assert _live(tm) > base
    sim.close()
    assert _live(tm) == base


def test_d_local_tiled_job_of_two_virtual_ranks_with_a_migration(tm):
    """(the halo arena of each rank is allocated by one of two runtime calls and mapped by peers: the one array outside the counter)"""
    from taichi_mpm_amd import tiled
    from taichi_mpm_amd.mpm import F_ID
    base = _live(tm)
    res, dx = 32, 1.0 / 32
    s = make_state(lattice_cube(res, 14, 18, dx, jitter=0.2, seed=4), "jelly", dx, perturb_F=0.0, vel_scale=0.0)
    s.v[:] = (25.0, 0.0, 0.0)  # 0.08 cells per substep: in 50 substeps rank 0's two cells of particles cross the cut and the margin
    s.B[:] = 0
    part = tiled.Partition.balanced((res,) * 3, 2, s.x, dx, margin=2, dims=(2, 1, 1))
    owner = part.rank_of_cells(tiled.base_cells(s.x, dx))
    sims = []
    for r in range(2):
        m = owner == r
        sim = tm.create_simulation3("mpm").initialize(dict(res=(res,) * 3, delta_x=dx, base_delta_t=1e-4, max_particles=s.n, reorder_interval=0))
        sim.add_particles(dict(type="jelly", positions=s.x[m], velocities=s.v[m], F=s.F[m], B=s.B[m], aux=s.aux[m], params=s.gparams[0]))
        sim.upload(F_ID, np.nonzero(m)[0].astype(np.int32))
        sims.append(sim)
    job = tiled.NativeVirtualJob([tiled.HipEngine(sim, 0) for sim in sims], part, migrate_interval=2, inbox_records=s.n)
    job.run(50)
    st = job.state()
    assert all(t["substeps"] == 50 for t in st) and sum(t["migrated_out"] for t in st) > 0, st
    assert sum(sim.get_num_particles() for sim in sims) == s.n
    assert _live(tm) > base
    del job
    for sim in sims:
        sim.close()
    assert _live(tm) == base


def test_e_2d_objects_deterministic_cpic_and_a_growing_async_store(tm, tmp_path):
    base = _live(tm)
    sim, rid = cs.build_device2(tm, "bar", "jelly", penalty=1e3, deterministic=True)
    sim.run_substeps(3)
    assert _live(tm) > base
    assert len(sim.get_rigid_samples(rid)) > 0
    path = str(tmp_path / "e.snapshot")
    sim.save_snapshot(path)
    sim.load_snapshot(path)
    sim.substep()
    assert len(sim.bgeo_bytes()) > 0
    sim.close()
    assert _live(tm) == base
    # the resident 2D stepper: 300 particles, then 5000 more than the arrays (1474) and the container store (4096) were made for
    res, dx = 16, 1.0 / 16
    a = tm.create_simulation2("async_mpm").initialize(dict(res=(res, res), delta_x=dx, unit_delta_t=2e-6, max_units=1024))
    x = _middle(res, 300, 2, seed=5)
    a.add_particles(dict(type="elastic", positions=x, velocities=np.zeros_like(x)))
    a.step(1e-3)
    x2 = _middle(res, 5000, 2, seed=6)
    a.add_particles(dict(type="elastic", positions=x2, velocities=np.zeros_like(x2)))
    a.step(1e-3)
    assert a.get_num_pool_particles() >= len(x) + len(x2)
    assert len(a.get_particles()["id"]) >= len(x) + len(x2)  # mpmhip2d_async_load_pools: the view of every container
    assert _live(tm) > base
    a.close()
    assert _live(tm) == base


def test_f_mpm88_and_the_standalone_voxeliser(tm):
    base = _live(tm)
    sim = tm.MPM88(n=16)
    sim.add_object((0.5, 0.5), count=200)
    sim.advance(2)
    sim.add_object((0.45, 0.55), count=300)  # past the first capacity: the arrays grow
    sim.advance(2)
    assert sim.num_particles() == 500 and _live(tm) > base
    sim.close()
    assert _live(tm) == base
    mesh = cs.box() + np.float32([0.5037, 0.4971, 0.5013])
    sdf = tm.SampledLevelSet.from_mesh(mesh, (17,) * 3, (0.3, 0.3, 0.3), 0.025, band=0.1)  # mpmhip_mesh_to_sdf: no object survives the call
    assert np.isfinite(sdf.phi).all() and (sdf.phi < 0).any() and (sdf.phi > 0).any()
    assert _live(tm) == base
