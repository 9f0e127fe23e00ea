"""The four tiny scenes behind the snapshot fixtures tests/golden/snapshot_*.bin, shared by the generator
(tests/golden/make_snapshot_golden.py) and tests/test_gpu_snapshot_compat.py.  Only the host path of save / load is under test:
at most 200 particles on a 16^3 or a 32^2 grid.  build(tm, name, with_particles) sets the scene up; a simulation that is going to
load a blob is built without the particles (bodies, level set and configuration come from the scene, the rest from the blob)."""
import os

from tests import cpic_scenes as cs
from tests.common import lattice_cube, make_state
from tests.golden.make_golden import mpm2d_state

SCENES = ("rigid3d", "async3d", "rigid2d", "async2d")
FLOOR = -0.2  # the plane y = 0.2
ASYNC_KW = dict(unit_delta_t=2e-6, max_units=1024)


def _two_groups_3d():
    """the 2 x 2 x 2 cells in the middle of a 16^3 grid (add_particles ignores whatever lies within 7 cells of a wall), 8 particles per
    cell: the left half elastic, the right half sand — 32 particles each"""
    dx = 1.0 / 16
    x = lattice_cube(16, 7, 9, dx, jitter=0.2, seed=1)
    left = x[:, 0] < 0.5
    return [(mat, make_state(x[half], mat, dx, perturb_F=0.01, vel_scale=0.5, seed=seed))
            for mat, half, seed in (("elastic", left, 1), ("sand", ~left, 2))]


def _two_groups_2d(tm):
    dx = 1.0 / 32
    vol = dx * dx / 4
    out = []
    for mat, lo, seed in (("elastic", (9, 12), 3), ("sand", (14, 12), 4)):  # 100 particles each
        x, v, F, B = mpm2d_state(32, lo=lo, cells=5, seed=seed)
        out.append((mat, tm.group_params(mat, 400 * vol, vol)[0], x, 0.3 * v, F, B))
    return out


def build(tm, name, with_particles=True):
    if name == "rigid3d":  # one box on a distance joint to the background above two blocks of particles; the collision pass is set
        sim = tm.create_simulation3("mpm").initialize(dict(res=(16,) * 3, delta_x=1.0 / 16, base_delta_t=1e-4, gravity=(0, -10, 0),
                                                           max_particles=256, penalty=1e3, rigid_body_collision=True,
                                                           rigid_body_iterations=3, rigid_penalty=2e3))
        sim.set_levelset(tm.mpm.LevelSet(friction=0.4).add_plane((0, 1, 0), d=FLOOR))
        sim.add_particles(dict(type="rigid", mesh=cs.box(0.1, 0.06, 0.12), codimensional=False, density=400.0, friction=0.3,
                               initial_position=(0.47, 0.66, 0.46), initial_rotation=(0.0, 30.0, 15.0), initial_velocity=(0.3, -0.5, 0.1)))
        if with_particles:
            sim.general_action(dict(action="add_articulation", type="distance", obj0=1, obj1=0, offset1=(0.45, 0.9, 0.5), penalty=2e3))
            for mat, s in _two_groups_3d():
                sim.add_particles(dict(type=mat, positions=s.x, velocities=s.v, F=s.F, B=s.B, aux=s.aux, params=s.gparams[0]))
        return sim
    if name == "async3d":
        sim = tm.create_simulation3("async_mpm").initialize(dict(res=(16,) * 3, delta_x=1.0 / 16, **ASYNC_KW))
        sim.set_levelset(tm.mpm.LevelSet(friction=0.4).add_plane((0, 1, 0), d=FLOOR))
        if with_particles:
            for mat, s in _two_groups_3d():
                sim.add_particles(dict(type=mat, positions=s.x, velocities=s.v, F=s.F, B=s.B, aux=s.aux, params=s.gparams[0]))
        return sim
    if name == "rigid2d":
        sim = tm.create_simulation2("mpm").initialize(dict(res=(32, 32), delta_x=1.0 / 32, base_delta_t=1e-4, gravity=(0, -10),
                                                           max_particles=256, penalty=1e3, rigid_body_levelset_collision=True))
        sim.set_levelset(tm.mpm.LevelSet(friction=0.4).add_plane((0, 1, 0), d=FLOOR))
        sim.add_particles(dict(type="rigid", mesh=cs.box2(0.1, 0.06), codimensional=False, density=400.0, friction=0.3,
                               initial_position=(0.45, 0.62), initial_rotation=30.0, initial_velocity=(0.3, -0.5), initial_angular_velocity=2.0))
        if with_particles:
            x, v, F, B = mpm2d_state(32, lo=(11, 10), cells=6, seed=5)  # 144 particles
            vol = (1.0 / 32) ** 2 / 4
            sim.add_particles(dict(type="sand", positions=x, velocities=v, F=F, B=B, params=tm.group_params("sand", 400 * vol, vol)[0]))
        return sim
    if name == "async2d":
        sim = tm.create_simulation2("async_mpm").initialize(dict(res=(32, 32), delta_x=1.0 / 32, **ASYNC_KW))
        sim.set_levelset(tm.mpm.LevelSet(friction=0.4).add_plane((0, 1, 0), d=FLOOR))
        if with_particles:
            for mat, gp, x, v, F, B in _two_groups_2d(tm):
                sim.add_particles(dict(type=mat, positions=x, velocities=v, F=F, B=B, params=gp))
        return sim
    raise KeyError(name)


def advance(sim, name, substeps):
    """`substeps` substeps of the synchronous steppers; the asynchronous ones take as many steps of 50 unit_delta_t"""
    if name.startswith("async"):
        for _ in range(substeps):
            sim.step(50 * ASYNC_KW["unit_delta_t"])
    else:
        sim.run_substeps(substeps)


def fixture_path(name, which):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snapshot_%s_%s.bin" % (name, which))


def n_particles(sim, name):
    return sim.get_num_pool_particles() if name.startswith("async") else sim.get_num_particles()

