"""Rigid-rigid collisions on the device (MPM::rigidify, src/mpm_rigid_body.cpp:306-345; taichi_mpm_amd/csrc/k_rigid_collide.h):
the detection kernel against libccd's recorded answers, the whole pass against the host build of the same header (bit for bit),
what the pass does to a scene, its settings, and that a scene without it runs what it ran before."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

from tests import cpic_scenes as cs
from tests import rigid_collide_host as rh

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


# ------------------------------------------------------------------------------------------------------------- detection
def test_detection_kernel_reproduces_the_fixture_bit_for_bit(tm):
    """mpmhip_rigid_mpr_test on the whole fixture in one launch (one workgroup per pair): hit flags, depth, dir, pos and the
    number of support calls equal libccd's — and so the host build's — on every pair"""
    g = rh.fixture()
    L = tm.load()
    n = len(g["ret"])
    out = np.full((n, 9), np.nan, F)
    v, o = np.ascontiguousarray(g["verts"], F), np.ascontiguousarray(g["offsets"], np.int64)
    r, c = np.ascontiguousarray(g["rot"], F), np.ascontiguousarray(g["ctr"], F)
    rc = L.mpmhip_rigid_mpr_test(0, n, v.ctypes.data_as(rh.fp), o.ctypes.data_as(C.POINTER(C.c_int64)), r.ctypes.data_as(rh.fp),
                                 c.ctypes.data_as(rh.fp), out.ctypes.data_as(rh.fp))
    assert rc == 0, L.mpmhip_last_error(None).decode()
    want = rh.fixture_expected(g)
    same = rh.same_bits(out, want)
    bad = np.nonzero(~same.all(axis=1))[0]
    assert len(bad) == 0, [(int(k), str(g["cls"][k]), out[k].tolist(), want[k].tolist()) for k in bad[:5]]
    host, expired = rh.host_mpr(g)
    assert expired == 0 and rh.same_bits(out, host).all()


# ------------------------------------------------------------------------------------------------------------ list order
def uv_sphere(radius, nu=16, nv=16):
    """a closed sphere of 2 nu (nv - 1) triangles: 16 x 16 -> 480 triangles, 1 440 hull vertices in element order"""
    tri = []
    pt = lambda i, j: radius * np.array([np.sin(np.pi * j / nv) * np.cos(2 * np.pi * i / nu), np.cos(np.pi * j / nv),
                                         np.sin(np.pi * j / nv) * np.sin(2 * np.pi * i / nu)])
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = pt(i, j), pt(i + 1, j), pt(i + 1, j + 1), pt(i, j + 1)
            if j > 0:
                tri.append([a, b, c])
            if j < nv - 1:
                tri.append([a, c, d])
    return np.array(tri, F)


def quat_to_matrix_f32(q):
    """quat_to_matrix of the library's host code (rigid_api.h), operation by operation in float32"""
    w, x, y, z = (F(a) for a in q)
    one, two = F(1), F(2)
    return np.array([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                     two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                     two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], F).reshape(3, 3)


def eleven_bodies(tm, cfg):
    """ten boxes (8 distinct vertices each) and a sphere of 1 440 vertices, posed so that several overlap; bodies 3 and 7 follow
    scripts in position and rotation (their pair is skipped, their pairs with free bodies are not)"""
    rng = np.random.default_rng(11)
    sim = tm.create_simulation3("mpm").initialize(dict(res=(cs.RES,) * 3, delta_x=cs.DX, base_delta_t=cs.DT, max_particles=4096, **cfg))
    fric, rest, scripted = [0.0], [0.0], [0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for b in range(1, 12):
            pos = tuple(float(a) for a in rng.uniform(0.38, 0.62, 3))
            eul = tuple(float(a) for a in rng.uniform(-60, 60, 3))
            mesh = uv_sphere(0.09) if b == 5 else cs.box(*rng.uniform(0.03, 0.07, 3))
            f, e = float(rng.uniform(0.1, 0.8)), float(rng.uniform(0.0, 0.6))
            kw = dict(type="rigid", mesh=mesh, codimensional=False, density=float(rng.uniform(100, 600)), friction=f, restitution=e)
            if b in (3, 7):
                kw.update(scripted_position=lambda t, p=pos: p, scripted_rotation=lambda t, a=eul: a)
            else:
                kw.update(initial_position=pos, initial_rotation=eul, initial_velocity=tuple(rng.uniform(-1, 1, 3)),
                          initial_angular_velocity=tuple(rng.uniform(-3, 3, 3)))
            assert int(sim.add_particles(kw)) == b
            fric.append(f); rest.append(e); scripted.append(3 if b in (3, 7) else 0)
    x = (np.stack(np.meshgrid(*[np.arange(8, 11) + 0.5] * 3, indexing="ij"), -1).reshape(-1, 3) * cs.DX).astype(F)
    sim.add_particles(dict(type="jelly", positions=x))
    return sim, fric, rest, scripted


def host_state(sim, nb):
    states, hulls = [rh_background()], [None]
    for b in range(1, nb):
        st = sim.get_rigid_state(b)
        states.append(dict(pos=st["position"], vel=st["velocity"], omega=st["angular_velocity"], R=quat_to_matrix_f32(st["rotation"]),
                           inv_mass=st["inv_mass"], inv_I=st["inv_inertia"]))
        hulls.append(sim.get_rigid_hull(b))
    return states, hulls


def rh_background():
    return dict(pos=np.zeros(3, F), vel=np.zeros(3, F), omega=np.zeros(3, F), R=np.eye(3, dtype=F), inv_mass=0.0, inv_I=np.zeros((3, 3), F))


@pytest.mark.parametrize("env", [{}, {"MPMHIP_RIGID_WGS": "2"}, {"MPMHIP_RIGID_CONCURRENT": "0"}], ids=["default", "rigid_wgs_2", "one_stream"])
def test_collision_list_and_velocities_equal_the_host_build(tm, monkeypatch, env):
    """eleven bodies, rigidify() once: the collision list is the host build's, in (i, j) order whatever order the workgroups finish
    in, and every body's vel / omega equal the host build's bit for bit"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (read when the ctx is created)
    sim, fric, rest, scripted = eleven_bodies(tm, dict(rigid_body_collision=True))
    nb = sim.get_num_rigid_bodies()
    assert nb == 12 and len(sim.get_rigid_hull(5)) == 1440 and len(sim.get_rigid_hull(1)) == 36
    states, hulls = host_state(sim, nb)
    want_rows, want_v, want_w = rh.host_rigidify(states, scripted, hulls, fric, rest, dt=cs.DT)
    sim.rigidify()
    got = sim.get_rigid_collisions()
    rows = np.array([[c["i"], c["j"], c["depth"]] + list(c["normal"]) + list(c["position"]) for c in got], F).reshape(-1, 9)
    assert len(rows) == len(want_rows) >= 5, (len(rows), len(want_rows))
    pairs = [(int(r[0]), int(r[1])) for r in rows]
    assert pairs == sorted(pairs) and all(i > j >= 1 for i, j in pairs) and (7, 3) not in pairs
    assert any(5 in p for p in pairs), "the large hull has to take part"
    assert rh.same_bits(rows, want_rows).all(), (rows, want_rows)
    moved = 0
    for b in range(1, nb):
        st = sim.get_rigid_state(b)
        assert rh.same_bits(st["velocity"], want_v[b]).all() and rh.same_bits(st["angular_velocity"], want_w[b]).all(), b
        moved += int(not np.array_equal(st["velocity"], states[b]["vel"]))
    assert moved >= 4
    sim.close()


# -------------------------------------------------------------------------------------------------------------- behaviour
PLATFORM_Y, PLATFORM_HALF, BOX_HALF, GAP = 0.4, 0.01, 0.02, 0.002


def platform_scene(tm, cfg, v0=-1.0):
    """a scripted platform box, a free box released just above it, a handful of jelly particles far away"""
    sim = tm.create_simulation3("mpm").initialize(dict(res=(cs.RES,) * 3, delta_x=cs.DX, base_delta_t=cs.DT, gravity=(0, -10, 0),
                                                       max_particles=4096, **cfg))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        plat = int(sim.add_particles(dict(type="rigid", mesh=cs.box(0.12, PLATFORM_HALF, 0.12), codimensional=False, friction=0.5,
                                          scripted_position=lambda t: (0.6, PLATFORM_Y, 0.6), scripted_rotation=lambda t: (0.0, 0.0, 0.0))))
        box = int(sim.add_particles(dict(type="rigid", mesh=cs.box(BOX_HALF, BOX_HALF, BOX_HALF), codimensional=False, density=400.0, friction=0.5,
                                         initial_position=(0.6, PLATFORM_Y + PLATFORM_HALF + BOX_HALF + GAP, 0.6), initial_velocity=(0.0, v0, 0.0))))
    x = (np.stack(np.meshgrid(*[np.arange(8, 11) + 0.5] * 3, indexing="ij"), -1).reshape(-1, 3) * cs.DX).astype(F)
    sim.add_particles(dict(type="jelly", positions=x))
    return sim, plat, box


def test_a_free_box_rests_on_a_scripted_platform(tm):
    """600 substeps of 1e-4 s: free fall alone would carry the box 0.078 below its start — through the 0.02-thick platform.
    With the pass its lowest vertex stays above the platform's mid-plane and it has come to rest (its downward speed is below
    what free fall gains in a tenth of the run); without the key the box ends below the platform: the default is unchanged."""
    steps = 600
    sim, plat, box = platform_scene(tm, dict(rigid_body_collision=True))
    sim.run_substeps(steps)
    lowest = sim.get_rigid_mesh(box)[..., 1].min()
    st = sim.get_rigid_state(box)
    assert len(sim.get_rigid_collisions()) == 1
    sim.close()
    assert lowest > PLATFORM_Y, lowest
    assert -st["velocity"][1] < 0.1 * 10.0 * steps * cs.DT, st["velocity"]
    sim, plat, box = platform_scene(tm, dict())
    sim.run_substeps(steps)
    highest = sim.get_rigid_mesh(box)[..., 1].max()
    st = sim.get_rigid_state(box)
    assert sim.get_rigid_collisions() == []
    sim.close()
    assert highest < PLATFORM_Y - PLATFORM_HALF, highest
    # nothing but gravity: 600 float32 additions of g dt to a value below 2, each rounded by at most half an ulp of 2 (2^-23)
    np.testing.assert_allclose(st["velocity"], (0.0, -1.0 - 10.0 * steps * cs.DT, 0.0), atol=steps * 2.0 ** -23)


# --------------------------------------------------------------------------------------------------------------- settings
def two_overlapping_boxes(tm, cfg, scripted=False):
    sim = tm.create_simulation3("mpm").initialize(dict(res=(cs.RES,) * 3, delta_x=cs.DX, base_delta_t=cs.DT, max_particles=4096, **cfg))
    ids = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for p, v in (((0.5, 0.5, 0.5), (0.5, 0.0, 0.0)), ((0.56, 0.52, 0.5), (-0.5, 0.1, 0.0))):
            kw = dict(type="rigid", mesh=cs.box(0.05, 0.05, 0.05), codimensional=False, density=400.0, friction=0.3)
            if scripted:
                kw.update(scripted_position=lambda t, p=p: p, scripted_rotation=lambda t: (0.0, 10.0, 0.0))
            else:
                kw.update(initial_position=p, initial_velocity=v, initial_rotation=(0.0, 10.0, 0.0))
            ids.append(int(sim.add_particles(kw)))
    x = (np.stack(np.meshgrid(*[np.arange(8, 11) + 0.5] * 3, indexing="ij"), -1).reshape(-1, 3) * cs.DX).astype(F)
    sim.add_particles(dict(type="jelly", positions=x))
    return sim, ids


def test_zero_iterations_detect_but_leave_the_velocities(tm):
    sim, ids = two_overlapping_boxes(tm, dict(rigid_body_collision=True, rigid_body_iterations=0))
    before = [sim.get_rigid_state(b) for b in ids]
    sim.rigidify()
    assert [(c["i"], c["j"]) for c in sim.get_rigid_collisions()] == [(2, 1)]
    for b, s0 in zip(ids, before):
        s1 = sim.get_rigid_state(b)
        assert np.array_equal(s1["velocity"], s0["velocity"]) and np.array_equal(s1["angular_velocity"], s0["angular_velocity"])
    sim.close()
    # ... and with the default five the same pair does get its impulses; without position iterations and penalty they differ
    results = []
    for cfg in (dict(), dict(rigid_body_position_iterations=False), dict(rigid_penalty=1e5)):
        sim, ids = two_overlapping_boxes(tm, dict(rigid_body_collision=True, **cfg))
        sim.rigidify()
        results.append(np.concatenate([sim.get_rigid_state(b)["velocity"] for b in ids]))
        sim.close()
    assert not np.array_equal(results[0][:3], before[0]["velocity"])
    assert not np.array_equal(results[0], results[1]) and not np.array_equal(results[0], results[2])


def test_two_fully_scripted_bodies_give_an_empty_list(tm):
    sim, ids = two_overlapping_boxes(tm, dict(rigid_body_collision=True), scripted=True)
    sim.rigidify()
    assert sim.get_rigid_collisions() == []
    sim.run_substeps(2)
    assert sim.get_rigid_collisions() == []
    sim.close()


def test_a_snapshot_restart_continues_bit_equal_and_buffers_balance(tm, tmp_path):
    """50 substeps into the contact, a snapshot, 50 more; a second simulation built WITHOUT the keys loads the snapshot — the four
    settings travel in it — and its 50 substeps end in the same bits.  Every device buffer of the pass is gone after close()."""
    L = tm.load()
    live0 = L.mpmhip_debug_live_buffers()
    keys = dict(rigid_body_collision=True, rigid_body_iterations=3, rigid_penalty=2e3, rigid_body_position_iterations=True)
    sim, plat, box = platform_scene(tm, keys, v0=-2.0)
    sim.run_substeps(50)
    path = str(tmp_path / "contact.snap")
    sim.save_snapshot(path)
    sim.run_substeps(50)
    assert len(sim.get_rigid_collisions()) == 1
    want = cs.rigid_vector(sim.get_rigid_state(box))
    sim.close()
    sim, plat, box = platform_scene(tm, dict(), v0=-2.0)
    sim.load_snapshot(path)
    sim.run_substeps(50)
    got = cs.rigid_vector(sim.get_rigid_state(box))
    assert len(sim.get_rigid_collisions()) == 1
    sim.close()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    assert L.mpmhip_debug_live_buffers() == live0


def test_the_pass_is_refused_where_no_bodies_are(tm):
    with pytest.raises(tm.mpm.MPMError, match="rigid_body_collision"):
        tm.create_simulation2("mpm").initialize(dict(res=(32, 32), rigid_body_collision=True))
    with pytest.raises(tm.mpm.MPMError, match="rigid_body_collision"):
        tm.create_simulation3("async_mpm").initialize(dict(res=(32,) * 3, rigid_body_collision=True))


# ----------------------------------------------------------------------------------------------------------- cost when off
def test_a_scene_without_the_pass_runs_what_it_ran_before(tm):
    """a paddle wheel in sand, one substep: a run that never touches the new entry points against a run that calls them with the
    pass off (set_rigid_collision(0, ...), rigidify()) — the same launch plan, the same bits"""
    from tests.common import lattice_cube
    from tests.test_gpu_cpic import paddle
    res, dx = 64, 1.0 / 64
    x = lattice_cube(res, 24, 40, dx, jitter=0.15, seed=5)

    def run(touch):
        sim = tm.create_simulation3("mpm").initialize(dict(res=(res,) * 3, delta_x=dx, base_delta_t=1e-4, gravity=(0, -10, 0),
                                                           max_particles=len(x) + 16, deterministic=True))
        sim.add_particles(dict(type="rigid", mesh=paddle(0.2, 0.15), codimensional=True, friction=-2,
                               scripted_position=lambda t: (0.5, 0.5, 0.5), scripted_rotation=lambda t: (0.0, 0.0, 720.0 * t)))
        sim.add_particles(dict(type="sand", positions=x))
        if touch:
            sim._check(sim._L.mpmhip_set_rigid_collision(sim._ctx, 0, 5, 1e3, 1))
            sim.rigidify()
            assert sim.get_rigid_collisions() == []
        plan = sim.transfer_kernels()
        sim.substep()
        p = sim.get_particles(sort_by_id=True)
        sim.close()
        return plan, p
    (plan_a, a), (plan_b, b) = run(False), run(True)
    assert plan_a == plan_b
    assert (a["states"] != 0).sum() > 100, "the scene must colour particles"
    for k in ("x", "v", "F"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
