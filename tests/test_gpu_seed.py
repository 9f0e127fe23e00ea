"""mpmhip_seed_particles / add_particles(region=...) (include/mpmhip.h): particles seeded on the device from the periodic Poisson-disk
tile against the numpy model of the call (tests/seed_model.py).  Once the tile is fixed the call is a pure function of its inputs, so
the tests ask for the exact set and order of particles: bit for bit where the region is a sampled field (the sampler forbids
contraction, the model restates it), and for shapes after the candidates with |phi| < 1e-4 grid units are set aside (the device's
compiler may contract the multiply-adds of a shape's distance; 1e-4 cells is three orders above the rounding of phi, ~1e-7 * 12).
Setup: res 64^3, dx = 1/64, ppc 8: the tile is 17.94 dx wide — 2 x 2 x 2 replicas for a sphere of r = 12 dx, one for r = 4 dx."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.seed_model import SampledRegion, SeedModel, ShapeRegion, load_tile

pytestmark = pytest.mark.gpu
RES, DX, DT, PPC = 64, 1.0 / 64, 1e-4, 8.0
R12, R4 = 12 * DX, 4 * DX
MARGIN = 1e-4  # grid units
ECAPACITY = -4


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP_SRC = os.path.join(ROOT, "tests", "cpp", "seed_host_layer.cpp")
CPP_OUT = os.path.join(ROOT, "tests", "cpp", "_build", "seed_host_layer")


def build_cpp():
    """tests/cpp/seed_host_layer.cpp against include/mpm_amd/mpm.h and the library (__graft_entry__.build() calls this too)"""
    from taichi_mpm_amd import _lib
    lib = _lib.build()
    os.makedirs(os.path.dirname(CPP_OUT), exist_ok=True)
    deps = [CPP_SRC, os.path.join(ROOT, "include", "mpm_amd", "mpm.h"), os.path.join(ROOT, "include", "mpmhip.h"), lib]
    if not os.path.exists(CPP_OUT) or any(os.path.getmtime(d) > os.path.getmtime(CPP_OUT) for d in deps):
        libdir = os.path.dirname(lib)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), CPP_SRC, "-o", CPP_OUT,
                               "-L", libdir, "-lmpmhip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib",
                               "-Wl,--allow-shlib-undefined"])
    return CPP_OUT


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


@pytest.fixture(scope="module")
def tile(tm):
    return load_tile()


def make_sim(tm, **cfg):
    return tm.create_simulation3("mpm").initialize(dict(res=(RES,) * 3, delta_x=DX, base_delta_t=DT, **cfg))


def seeded(sim):
    """positions and ids in creation order (slot order: nothing has moved a record yet)"""
    p = sim.get_particles(sort_by_id=False)
    return p["x"], p["id"]


def sampled_sphere(tm, centre, r=R12):
    """the sphere baked on a lattice of spacing dx / 2 that is not aligned with the grid"""
    origin = tuple(np.float32(c - 14.3 * DX + 0.0137 * DX) for c in centre)
    c = np.asarray(centre, np.float64)
    return tm.mpm.SampledLevelSet.from_function(lambda x: np.linalg.norm(x - c, axis=1) - r, (60, 60, 60), origin, DX / 2)


def sampled_model(sls, tile, **kw):
    return SeedModel(RES, DX, SampledRegion(sls.phi, sls.origin, sls.spacing, DX), ppc=PPC, tile=tile, base_dt=DT, **kw)


@pytest.fixture(scope="module")
def centre_sphere(tm, tile):
    """the sampled r = 12 dx sphere at the centre, its model and the model's result, shared and left unchanged"""
    sls = sampled_sphere(tm, (0.5, 0.5, 0.5))
    m = sampled_model(sls, tile)
    return sls, m, m.run()


def test_sampled_region_exact(tm, centre_sphere):
    sls, m, want = centre_sphere
    assert tuple(m.nrep) == (2, 2, 2) and want["n_cand"] == 8 * len(m.tile)
    sim = make_sim(tm)
    sim.add_particles(dict(type="sand", region=sls, ppc=PPC))
    x, ids = seeded(sim)
    v, F, aux = (sim.get_particles(sort_by_id=False)[k] for k in ("v", "F", "aux"))
    sim.close()
    print("sampled sphere: %d candidates, %d survivors (model %d)" % (want["n_cand"], len(x), len(want["x"])))
    assert x.shape == want["x"].shape and x.tobytes() == want["x"].tobytes()
    assert np.array_equal(ids, np.arange(len(x)))
    assert not v.any() and not aux.any() and np.array_equal(F, np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (len(x), 1)))


def _strip(x, unsure_x):
    """rows of x whose bytes are not among unsure_x"""
    key = lambda a: np.ascontiguousarray(a, np.float32).view(np.dtype((np.void, 12))).reshape(-1)
    return x[~np.isin(key(x), key(unsure_x))]


SHAPES = {
    "sphere_r12": ((1, 0, [0.5, 0.5, 0.5, R12, 0, 0]), (2, 2, 2)),
    "cuboid": ((2, 0, [0.3, 0.33, 0.28, 0.62, 0.52, 0.71]), (2, 1, 2)),
    "sphere_r4": ((1, 0, [0.5, 0.5, 0.5, R4, 0, 0]), (1, 1, 1)),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shape_regions(tm, tile, name):
    shape, nrep = SHAPES[name]
    m = SeedModel(RES, DX, ShapeRegion([shape], DX), ppc=PPC, tile=tile, base_dt=DT)
    want = m.run(margin=MARGIN)
    assert tuple(m.nrep) == nrep
    ls = tm.mpm.LevelSet()
    ls._add(*shape)
    sim = make_sim(tm)
    sim.add_particles(dict(type="sand", region=ls, ppc=PPC))
    x, ids = seeded(sim)
    sim.close()
    unsure = want["unsure"]
    print("%s: %d candidates, %d unsure, device %d, model %d" % (name, want["n_cand"], len(unsure), len(x), len(want["x"])))
    assert len(unsure) <= 0.005 * want["n_cand"]
    assert np.array_equal(ids, np.arange(len(x)))
    ux = np.concatenate([m.positions(int(c) // m.n_rep, int(c) // m.n_rep + 1)[int(c) % m.n_rep][None] for c in unsure]) if len(unsure) else np.zeros((0, 3), np.float32)
    got, ref = _strip(x, ux), want["x"][~np.isin(want["c"], unsure)]
    assert abs(len(x) - len(want["x"])) <= len(unsure)
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes()


def test_cpp_host_layer_seeds_the_same_particles(tile):
    """MPM<3>::add_particles_region (include/mpm_amd/mpm.h) on a ctx created for 1024 particles: it grows the ctx, and the count and
    the first particle are the model's (no candidate of this sphere is within the margin: test_shape_regions[sphere_r12] prints it)"""
    m = SeedModel(RES, DX, ShapeRegion([SHAPES["sphere_r12"][0]], DX), ppc=PPC, tile=tile, base_dt=DT)
    want = m.run(margin=MARGIN)
    r = subprocess.run([build_cpp()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.split()
    assert abs(int(f[0]) - len(want["x"])) <= len(want["unsure"]) and int(f[1]) == int(f[0])
    if not len(want["unsure"]):
        assert np.array_equal(np.array(f[2:5], np.float32), want["x"][0])


def test_near_wall_rejection(tm, tile, centre_sphere):
    """the sphere centred 16 dx from the -x wall reaches to 4 dx from it: what lies within 7 cells of the wall is rejected"""
    sls = sampled_sphere(tm, (16 * DX, 0.5, 0.5))
    m = sampled_model(sls, tile)
    want = m.run()["x"]
    whole = len(centre_sphere[2]["x"])
    sim = make_sim(tm)
    sim.add_particles(dict(type="sand", region=sls, ppc=PPC))
    x, _ = seeded(sim)
    sim.close()
    assert x.tobytes() == want.tobytes()
    assert (x[:, 0] * np.float32(RES)).min() >= 7.0
    assert 0.5 * whole < len(x) < 0.97 * whole  # a cap of the ball is missing, not the ball


def test_no_pair_closer_than_the_spacing_across_replicas(tm, centre_sphere):
    from scipy.spatial import cKDTree
    sls, m, _ = centre_sphere
    sim = make_sim(tm)
    sim.add_particles(dict(type="sand", region=sls, ppc=PPC))
    x, _ = seeded(sim)
    sim.close()
    d, _ = cKDTree(x.astype(np.float64)).query(x.astype(np.float64), k=2)
    print("nearest pair / min_distance = %.7f" % (d[:, 1].min() / float(m.min_distance)))
    assert d[:, 1].min() >= float(m.min_distance) * (1 - 1e-5)


def test_source_mode(tm, tile, centre_sphere):
    """an emitter: two calls, the clock advanced by delta_t in between.  Each fills the shell the jet vacates within delta_t; the
    tile drifts with the jet, so the first call's particles, moved on by velocity * delta_t (gravity 0), and the second call's keep
    the spacing"""
    from scipy.spatial import cKDTree
    sls = centre_sphere[0]
    vel, delta_t = (0.0, -2.0, 0.0), 1e-3
    kw = dict(velocity=vel, source=True, delta_t=delta_t, gravity=(0, 0, 0))
    m0, m1 = sampled_model(sls, tile, current_t=0.0, **kw), sampled_model(sls, tile, current_t=np.float32(delta_t), **kw)
    w0, w1 = m0.run()["x"], m1.run()["x"]
    sim = make_sim(tm, gravity=(0, 0, 0))
    cfg = dict(type="sand", region=sls, ppc=PPC, pd_source=True, delta_t=delta_t, initial_velocity=vel)
    sim.add_particles(cfg)
    x0, _ = seeded(sim)
    assert sim._L.mpmhip_set_time(sim._ctx, C.c_double(float(np.float32(delta_t)))) == 0
    sim.add_particles(cfg)
    x, ids = seeded(sim)
    v = sim.get_particles(sort_by_id=False)["v"]
    sim.close()
    x1 = x[len(x0):]
    print("source mode: %d + %d particles (model %d + %d)" % (len(x0), len(x1), len(w0), len(w1)))
    assert 0 < len(w0) < 0.05 * len(centre_sphere[2]["x"])  # a shell, not the ball
    assert x0.tobytes() == w0.tobytes() and x1.tobytes() == w1.tobytes()
    assert np.array_equal(ids, np.arange(len(x))) and np.array_equal(v, np.tile(np.asarray(vel, np.float32), (len(x), 1)))
    moved = (x0 + (np.asarray(vel, np.float32) * np.float32(delta_t))[None, :]).astype(np.float32)
    both = np.concatenate([moved, x1]).astype(np.float64)
    d, _ = cKDTree(both).query(both, k=2)
    assert d[:, 1].min() >= float(m0.min_distance) * (1 - 1e-5)


def test_bytes_and_buffers(tm, centre_sphere):
    sls = centre_sphere[0]
    L = tm.load()
    live0 = L.mpmhip_debug_live_buffers()
    sim = make_sim(tm)
    sim._ensure_ctx()
    before = L.mpmhip_host_particle_bytes(sim._ctx)
    sim.add_particles(dict(type="sand", region=sls, ppc=PPC))
    assert sim._L.mpmhip_num_slots(sim._ctx) == len(centre_sphere[2]["x"])
    assert L.mpmhip_host_particle_bytes(sim._ctx) == before
    assert L.mpmhip_debug_live_buffers() > live0
    sim.close()
    assert L.mpmhip_debug_live_buffers() == live0


def test_capacity(tm, centre_sphere):
    sls, _, want = centre_sphere
    sim = make_sim(tm, max_particles=1024)
    sim._ensure_ctx()
    params, mat = tm.materials.group_params("sand", 1.0, 1.0)
    gi = sim._check(sim._L.mpmhip_add_group(sim._ctx, mat, params.ctypes.data_as(C.POINTER(C.c_float))))
    sim._groups.append((mat, params))
    d, keep = sim._seed_desc(dict(region=sls), "sand", PPC)
    n = C.c_int64(-1)
    assert sim._L.mpmhip_seed_particles(sim._ctx, gi, C.byref(d), C.byref(n)) == ECAPACITY
    assert n.value == len(want["x"])  # the needed count
    assert sim.get_num_particles() == 0 and sim._L.mpmhip_num_slots(sim._ctx) == 0  # nothing was written
    sim.add_particles(dict(type="sand", region=sls, ppc=PPC))  # the wrapper reserves and calls again
    x, ids = seeded(sim)
    assert sim._L.mpmhip_capacity(sim._ctx) >= len(x) > 1024
    sim.close()
    assert x.tobytes() == want["x"].tobytes() and np.array_equal(ids, np.arange(len(x)))


def test_deterministic_mode_seeded_run_equals_the_uploaded_one(tm, centre_sphere):
    """sand on a plane, 20 substeps: a ctx seeded through region= and one given the model's positions through positions= agree in
    every particle field, bit for bit"""
    sls, _, want = centre_sphere

    def run(**how):
        sim = make_sim(tm, deterministic=True)
        sim.set_levelset(tm.mpm.LevelSet(friction=0.4).add_plane((0, 1, 0), d=-0.31))
        sim.add_particles(dict(type="sand", ppc=PPC, initial_velocity=(0.0, -3.0, 0.0), **how))
        sim.run_substeps(20)
        out = sim.get_particles()
        sim.close()
        return out
    a, b = run(region=sls), run(positions=want["x"])
    assert len(a["id"]) == len(want["x"])
    assert np.abs(a["x"] - want["x"]).max() > 1e-4  # it moved
    for f in ("id", "gid", "x", "v", "F", "B", "aux", "states"):
        assert a[f].tobytes() == b[f].tobytes(), f


def test_refusals(tm, centre_sphere):
    sls = centre_sphere[0]
    MPMError = tm.mpm.MPMError
    sim = make_sim(tm)
    # a sphere smaller than a cell, between the cell centres (the nearest is 0.87 dx away)
    tiny = tm.mpm.LevelSet().add_sphere((0.5, 0.5, 0.5), 0.4 * DX)
    with pytest.raises(MPMError, match="region is empty"):
        sim.add_particles(dict(type="sand", region=tiny, ppc=PPC))
    with pytest.raises(MPMError, match="ppc must be"):
        sim.add_particles(dict(type="sand", region=sls, ppc=0))
    d, keep = sim._seed_desc(dict(region=sls), "sand", PPC)
    n = C.c_int64(0)
    d.ppc = 0.0
    with pytest.raises(MPMError, match="ppc must be"):
        sim._check(sim._L.mpmhip_seed_particles(sim._ctx, 0, C.byref(d), C.byref(n)))
    d.ppc = PPC
    with pytest.raises(MPMError, match="unknown group 99"):
        sim._check(sim._L.mpmhip_seed_particles(sim._ctx, 99, C.byref(d), C.byref(n)))
    # min_distance 9e-5 dx and 9e-11 dx: 26 dx / (40 min_distance) = 7e3 and 7e9 replicas per axis, the latter more than an int holds
    for ppc in (1e12, 1e30):
        d.ppc = ppc
        with pytest.raises(MPMError, match=r"more than 2\^31 candidates"):
            sim._check(sim._L.mpmhip_seed_particles(sim._ctx, 0, C.byref(d), C.byref(n)))
        assert sim.get_num_particles() == 0
    d.ppc = PPC
    sim.add_particles(dict(type="sand", region=sls, ppc=PPC))  # (a substep needs particles)
    count = sim.get_num_particles()
    sim._check(sim._L.mpmhip_substep_begin(sim._ctx))
    with pytest.raises(MPMError, match="inside a substep"):
        sim.add_particles(dict(type="sand", region=sls, ppc=PPC))
    sim._check(sim._L.mpmhip_substep_end(sim._ctx))
    sim.synchronize()
    assert sim.get_num_particles() == count
    ip = C.POINTER(C.c_int32)
    dims, cx, cyz = np.array([2, 1, 1], np.int32), np.array([0, 32, 64], np.int32), np.array([0, 64], np.int32)
    sim._check(sim._L.mpmhip_set_partition(sim._ctx, 0, dims.ctypes.data_as(ip), cx.ctypes.data_as(ip), cyz.ctypes.data_as(ip),
                                           cyz.ctypes.data_as(ip), 2))
    with pytest.raises(MPMError, match="tiled ctx"):
        sim.add_particles(dict(type="sand", region=sls, ppc=PPC))
    sim.close()
