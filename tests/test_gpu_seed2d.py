"""mpmhip2d_seed_particles / Simulation2D.add_particles(region=...) (include/mpmhip.h): particles seeded on the device from the 2D
periodic Poisson-disk tile against the numpy model of the call (tests/seed2d_model.py).  Once the tile is fixed the call is a pure
function of its inputs, so the tests ask for the exact set and order of particles: bit for bit where the region is a sampled field
(the sampler forbids contraction, the model restates it), and for shapes after the candidates with |phi| < 1e-4 grid units are set
aside (the device's compiler may contract the multiply-adds of a shape's distance; 1e-4 cells is three orders above the rounding of
phi, ~1e-7 * 12).  Setup (tests/test_seed2d_cpu.py): res 64^2, dx = 1/64, ppc 4: the tile is 16.33 dx wide — 2 x 2 replicas for a disc
of r = 12 dx (4 * 997 candidates: four workgroups, the last one partial), one for r = 4 dx."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.seed2d_model import SampledRegion2D, SeedModel2D, ShapeRegion2D, load_tile
from tests.test_seed2d_cpu import DT, DX, MARGIN, PPC, R12, RES, SHAPES

pytestmark = pytest.mark.gpu
EINVAL, ECAPACITY = -1, -4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP_SRC = os.path.join(ROOT, "tests", "cpp", "seed2d_host_layer.cpp")
CPP_OUT = os.path.join(ROOT, "tests", "cpp", "_build", "seed2d_host_layer")


def build_cpp():
    """tests/cpp/seed2d_host_layer.cpp against include/mpm_amd/mpm2d.h and the library (__graft_entry__.build() calls this too)"""
    from taichi_mpm_amd import _lib
    lib = _lib.build()
    os.makedirs(os.path.dirname(CPP_OUT), exist_ok=True)
    inc = os.path.join(ROOT, "include")
    deps = [CPP_SRC, os.path.join(inc, "mpm_amd", "mpm2d.h"), os.path.join(inc, "mpm_amd", "mpm.h"), os.path.join(inc, "mpmhip.h"), lib]
    if not os.path.exists(CPP_OUT) or any(os.path.getmtime(d) > os.path.getmtime(CPP_OUT) for d in deps):
        libdir = os.path.dirname(lib)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", inc, CPP_SRC, "-o", CPP_OUT,
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
    return tm.create_simulation2("mpm").initialize(dict(res=(RES, RES), delta_x=DX, base_delta_t=DT, **cfg))


def seeded(sim):
    """positions and ids in creation order (slot order: the 2D arrays never move a row)"""
    p = sim.get_particles(sort_by_id=False)
    return p["x"], p["id"]


def sampled_disc(tm, centre=(0.5, 0.5), r=R12):
    """the disc baked on a lattice of spacing dx / 2 that is not aligned with the grid"""
    origin = tuple(np.float32(c - 14.3 * DX + 0.0137 * DX) for c in centre)
    c = np.asarray(centre, np.float64)
    return tm.SampledLevelSet2D.from_function(lambda x: np.linalg.norm(x - c, axis=1) - r, (60, 60), origin, DX / 2)


def sampled_model(sls, tile, **kw):
    return SeedModel2D(RES, DX, SampledRegion2D(sls.phi, sls.origin, sls.spacing, DX), ppc=PPC, tile=tile, base_dt=DT, **kw)


def shape_model(shapes, tile, **kw):
    return SeedModel2D(RES, DX, ShapeRegion2D(shapes, DX), ppc=PPC, tile=tile, base_dt=DT, **kw)


def levelset(tm, shapes):
    ls = tm.mpm.LevelSet()
    for s in shapes:
        ls._add(*s)
    return ls


@pytest.fixture(scope="module")
def centre_disc(tm, tile):
    """the sampled r = 12 dx disc at the centre, its model and the model's result, shared and left unchanged"""
    sls = sampled_disc(tm)
    m = sampled_model(sls, tile)
    return sls, m, m.run()


def test_sampled_region_exact(tm, centre_disc):
    sls, m, want = centre_disc
    assert tuple(m.nrep) == (2, 2) and want["n_cand"] == 4 * len(m.tile)
    assert (want["n_cand"] + 1023) // 1024 == 4 and want["n_cand"] % 1024 != 0  # four workgroups, the last one partial
    sim = make_sim(tm)
    sim.add_particles(dict(type="sand", region=sls, ppc=PPC))
    p = sim.get_particles(sort_by_id=False)
    sim.close()
    x = p["x"]
    print("sampled disc: %d candidates, %d survivors (model %d)" % (want["n_cand"], len(x), len(want["x"])))
    assert x.shape == want["x"].shape and x.tobytes() == want["x"].tobytes()
    assert np.array_equal(p["id"], np.arange(len(x))) and not p["gid"].any()
    assert not p["v"].any() and not p["B"].any() and not p["aux"].any()  # (sand's default aux is 0)
    assert np.array_equal(p["F"], np.tile(np.eye(2, dtype=np.float32).reshape(1, 4), (len(x), 1)))


def _strip(x, unsure_x):
    """rows of x whose bytes are not among unsure_x"""
    key = lambda a: np.ascontiguousarray(a, np.float32).view(np.dtype((np.void, 8))).reshape(-1)
    return x[~np.isin(key(x), key(unsure_x))]


def check_against_model(m, want, x):
    """the device's positions x against the model's result `want` (run with margin=MARGIN), the unsure candidates set aside"""
    unsure = want["unsure"]
    assert len(unsure) <= 0.01 * want["n_cand"]
    allx = m.positions()
    got, ref = _strip(x, allx[unsure]), want["x"][~np.isin(want["c"], unsure)]
    assert abs(len(x) - len(want["x"])) <= len(unsure)
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes()


@pytest.mark.parametrize("name", ["disc_r12", "box", "disc_r4", "inside_out_disc"])
def test_shape_regions(tm, tile, name):
    shapes, nrep = SHAPES[name]
    m = shape_model(shapes, tile)
    want = m.run(margin=MARGIN)
    assert tuple(m.nrep) == nrep
    sim = make_sim(tm)
    sim.add_particles(dict(type="sand", region=levelset(tm, shapes), ppc=PPC))
    x, ids = seeded(sim)
    sim.close()
    print("%s: %d candidates, %d unsure, device %d, model %d" % (name, want["n_cand"], len(want["unsure"]), len(x), len(want["x"])))
    assert len(x) > 0 and np.array_equal(ids, np.arange(len(x)))
    check_against_model(m, want, x)
    if name == "inside_out_disc":  # the region reaches every wall: the 7-cell margin is what bounds the particles
        X = x * np.float32(RES)
        assert X.min() >= 7.0 and X.max() <= RES - 7.0 and X.min() < 7.5 and X.max() > RES - 7.5


def test_wall_margin(tm, tile):
    """a box reaching x = 0.05, 3.2 cells from the wall: what lies within 7 cells of the wall is rejected"""
    shapes, nrep = SHAPES["wall_box"]
    m = shape_model(shapes, tile)
    want = m.run(margin=MARGIN)
    assert tuple(m.nrep) == nrep
    assert (m.positions()[:, 0] * np.float32(RES) < 7.0).any()  # candidates do fall into the margin
    sim = make_sim(tm)
    sim.add_particles(dict(type="sand", region=levelset(tm, shapes), ppc=PPC))
    x, _ = seeded(sim)
    sim.close()
    assert len(x) > 0 and (x[:, 0] * np.float32(RES)).min() >= 7.0
    check_against_model(m, want, x)


SOURCE_BOX = [(2, 0, [0.25, 0.6, 0.0, 0.75, 0.62, 0.0])]


def test_emitter(tm, tile):
    """a slot pouring water downwards: the call before each of 5 frames fills the strip the jet vacates within delta_t; the new
    particles are the model's, the model fed the clock and base_delta_t of the run"""
    vel, delta_t = (0.0, -1.0), 1e-3
    sim = make_sim(tm)
    cfg = dict(type="water", region=levelset(tm, SOURCE_BOX), ppc=PPC, pd_source=True, delta_t=delta_t, initial_velocity=vel)
    total = 0
    for frame in range(5):
        t = sim.get_current_time()
        m = shape_model(SOURCE_BOX, tile, velocity=vel, source=True, delta_t=delta_t, current_t=np.float32(t))
        want = m.run(margin=MARGIN)
        sim.add_particles(cfg)
        p = sim.get_particles(sort_by_id=False)
        x, ids = p["x"][total:], p["id"][total:]
        print("frame %d at t = %.7f: %d new particles (model %d, %d unsure)" % (frame, t, len(x), len(want["x"]), len(want["unsure"])))
        assert len(x) > 0  # the total grows every frame
        assert len(x) < 0.2 * len(shape_model(SOURCE_BOX, tile).run()["x"])  # a strip, not the box
        assert np.array_equal(ids, np.arange(total, total + len(x)))
        check_against_model(m, want, x)
        assert np.array_equal(p["v"][total:], np.tile(np.asarray(vel, np.float32), (len(x), 1)))
        assert np.all(p["aux"][total:] == 1.0) and not p["gid"].any()  # (water's default; one group row serves every call)
        total += len(x)
        assert sim.get_num_particles() == total
        sim.step(1e-3)
    assert sim.get_current_time() > 4e-3
    sim.close()


def _host_points(n, seed):
    """n points well inside the grid, away from the centre disc's rows only in what the tests compare"""
    rng = np.random.default_rng(seed)
    return (0.2 + 0.6 * rng.random((n, 2))).astype(np.float32)


def _fields(sim):
    return sim.get_particles(sort_by_id=False)


def test_capacity(tm, centre_disc):
    sls, _, want = centre_disc
    n_want, n_host = len(want["x"]), 300
    sim = make_sim(tm, max_particles=1024)  # (the wrapper adds its own head room: 1.5 * 300 + 1024 slots)
    sim.add_particles(dict(type="jelly", positions=_host_points(n_host, 1)))
    sim._ensure_ctx()
    assert n_host + n_want > sim._capacity
    params, mat = tm.materials.group_params("sand", 1.0, 1.0)
    gi = sim._check(sim._L.mpmhip2d_add_group(sim._ctx, mat, params.ctypes.data_as(C.POINTER(C.c_float))))
    sim._groups.append((mat, params))
    before = _fields(sim)
    d, keep = sim._seed_desc(dict(region=sls), "sand", PPC)
    n = C.c_int64(-1)
    assert sim._L.mpmhip2d_seed_particles(sim._ctx, gi, C.byref(d), C.byref(n)) == ECAPACITY
    assert b"capacity exceeded" in sim._L.mpmhip2d_last_error(sim._ctx)
    assert n.value == n_want  # the needed count
    assert sim._L.mpmhip2d_num_slots(sim._ctx) == n_host and sim.get_num_particles() == n_host  # nothing was written
    same = _fields(sim)
    assert all(before[k].tobytes() == same[k].tobytes() for k in before)
    assert sim._L.mpmhip2d_reserve(sim._ctx, 64) == 0  # (a capacity that already suffices)
    assert sim._L.mpmhip2d_reserve(sim._ctx, n_host + n_want) == 0
    assert sim._L.mpmhip2d_seed_particles(sim._ctx, gi, C.byref(d), C.byref(n)) == 0 and n.value == n_want
    after = _fields(sim)
    sim.close()
    assert len(after["id"]) == n_host + n_want
    assert all(before[k].tobytes() == after[k][:n_host].tobytes() for k in before)  # the earlier particles, bit for bit
    assert after["x"][n_host:].tobytes() == want["x"].tobytes()
    assert np.array_equal(after["id"], np.arange(n_host + n_want)) and np.all(after["gid"][n_host:] == gi)


def test_python_grows_by_itself_and_ids_follow_call_order(tm, centre_disc):
    """positions= (staged before the ctx exists), region=, positions=: the ctx of 1024 slots is grown by the seeding call, and the
    creation ids follow the order of the calls"""
    sls, _, want = centre_disc
    n_want = len(want["x"])
    a, b = _host_points(200, 2), _host_points(100, 3)
    sim = make_sim(tm, max_particles=1024)
    sim.add_particles(dict(type="jelly", positions=a))
    assert sim._ctx is None  # staged
    sim.add_particles(dict(type="sand", region=sls, ppc=PPC))
    assert sim._capacity >= 200 + n_want  # (created for 1324 slots)
    sim.add_particles(dict(type="jelly", positions=b))
    p = sim.get_particles(sort_by_id=False)
    sim.close()
    assert len(p["id"]) == 300 + n_want > 1324
    assert np.array_equal(p["id"], np.arange(300 + n_want))
    assert p["x"][:200].tobytes() == a.tobytes() and p["x"][200 + n_want:].tobytes() == b.tobytes()
    assert p["x"][200:200 + n_want].tobytes() == want["x"].tobytes()
    assert np.array_equal(p["gid"], np.repeat([0, 1, 2], [200, n_want, 100]))


def test_seeded_disc_steps_in_both_modes(tm, centre_disc):
    """the seeded disc of sand over a floor line, 50 substeps: the default mode and the deterministic one (whose per-particle arrays
    are sized after the seeding call grew the ctx); two deterministic runs are bitwise equal"""
    sls, _, want = centre_disc

    def run(**cfg):
        sim = make_sim(tm, max_particles=1024, **cfg)
        sim.set_levelset(tm.mpm.LevelSet(friction=0.4).add_plane((0, 1, 0), d=-0.3))
        sim.add_particles(dict(type="sand", region=sls, ppc=PPC, initial_velocity=(0.0, -1.0)))
        sim.run_substeps(50)
        out = sim.get_particles()
        sim.close()
        assert len(out["id"]) == len(want["x"])
        assert all(np.isfinite(out[k]).all() for k in ("x", "v", "F", "B", "aux"))
        assert np.abs(out["x"] - want["x"]).max() > 1e-4  # it moved
        return out
    run()
    a, b = run(deterministic=True), run(deterministic=True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_refusals(tm, centre_disc):
    sls = centre_disc[0]
    MPMError = tm.mpm.MPMError
    sim = make_sim(tm)
    L = sim._L

    def call(d, group=0):
        n = C.c_int64(0)
        return sim._check(L.mpmhip2d_seed_particles(sim._ctx, group, C.byref(d), C.byref(n)))
    # a disc smaller than a cell, between the cell centres (the nearest is 0.71 dx away)
    tiny = tm.mpm.LevelSet().add_sphere((0.5, 0.5, 0.0), 0.4 * DX)
    with pytest.raises(MPMError, match="region is empty"):
        sim.add_particles(dict(type="sand", region=tiny, ppc=PPC))
    with pytest.raises(MPMError, match="ppc must be"):
        sim.add_particles(dict(type="sand", region=sls, ppc=0))
    for bad, msg in ((dict(pd=False), "periodic Poisson-disk tile only"), (dict(pd_periodic=False), "periodic Poisson-disk tile only"),
                     (dict(pd_packed=True), "does not take 'pd_packed'"), (dict(velocities=np.zeros((4, 2))), "does not take 'velocities'"),
                     (dict(region=object()), "takes a LevelSet or a SampledLevelSet2D")):
        with pytest.raises(MPMError, match=msg):
            sim.add_particles(dict(dict(type="sand", region=sls, ppc=PPC), **bad))
    with pytest.raises(MPMError, match="region for add_particles"):
        sim.set_levelset(sls)
    assert sim.get_num_particles() == 0

    def desc():
        return sim._seed_desc(dict(region=sls), "sand", PPC)
    with pytest.raises(MPMError, match="unknown group 99"):
        call(desc()[0], 99)
    for field, value, msg in (("ppc", 0.0, "ppc must be"), ("ppc", -1.0, "ppc must be"), ("ppc", float("nan"), "ppc must be"),
                              ("ppc", float("inf"), "ppc must be"), ("initial_dg", float("nan"), "initial_dg is not finite")):
        d, keep = desc()
        setattr(d, field, value)
        with pytest.raises(MPMError, match=msg):
            call(d)
    d, keep = desc()
    d.velocity[1] = float("inf")
    with pytest.raises(MPMError, match=r"velocity\[1\] is not finite"):
        call(d)
    d, keep = desc()
    d.source, d.source_delta_t = 1, float("inf")
    with pytest.raises(MPMError, match="source_delta_t is not finite"):
        call(d)
    d, keep = desc()
    keep[0].res[1] = 1
    with pytest.raises(MPMError, match=r"res\[1\] = 1, at least 2 samples"):
        call(d)
    d, keep = desc()
    keep[0].origin[0] = float("nan")
    with pytest.raises(MPMError, match=r"origin\[0\] is not finite"):
        call(d)
    for spacing in (0.0, -1.0, float("inf")):
        d, keep = desc()
        keep[0].spacing = spacing
        with pytest.raises(MPMError, match="spacing must be a finite number > 0"):
            call(d)
    d, keep = desc()
    d.phi = None
    with pytest.raises(MPMError, match="needs its phi array"):
        call(d)
    d, keep = desc()
    d.ppc = 1e12  # min_distance 8e-7 dx: 26 dx / (40 * 8e-7 dx) replicas per axis
    with pytest.raises(MPMError, match=r"more than 2\^31 candidates"):
        call(d)
    assert sim.get_num_particles() == 0 and L.mpmhip2d_num_slots(sim._ctx) == 0
    # creation ids: one host particle named 2^31 - 2 leaves room for one more id
    sim.add_particles(dict(type="sand", positions=_host_points(1, 4)))
    sim.upload_ids([2 ** 31 - 2])
    with pytest.raises(MPMError, match=r"creation ids exceed 2\^31"):
        sim.add_particles(dict(type="sand", region=sls, ppc=PPC))
    assert sim.get_num_particles() == 1
    sim.close()
    # a resident asynchronous stepper
    sim = make_sim(tm)
    sim._ensure_ctx()
    a = tm._lib.AsyncConfig(1e-6, 8192, 1.0, 1.0, 0)
    sim._check(L.mpmhip2d_async_begin(sim._ctx, C.byref(a)))
    with pytest.raises(MPMError, match="seed before mpmhip2d_async_begin"):
        sim.add_particles(dict(type="sand", region=sls, ppc=PPC))
    sim.close()


def test_buffers(tm, centre_disc):
    sls = centre_disc[0]
    L = tm.load()
    live0 = L.mpmhip_debug_live_buffers()
    sim = make_sim(tm, max_particles=1024)
    sim._ensure_ctx()
    created = L.mpmhip_debug_live_buffers()
    sim.add_particles(dict(type="sand", region=sls, ppc=PPC))
    assert L.mpmhip_debug_live_buffers() > created > live0  # the tile, the ballots, the totals, the box, the field
    grown = L.mpmhip_debug_live_buffers()
    sim.add_particles(dict(type="sand", region=sls, ppc=PPC))  # the work buffers are kept between calls
    assert L.mpmhip_debug_live_buffers() == grown
    sim.close()
    assert L.mpmhip_debug_live_buffers() == live0


def test_cpp_host_layer_seeds_the_same_particles(centre_disc, tmp_path):
    """MPM<2>::add_particles_region (include/mpm_amd/mpm2d.h) with the sampled disc on a ctx created for 1024 particles: it grows
    the ctx; the count and an order-sensitive checksum of the positions' bits are the model's"""
    sls, _, want = centre_disc
    path = tmp_path / "disc.f32"
    np.concatenate([np.asarray(sls.origin, np.float32), np.asarray([sls.spacing], np.float32), sls.phi.reshape(-1)]).tofile(str(path))
    r = subprocess.run([build_cpp(), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.split()
    b = want["x"].view(np.uint32).astype(np.uint64)
    check = np.sum((b[:, 0] + np.uint64(31) * b[:, 1]) * np.arange(1, len(b) + 1, dtype=np.uint64), dtype=np.uint64)
    assert int(f[0]) == len(want["x"]) > 1024 and int(f[1]) == int(f[0])
    assert int(f[2]) == int(check)
