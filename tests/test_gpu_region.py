"""Region expressions in 3D (include/mpmhip.h, "Region expressions"; csrc/k_region.h) against the numpy model (tests/region_model.py):
the evaluator through Region.sample, the seeding through add_particles(region=<Region>), the baking through Region.to_sampled, the
refusals and the C++ host layer.  Where every leaf is a sampled field the device must match the model bit for bit (the sampler and
the placement forbid contraction; min, max and negation are exact).  Shape leaves go through levelset_eval_key, where the device's
compiler may contract a multiply and an add: candidates with a leaf value or a band-edge difference within MARGIN = 1e-4 grid units
are set aside (at most 0.5 % of them), the rest must match to the byte.
Setup as in tests/test_gpu_seed.py: res 64^3, dx = 1/64, ppc 8; lattices of 60 samples per axis, spacing dx / 2, off the grid."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.region_model import RegionModel
from tests.region_scenes import DX, R12, sampled_ball, sampled_scenes, shape_scenes
from tests.seed_model import SeedModel, load_tile

pytestmark = pytest.mark.gpu
RES, DT, PPC = 64, 1e-4, 8.0
MARGIN = 1e-4  # grid units
EINVAL, ECAPACITY = -1, -4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP_SRC = os.path.join(ROOT, "tests", "cpp", "region_host_layer.cpp")
CPP_OUT = os.path.join(ROOT, "tests", "cpp", "_build", "region_host_layer")


def build_cpp():
    """tests/cpp/region_host_layer.cpp against include/mpm_amd/mpm.h, mpm2d.h and the library (__graft_entry__.build() calls this)"""
    from taichi_mpm_amd import _lib
    lib = _lib.build()
    os.makedirs(os.path.dirname(CPP_OUT), exist_ok=True)
    inc = os.path.join(ROOT, "include")
    deps = [CPP_SRC, os.path.join(inc, "mpm_amd", "mpm.h"), os.path.join(inc, "mpm_amd", "mpm2d.h"), os.path.join(inc, "mpmhip.h"), lib]
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


@pytest.fixture(scope="module")
def sampled(tm):
    return sampled_scenes(tm, 3)


@pytest.fixture(scope="module")
def shapes(tm):
    return shape_scenes(tm, 3)


def model_of(region):
    return RegionModel.from_desc(region.compile(3, DX)[0], 3, DX)


def make_sim(tm, **cfg):
    return tm.create_simulation3("mpm").initialize(dict(res=(RES,) * 3, delta_x=DX, base_delta_t=DT, **cfg))


def seeded(sim):
    p = sim.get_particles(sort_by_id=False)
    return p["x"], p["id"]


def seed_model(region_model, tile, **kw):
    return SeedModel(RES, DX, region_model, ppc=PPC, tile=tile, base_dt=DT, **kw)


def _strip(x, unsure_x):
    key = lambda a: np.ascontiguousarray(a, np.float32).view(np.dtype((np.void, 12))).reshape(-1)
    return x[~np.isin(key(x), key(unsure_x))]


def check_with_margin(name, m, want, x, ids):
    """the device's particles against a model run with margin=MARGIN on the region's margin_view: the unsure candidates set aside"""
    unsure = want["unsure"]
    print("%s: %d candidates, %d unsure, device %d, model %d" % (name, want["n_cand"], len(unsure), len(x), len(want["x"])))
    assert len(unsure) <= 0.005 * want["n_cand"]
    assert np.array_equal(ids, np.arange(len(x)))
    ux = np.concatenate([m.positions(int(c) // m.n_rep, int(c) // m.n_rep + 1)[int(c) % m.n_rep][None] for c in unsure]) if len(unsure) else np.zeros((0, 3), np.float32)
    got, ref = _strip(x, ux), want["x"][~np.isin(want["c"], unsure)]
    assert abs(len(x) - len(want["x"])) <= len(unsure)
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes()


# ---------------------------------------------------------------------------------------------- 4. the evaluator
def _points():
    return np.random.default_rng(5).uniform(0.1, 0.9, (20000, 3)).astype(np.float32)


@pytest.mark.parametrize("name", ["a", "b"])
def test_evaluator_sampled_leaves_bit_for_bit(tm, sampled, name):
    region, x = sampled[name], _points()
    got, want = region.sample(x, DX), model_of(region).phi(x)[0]
    inf = np.isinf(want)
    print("program (%s): %d of %d points have no lattice (+-inf), %d inside" % (name, inf.sum(), len(x), (want < 0).sum()))
    assert inf.any() and (~inf).any() and (want < 0).any()
    if name == "a":
        assert np.all(want[inf] > 0)  # a - b outside the lattice: max(+inf, -inf)
    assert got.tobytes() == want.tobytes()


def test_evaluator_shape_leaves(tm, shapes):
    region, x = shapes["clipped_shell"][0], _points()
    m = model_of(region)
    got, want = region.sample(x, DX), m.phi(x)[0]
    err = np.abs(got - want).max()
    sure = m.closeness(x) > MARGIN
    print("program (c): max |device - model| = %.3g grid units, %d of %d points within the margin" % (err, (~sure).sum(), len(x)))
    assert err <= MARGIN
    assert np.array_equal((got < 0)[sure], (want < 0)[sure]) and (want < 0).any()


# ---------------------------------------------------------------------------------------------- 5. seeding, sampled leaves
@pytest.fixture(scope="module")
def sampled_runs(sampled, tile):
    """name -> (seeding model, its result), shared and left unchanged"""
    out = {}
    for name in ("a", "b"):
        m = seed_model(model_of(sampled[name]), tile)
        out[name] = (m, m.run())
    return out


@pytest.mark.parametrize("name,nrep", [("a", (2, 2, 2)), ("b", (2, 2, 1))])
def test_seeding_sampled_leaves_exact(tm, sampled, sampled_runs, name, nrep):
    m, want = sampled_runs[name]
    assert tuple(m.nrep) == nrep and want["n_cand"] == int(np.prod(nrep)) * len(m.tile)
    sim = make_sim(tm)
    sim.add_particles(dict(type="sand", region=sampled[name], ppc=PPC))
    x, ids = seeded(sim)
    v, F, aux = (sim.get_particles(sort_by_id=False)[k] for k in ("v", "F", "aux"))
    sim.close()
    print("program (%s): %d candidates, %d survivors (model %d)" % (name, want["n_cand"], len(x), len(want["x"])))
    assert x.shape == want["x"].shape and x.tobytes() == want["x"].tobytes()
    assert np.array_equal(ids, np.arange(len(x)))
    assert not v.any() and not aux.any() and np.array_equal(F, np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (len(x), 1)))


# ---------------------------------------------------------------------------------------------- 6. seeding, shape leaves
@pytest.mark.parametrize("name,nrep", [("clipped_shell", (2, 1, 2)), ("placed_boxes", (3, 1, 1)), ("ground_band", (2, 1, 2)),
                                       ("complement", (1, 1, 1))])
def test_seeding_shape_leaves(tm, tile, shapes, name, nrep):
    region = shapes[name][0]
    m = seed_model(model_of(region).margin_view(), tile)
    want = m.run(margin=MARGIN)
    assert tuple(m.nrep) == nrep
    sim = make_sim(tm)
    sim.add_particles(dict(type="sand", region=region, ppc=PPC))
    x, ids = seeded(sim)
    sim.close()
    check_with_margin(name, m, want, x, ids)
    assert len(x) > 5000


# ---------------------------------------------------------------------------------------------- 7. the emitter
def test_emitter_fills_only_the_vacated_shell(tm, tile, shapes):
    region = shapes["clipped_shell"][0]
    vel, delta_t, t = (0.0, -2.0, 0.0), 1e-3, np.float32(3e-3)
    m = seed_model(model_of(region).margin_view(), tile, velocity=vel, source=True, delta_t=delta_t, current_t=t, gravity=(0, 0, 0))
    want = m.run(margin=MARGIN)
    whole = seed_model(model_of(region), tile).run()
    sim = make_sim(tm, gravity=(0, 0, 0))
    sim._ensure_ctx()
    assert sim._L.mpmhip_set_time(sim._ctx, C.c_double(float(t))) == 0
    sim.add_particles(dict(type="sand", region=region, ppc=PPC, pd_source=True, delta_t=delta_t, initial_velocity=vel))
    x, ids = seeded(sim)
    v = sim.get_particles(sort_by_id=False)["v"]
    sim.close()
    check_with_margin("emitter", m, want, x, ids)
    assert 0 < len(want["x"]) < 0.1 * len(whole["x"])  # a shell, not the body
    assert np.array_equal(v, np.tile(np.asarray(vel, np.float32), (len(x), 1)))


# ---------------------------------------------------------------------------------------------- 8. a plain region
def test_a_plain_region_and_its_expression_seed_the_same_bytes(tm):
    """region=sls and region=Region(sls) give byte-identical particles.  (A seeding call reports no kernel forms — only the
    asynchronous steppers do, mpmhip_async_forms — so that the plain call launches the kernels it launched is held by
    profiles/kernel_diff.py against the parent's library, recorded in profiles/seed_ab.txt, and by
    tests/test_region_resources_cpu.py, which finds the SeedRegion / SeedRegion2 instantiations beside the new ones.)"""
    sls = sampled_ball(tm, (0.5, 0.5, 0.5), R12)
    out = []
    for region in (sls, tm.mpm.Region(sls)):
        sim = make_sim(tm)
        sim.add_particles(dict(type="sand", region=region, ppc=PPC))
        p = sim.get_particles(sort_by_id=False)
        sim.close()
        out.append(p)
    assert len(out[0]["x"]) > 20000
    for k in ("x", "v", "F", "aux", "id", "gid"):
        assert out[0][k].tobytes() == out[1][k].tobytes(), k


# ---------------------------------------------------------------------------------------------- 9. baking
def test_to_sampled_matches_the_model_at_every_node(tm, sampled):
    region = sampled["a"]
    res, origin, spacing = (40, 40, 40), (0.2631, 0.2877, 0.3012), np.float32(DX * 0.55)  # (two planes of nodes lie outside the leaves' lattice)
    band = 3.0 * DX + 2.0 * float(spacing)
    got = region.to_sampled(res, origin, float(spacing), delta_x=DX)
    want = model_of(region).bake(res, np.asarray(origin, np.float32), spacing, np.float32(band))
    assert isinstance(got, tm.mpm.SampledLevelSet) and got.phi.shape == res
    print("baked: %d nodes, %d clamped, %d inside" % (want.size, (np.abs(want) == np.float32(band)).sum(), (want < 0).sum()))
    assert (want < 0).any() and (np.abs(want) == np.float32(band)).any() and np.all(np.isfinite(got.phi))
    assert got.phi.tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------- 10. refusals, capacity, buffers
def _group(tm, sim):
    sim._ensure_ctx()
    params, mat = tm.materials.group_params("sand", 1.0, 1.0)
    gi = sim._check(sim._L.mpmhip_add_group(sim._ctx, mat, params.ctypes.data_as(C.POINTER(C.c_float))))
    sim._groups.append((mat, params))
    return gi


def _spoil(tm, shapes, sampled):
    """(what the message must hold, the description with one fault) for every refusal of the check"""
    def shape_desc():
        return shapes["clipped_shell"][0].compile(3, DX)
    def placed_desc():
        return shapes["placed_boxes"][0].compile(3, DX)
    def band_desc():
        return shapes["ground_band"][0].compile(3, DX)
    def field_desc():
        return sampled["a"].compile(3, DX)
    L = tm._lib
    cases = []
    def case(msg, make, change):
        d, keep = make()
        change(d)
        cases.append((msg, d, keep))
    case("leaf index 3 out of range", shape_desc, lambda d: setattr(d.ops[1], "leaf", 3))
    case("field index 2 out of range", field_desc, lambda d: setattr(d.leaves[1], "field", 2))
    case("stack underflow", shape_desc, lambda d: setattr(d.ops[0], "op", L.REGION_UNION))
    def deep(d):
        for i in range(5):
            d.ops[i].op, d.ops[i].leaf = L.REGION_PUSH, 0
        for i in range(5, 9):
            d.ops[i].op = L.REGION_UNION
        d.n_ops = 9
    case("stack depth above 4", shape_desc, deep)
    case("leaves 2 values on the stack", shape_desc, lambda d: setattr(d, "n_ops", d.n_ops - 1))
    case("the program is empty", shape_desc, lambda d: setattr(d, "n_ops", 0))
    case("unknown opcode 7", shape_desc, lambda d: setattr(d.ops[2], "op", 7))
    case("rotation is not finite", placed_desc, lambda d: d.leaves[0].rot.__setitem__(4, float("nan")))
    case("rotation is not orthonormal", placed_desc, lambda d: d.leaves[0].rot.__setitem__(0, 1.5))
    case("scale must be", placed_desc, lambda d: setattr(d.leaves[0], "scale", 0.0))
    case("scale must be", placed_desc, lambda d: setattr(d.leaves[0], "scale", float("inf")))
    case("lo < hi", band_desc, lambda d: [setattr(d.leaves[k], "hi", d.leaves[k].lo) for k in range(d.n_leaves) if d.leaves[k].banded])
    case("lo < hi", band_desc, lambda d: [setattr(d.leaves[k], "lo", float("nan")) for k in range(d.n_leaves) if d.leaves[k].banded])
    case("at least 2 samples per axis", field_desc, lambda d: d.fields[0].res.__setitem__(1, 1))
    case("spacing must be", field_desc, lambda d: setattr(d.fields[0], "spacing", 0.0))
    case("phi array is missing", field_desc, lambda d: setattr(d.fields[0], "phi", C.POINTER(C.c_float)()))
    return cases


def test_refusals_arrive_with_their_messages(tm, shapes, sampled):
    MPMError = tm.mpm.MPMError
    L = tm.load()
    sim = make_sim(tm)
    gi = _group(tm, sim)
    how, keep0 = sim._seed_desc(dict(region=shapes["clipped_shell"][0]), "sand", PPC)
    n = C.c_int64(7)
    x = np.full((4, 3), 0.5, np.float32)
    out = np.zeros(4, np.float32)
    fp = C.POINTER(C.c_float)
    for msg, d, keep in _spoil(tm, shapes, sampled):
        assert L.mpmhip_seed_particles_region(sim._ctx, gi, C.byref(how), C.byref(d), C.byref(n)) == EINVAL, msg
        err = L.mpmhip_last_error(sim._ctx).decode()
        assert msg in err and err.startswith("seed_particles_region: "), (msg, err)
        assert n.value == 0 and L.mpmhip_num_slots(sim._ctx) == 0
        assert L.mpmhip_region_sample(0, 3, DX, C.byref(d), 4, x.ctypes.data_as(fp), out.ctypes.data_as(fp)) == EINVAL, msg
        err = L.mpmhip_last_error(None).decode()
        assert msg in err and err.startswith("region_sample: "), (msg, err)
    # the seed description's own region must be empty; the other arguments are judged as in the plain call
    d, keep = shapes["clipped_shell"][0].compile(3, DX)
    how.n_shapes = 1
    assert L.mpmhip_seed_particles_region(sim._ctx, gi, C.byref(how), C.byref(d), C.byref(n)) == EINVAL
    assert "own region must be empty" in L.mpmhip_last_error(sim._ctx).decode()
    how.n_shapes = 0
    how.ppc = 0.0
    assert L.mpmhip_seed_particles_region(sim._ctx, gi, C.byref(how), C.byref(d), C.byref(n)) == EINVAL
    assert "ppc must be" in L.mpmhip_last_error(sim._ctx).decode()
    how.ppc = PPC
    assert L.mpmhip_seed_particles_region(sim._ctx, 99, C.byref(how), C.byref(d), C.byref(n)) == EINVAL
    assert "unknown group 99" in L.mpmhip_last_error(sim._ctx).decode()
    assert L.mpmhip_region_sample(0, 4, DX, C.byref(d), 4, x.ctypes.data_as(fp), out.ctypes.data_as(fp)) == EINVAL
    assert "dim must be 2 or 3" in L.mpmhip_last_error(None).decode()
    lat = tm._lib.SdfDesc()
    lat.res[:], lat.origin[:], lat.spacing = (8, 8, 8), (0.4, 0.4, 0.4), DX
    big = np.zeros(512, np.float32)
    for band in (0.0, float("inf"), float("nan")):
        assert L.mpmhip_region_bake(0, 3, DX, C.byref(d), C.byref(lat), band, big.ctypes.data_as(fp)) == EINVAL
        assert "band must be a finite number > 0" in L.mpmhip_last_error(None).decode()
    # through Python
    tiny = tm.mpm.Region(tm.mpm.LevelSet().add_sphere((0.5, 0.5, 0.5), 0.4 * DX))
    with pytest.raises(MPMError, match="region is empty"):
        sim.add_particles(dict(type="sand", region=tiny & shapes["clipped_shell"][0], ppc=PPC))
    with pytest.raises(MPMError, match="ppc must be"):
        sim.add_particles(dict(type="sand", region=tiny, ppc=0))
    with pytest.raises(MPMError, match="is 2D, the call is 3D"):
        sim.add_particles(dict(type="sand", region=tiny.placed(rotate=30.0), ppc=PPC))
    assert sim.get_num_particles() == 0
    sim.close()


def test_capacity_and_buffers(tm, sampled, sampled_runs):
    region, (m, want) = sampled["a"], sampled_runs["a"]
    L = tm.load()
    live0 = L.mpmhip_debug_live_buffers()
    sim = make_sim(tm, max_particles=1024)
    gi = _group(tm, sim)
    before = L.mpmhip_host_particle_bytes(sim._ctx)
    how, keep0 = sim._seed_desc(dict(region=region), "sand", PPC)
    d, keep = region.compile(3, DX)
    n = C.c_int64(-1)
    assert L.mpmhip_seed_particles_region(sim._ctx, gi, C.byref(how), C.byref(d), C.byref(n)) == ECAPACITY
    assert n.value == len(want["x"])  # the needed count
    assert sim.get_num_particles() == 0 and L.mpmhip_num_slots(sim._ctx) == 0  # nothing was written
    sim.add_particles(dict(type="sand", region=region, ppc=PPC))  # the wrapper reserves and calls again
    assert L.mpmhip_host_particle_bytes(sim._ctx) == before  # (before anything is downloaded: no record went through the host)
    x, ids = seeded(sim)
    assert L.mpmhip_capacity(sim._ctx) >= len(x) > 1024
    assert L.mpmhip_debug_live_buffers() > live0
    sim.close()
    assert L.mpmhip_debug_live_buffers() == live0
    assert x.tobytes() == want["x"].tobytes() and np.array_equal(ids, np.arange(len(x)))


# ---------------------------------------------------------------------------------------------- 11. the C++ host layer
def test_cpp_host_layer_seeds_the_expression(tm, tile, shapes):
    """MPM<3>::add_particles_region and MPM<2>::add_particles_region with the clipped shell (3D) and the clipped annulus (2D) on
    contexts created for 1024 particles: they grow, the counts are the models', and so is the first particle: the first of the 16
    particles the program prints that is no candidate set aside by the margin protocol against the model's first such survivor"""
    from tests.seed2d_model import SeedModel2D
    from tests.seed2d_model import load_tile as load_tile2
    r = subprocess.run([build_cpp()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    m3 = seed_model(model_of(shapes["clipped_shell"][0]).margin_view(), tile)
    region2 = shape_scenes(tm, 2)["annulus"][0]
    m2 = SeedModel2D(RES, DX, RegionModel.from_desc(region2.compile(2, DX)[0], 2, DX).margin_view(), ppc=4.0, tile=load_tile2(), base_dt=DT)
    for f, m, dim in ((lines[0], m3, 3), (lines[1], m2, 2)):
        want = m.run(margin=MARGIN)
        print("%dD: host layer %s particles, model %d, %d unsure" % (dim, f[0], len(want["x"]), len(want["unsure"])))
        assert abs(int(f[0]) - len(want["x"])) <= len(want["unsure"]) and int(f[1]) == int(f[0]) and int(f[0]) > (1024 if dim == 3 else 300)  # (the 3D ctx had to grow)
        first = np.array(f[2:], np.float32).reshape(16, dim)
        ux = m.positions()[want["unsure"]] if dim == 2 else np.concatenate(
            [m.positions(int(c) // m.n_rep, int(c) // m.n_rep + 1)[int(c) % m.n_rep][None] for c in want["unsure"]] + [np.zeros((0, 3), np.float32)])
        key = lambda a: [r.tobytes() for r in np.ascontiguousarray(a, np.float32)]
        got = [r for r in key(first) if r not in key(ux)]
        ref = [r for r in key(want["x"][~np.isin(want["c"], want["unsure"])][:16])]
        assert len(got) >= 12 and got[0] == ref[0] and got == ref[:len(got)]
