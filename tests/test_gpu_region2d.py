"""Region expressions in the plane (include/mpmhip.h, "Region expressions"; csrc/k_region.h at D = 2) against the numpy model
(tests/region_model.py): the evaluator, the seeding through Simulation2D.add_particles(region=<Region>), and a baked composite
boundary.  The protocol is that of tests/test_gpu_region.py: sampled leaves bit for bit, shape leaves after the candidates within
MARGIN = 1e-4 grid units of a leaf surface or band edge are set aside.
Setup as in tests/test_gpu_seed2d.py: res 64^2, dx = 1/64, ppc 4 (997 tile points: 3 x 1 replicas end in a partial workgroup)."""
import ctypes as C

import numpy as np
import pytest

from tests.region_model import RegionModel
from tests.region_scenes import DX, sampled_scenes, shape_scenes
from tests.seed2d_model import SampledRegion2D, SeedModel2D, load_tile

pytestmark = pytest.mark.gpu
RES, DT, PPC = 64, 1e-4, 4.0
MARGIN = 1e-4
EINVAL = -1


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


@pytest.fixture(scope="module")
def tile(tm):
    return load_tile()


def model_of(region):
    return RegionModel.from_desc(region.compile(2, DX)[0], 2, DX)


def make_sim(tm, **cfg):
    return tm.create_simulation2("mpm").initialize(dict(res=(RES, RES), delta_x=DX, base_delta_t=DT, **cfg))


def _strip(x, unsure_x):
    key = lambda a: np.ascontiguousarray(a, np.float32).view(np.dtype((np.void, 8))).reshape(-1)
    return x[~np.isin(key(x), key(unsure_x))]


def _points():
    return np.random.default_rng(6).uniform(0.1, 0.9, (20000, 2)).astype(np.float32)


@pytest.mark.parametrize("name", ["a", "b"])
def test_evaluator_sampled_leaves_bit_for_bit(tm, name):
    region, x = sampled_scenes(tm, 2)[name], _points()
    got, want = region.sample(x, DX), model_of(region).phi(x)[0]
    inf = np.isinf(want)
    print("2D program (%s): %d of %d points have no lattice, %d inside" % (name, inf.sum(), len(x), (want < 0).sum()))
    assert inf.any() and (~inf).any() and (want < 0).any()
    assert got.tobytes() == want.tobytes()


def test_seeding_sampled_leaves_exact(tm, tile):
    region = sampled_scenes(tm, 2)["b"]
    m = SeedModel2D(RES, DX, model_of(region), ppc=PPC, tile=tile, base_dt=DT)
    want = m.run()
    sim = make_sim(tm)
    sim.add_particles(dict(type="sand", region=region, ppc=PPC))
    p = sim.get_particles(sort_by_id=False)
    sim.close()
    print("2D program (b): %s replicas, %d candidates, %d survivors (model %d)" % (tuple(m.nrep), want["n_cand"], len(p["x"]), len(want["x"])))
    assert len(want["x"]) > 200
    assert p["x"].shape == want["x"].shape and p["x"].tobytes() == want["x"].tobytes()
    assert np.array_equal(p["id"], np.arange(len(p["x"]))) and not p["v"].any()
    assert np.array_equal(p["F"], np.tile(np.eye(2, dtype=np.float32).reshape(1, 4), (len(p["x"]), 1)))


@pytest.mark.parametrize("name,nrep", [("annulus", (2, 1)), ("placed_boxes", (3, 1))])
def test_seeding_shape_leaves(tm, tile, name, nrep):
    region = shape_scenes(tm, 2)[name][0]
    m = SeedModel2D(RES, DX, model_of(region).margin_view(), ppc=PPC, tile=tile, base_dt=DT)
    want = m.run(margin=MARGIN)
    assert tuple(m.nrep) == nrep and want["n_cand"] == nrep[0] * nrep[1] * len(tile)
    if name == "placed_boxes":
        assert want["n_cand"] % 1024 != 0  # the last workgroup is partial: its ballot words hold lanes without a candidate
    sim = make_sim(tm)
    sim.add_particles(dict(type="sand", region=region, ppc=PPC))
    p = sim.get_particles(sort_by_id=False)
    sim.close()
    x, unsure = p["x"], want["unsure"]
    print("2D %s: %d candidates, %d unsure, device %d, model %d" % (name, want["n_cand"], len(unsure), len(x), len(want["x"])))
    assert len(unsure) <= 0.005 * want["n_cand"] and len(x) > 300
    assert np.array_equal(p["id"], np.arange(len(x)))
    got, ref = _strip(x, m.positions()[unsure]), want["x"][~np.isin(want["c"], unsure)]
    assert abs(len(x) - len(want["x"])) <= len(unsure)
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes()


def _solid(tm):
    """a floor with a mound on it and a slot cut down through both to y = 0.15 (closed below: no sand leaves through it towards the
    7 cells at the wall, where the domain rule deletes particles)"""
    LS, Region = tm.mpm.LevelSet, tm.mpm.Region
    floor = Region(LS().add_plane((0, 1, 0), d=-0.25))
    mound = Region(LS().add_sphere((0.5, 0.25, 0.0), 6 * DX))
    drain = Region(LS().add_cuboid((0.47, 0.15, 0.0), (0.53, 0.5, 0.0)))
    return (floor | mound) - drain


def test_baked_composite_boundary(tm):
    """to_sampled2d(...).as_boundary(friction) is an ordinary sampled boundary.  The installed set returns the baked array's
    bilinear value at 1 000 points, bit for bit.  Then, as tests/test_gpu_sdf2d.py holds its polygon hopper: sand with
    particle_collision, seeded where the baked phi is above half a cell (the baked array itself is a banded leaf of the seeding
    expression) and thrown at the solid at 3 m/s, is checked after every 20th of 200 substeps (the sand travels 3.8 cells): no particle is lost, none is NaN, and
    every particle's device-sampled phi is >= -(the model's one-step projection residual of the baked array)"""
    from tests.sdf2d_model import Sdf2DModel
    solid = _solid(tm)
    res, origin, spacing = (128, 128), (0.003, 0.002), DX / 2
    baked = solid.to_sampled2d(res, origin, spacing, delta_x=DX)
    band = np.float32(3.0 * DX + 2.0 * spacing)
    want = model_of(solid).bake(res, np.asarray(origin, np.float32), np.float32(spacing), band)
    # (shape leaves: the device may contract inside levelset_eval_key, so the baked values are held to the margin, not to the bit)
    assert baked.phi.shape == res and np.abs(baked.phi - want).max() <= MARGIN * DX and np.abs(baked.phi).max() <= band
    sim = make_sim(tm, particle_collision=True, deterministic=True)  # (no float atomics: the run, and the count below, repeat exactly)
    sim.set_levelset(baked.as_boundary(friction=0.4))
    x = np.random.default_rng(8).uniform(0.05, 0.95, (1000, 2)).astype(np.float32)
    phi, grad, dphidt, hit = sim.sample_levelset(x)
    model = Sdf2DModel(baked.phi, baked.origin, baked.spacing, DX)
    ref = SampledRegion2D(baked.phi, baked.origin, baked.spacing, DX).phi(x)[0]
    assert hit.all() and phi.tobytes() == ref.tobytes() and (phi < 0).any() and (phi > 0).any()
    residual = model.projection_residual(np.random.default_rng(2).uniform(0.1, 0.9, (1000000, 2)).astype(np.float32), DX)
    Region, LS = tm.mpm.Region, tm.mpm.LevelSet
    # (9 cells clear of the walls' 7-cell margin on either side, as the hopper's block is: the collapsing block spreads sideways, and
    # what gets within 7 cells of a wall is deleted by the domain rule)
    block = Region(LS().add_cuboid((0.25, 0.27, 0.0), (0.75, 0.62, 0.0))) & Region(baked).band(0.5, 100.0)  # 0.5 < baked phi (it is clamped at 4)
    sim.add_particles(dict(type="sand", region=block, ppc=PPC, initial_velocity=(0.0, -3.0)))
    n = sim.get_num_particles()
    start = sim.sample_levelset(sim.get_particles(sort_by_id=False)["x"])[0]
    assert n > 2000 and 0.5 < start.min() < 0.7  # the seeding and the boundary read one array with one sampler
    lowest, touched = float(start.min()), 0
    for k in range(10):
        sim.run_substeps(20)
        p = sim.get_particles()
        assert len(p["x"]) == n, (k, len(p["x"]), n, p["x"].min(axis=0), p["x"].max(axis=0))
        for f in ("x", "v", "F", "B", "aux"):
            assert np.isfinite(p[f]).all(), f
        phi, _, _, hit = sim.sample_levelset(p["x"])
        assert hit.all()
        lowest = min(lowest, float(phi.min()))
        touched = max(touched, int((phi < 0.25).sum()))
        assert phi.min() >= -residual, (k, float(phi.min()), residual)
    sim.close()
    print("baked boundary: %d particles, lowest phi %.4g cells, one-step projection residual %.4g cells, %d particles within 0.25 cells of the solid" % (
        n, lowest, residual, touched))
    assert touched > 20  # the sand did reach the solid


def test_refusals_in_the_plane(tm):
    L = tm.load()
    sim = make_sim(tm)
    sim._ensure_ctx()
    params, mat = tm.materials.group_params("sand", 1.0, 1.0)
    gi = sim._check(L.mpmhip2d_add_group(sim._ctx, mat, params.ctypes.data_as(C.POINTER(C.c_float))))
    sim._groups.append((mat, params))
    region = shape_scenes(tm, 2)["placed_boxes"][0]
    how, keep0 = sim._seed_desc(dict(region=region), "sand", PPC)
    n = C.c_int64(3)
    for msg, change in (("rotation is not finite", lambda d: d.leaves[0].rot.__setitem__(0, float("inf"))),
                        ("scale must be", lambda d: setattr(d.leaves[1], "scale", -1.0)),
                        ("stack underflow", lambda d: setattr(d.ops[0], "op", tm._lib.REGION_NEG)),
                        ("the program is empty", lambda d: setattr(d, "n_ops", 0))):
        d, keep = region.compile(2, DX)
        change(d)
        assert L.mpmhip2d_seed_particles_region(sim._ctx, gi, C.byref(how), C.byref(d), C.byref(n)) == EINVAL, msg
        err = L.mpmhip2d_last_error(sim._ctx).decode()
        assert msg in err and n.value == 0, (msg, err)
    d, keep = region.compile(2, DX)
    how.n_shapes = 2
    assert L.mpmhip2d_seed_particles_region(sim._ctx, gi, C.byref(how), C.byref(d), C.byref(n)) == EINVAL
    assert "own region must be empty" in L.mpmhip2d_last_error(sim._ctx).decode()
    with pytest.raises(tm.mpm.MPMError, match="cannot be composed"):
        sim.add_particles(dict(type="sand", region=region.placed(rotate=((0, 0, 1), 10.0)), ppc=PPC))
    assert sim.get_num_particles() == 0
    sim.close()
