"""mpmhip_seed_particles_brick / add_particles(region=..., brick=True), mpmhip_seed_histogram and the seeded jobs of taichi_mpm_amd.tiled
(include/mpmhip.h: "Seeding a tiled job") on ONE device: K ctxs, each with one brick of a partition, must hold exactly the particles one
ctx seeds — the same ids, the same bits — and a job built and fed that way must run as the one ctx does.  Setup of
tests/test_gpu_seed.py: res 64^3, dx = 1/64, ppc 8; the sampled r = 12 dx sphere at the centre is 2 x 2 x 2 replicas of the tile and
about 46 k particles."""
import ctypes as C

import numpy as np
import pytest

from tests import seed_brick_model as sbm
from tests.common import rel_l2
from tests.region_scenes import shape_scenes
from tests.seed_model import load_tile

pytestmark = pytest.mark.gpu
RES, DX, DT, PPC = 64, 1.0 / 64, 1e-4, 8.0
R12, R4 = 12 * DX, 4 * DX
EINVAL, ECAPACITY = -1, -4
WORLDS = [(2, None), (4, None), (8, None), (3, (1, 3, 1))]
SIM = dict(res=(RES,) * 3, delta_x=DX, base_delta_t=DT)


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


@pytest.fixture(scope="module")
def tiled():
    from taichi_mpm_amd import tiled
    return tiled


def make_sim(tm, **cfg):
    return tm.create_simulation3("mpm").initialize(dict(SIM, **cfg))


def seeded(sim):
    """positions and ids in slot order"""
    p = sim.get_particles(sort_by_id=False)
    return p["x"], p["id"]


def next_id(sim):
    return sim._check(sim._L.mpmhip_set_next_id(sim._ctx, 0))  # (never lowers the counter: 0 reads it)


@pytest.fixture(scope="module")
def sphere(tm):
    """the sampled r = 12 dx sphere at the centre; what one ctx seeds from it (x, id in slot order), its histograms from the device and
    the model's particles: computed once, shared and left unchanged"""
    sls = sbm.sampled_sphere(tm, (0.5, 0.5, 0.5), R12, DX)
    cfg = dict(type="sand", region=sls, ppc=PPC)
    sim = make_sim(tm)
    hist = sim.seed_histograms(cfg)
    sim.add_particles(cfg)
    x, ids = seeded(sim)
    sim.close()
    model = sbm.sampled_model(sls, RES, DX, load_tile(), ppc=PPC, base_dt=DT).run()["x"]
    return dict(cfg=cfg, x=x, id=ids, hist=hist, model=model)


def partition(tiled, hist, world, dims, margin=2):
    hists, lo, hi, _ = hist
    part = tiled.Partition.from_histograms((RES,) * 3, world, hists, lo, hi, margin, dims=dims)
    for a in range(3):  # every cut plane passes through the particles
        assert all(lo[a] < c < hi[a] for c in part.cuts[a][1:-1]), (part.cuts, lo, hi)
    return part


def gather(sims):
    parts = [sim.get_particles(sort_by_id=False) for sim in sims]
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    order = np.argsort(out["id"], kind="stable")
    return {k: v[order] for k, v in out.items()}


def check_ranks_hold_the_one_ctx_particles(tiled, sims, part, x_one, first_id=0, slots_from=None):
    """ids over the ranks = first_id + arange(n), positions by id bit-equal to x_one, slot order ascending in id, exact ownership;
    slots_from[r]: the first slot of rank r to look at (the records of an earlier call lie in front of it)"""
    ids, xs = [], []
    for r, sim in enumerate(sims):
        x, i = seeded(sim)
        x, i = x[(slots_from[r] if slots_from else 0):], i[(slots_from[r] if slots_from else 0):]
        assert (np.diff(i) > 0).all(), "rank %d: slot order is not ascending id" % r
        assert np.array_equal(part.rank_of_cells(tiled.base_cells(x, DX)), np.full(len(x), r)), "rank %d holds a particle of another brick" % r
        ids.append(i)
        xs.append(x)
    ids, xs = np.concatenate(ids), np.concatenate(xs)
    order = np.argsort(ids, kind="stable")
    assert np.array_equal(ids[order], first_id + np.arange(len(x_one)))
    assert xs[order].tobytes() == x_one.tobytes()


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("world,dims", WORLDS)
def test_k_ranks_seed_what_one_ctx_seeds(tm, tiled, sphere, world, dims):
    L = tm.load()
    live0 = L.mpmhip_debug_live_buffers()
    n_one = len(sphere["x"])
    assert 40000 < n_one < 60000 and sphere["x"].tobytes() == sphere["model"].tobytes()
    part = partition(tiled, sphere["hist"], world, dims)
    sims = tiled.build_seeded_rank_sims(tm, [], part, max_particles=1 << 17, **SIM)  # (no group yet: the ctxs with their bricks)
    before = [L.mpmhip_host_particle_bytes(s._ctx) for s in sims]
    for s in sims:
        s.add_particles(dict(sphere["cfg"], brick=True))
    counts = [s.seed_counts for s in sims]
    print("world %d: (here, job) = %s" % (world, counts))
    assert all(c[1] == n_one for c in counts) and sum(c[0] for c in counts) == n_one
    assert all(c[0] > 0.6 * n_one / world for c in counts)
    assert [int(L.mpmhip_num_slots(s._ctx)) for s in sims] == [c[0] for c in counts]
    assert [L.mpmhip_host_particle_bytes(s._ctx) for s in sims] == before  # (before the test itself downloads them)
    check_ranks_hold_the_one_ctx_particles(tiled, sims, part, sphere["x"])
    check_ranks_hold_the_one_ctx_particles(tiled, sims, part, sphere["model"])
    # every rank's next id is the job's: a second, disjoint region takes its ids from n_one on every rank, whether it holds any or not
    assert [next_id(s) for s in sims] == [n_one] * world
    cfg2 = dict(type="sand", ppc=PPC, region=tm.mpm.LevelSet().add_sphere((0.5, 0.5 + 18 * DX, 0.5), R4))
    one = make_sim(tm)
    one.add_particles(sphere["cfg"])
    one.add_particles(cfg2)
    x2 = seeded(one)[0][n_one:]
    one.close()
    for s in sims:
        s.add_particles(dict(cfg2, brick=True))
    assert 1000 < len(x2) and all(s.seed_counts[1] == len(x2) for s in sims)
    check_ranks_hold_the_one_ctx_particles(tiled, sims, part, x2, first_id=n_one, slots_from=[c[0] for c in counts])
    assert [next_id(s) for s in sims] == [n_one + len(x2)] * world
    for s in sims:
        s.close()
    assert L.mpmhip_debug_live_buffers() == live0


# ---------------------------------------------------------------------------------------------------- 2
def test_histogram(tm, tiled, sphere):
    hists, lo, hi, total = sphere["hist"]
    b = tiled.base_cells(sphere["x"], DX)
    for a in range(3):
        assert hists[a].dtype == np.int64 and np.array_equal(hists[a], np.bincount(b[:, a], minlength=RES))
    assert total == len(b) and np.array_equal(lo, b.min(0)) and np.array_equal(hi, b.max(0) + 1)
    # nothing is written and no counter moves, on a ctx that holds particles and on a tiled one
    sim = make_sim(tm)
    sim.add_particles(sphere["cfg"])
    slots, nid = int(sim._L.mpmhip_num_slots(sim._ctx)), next_id(sim)
    again = sim.seed_histograms(sphere["cfg"])
    assert int(sim._L.mpmhip_num_slots(sim._ctx)) == slots == total and next_id(sim) == nid == total and sim.get_num_particles() == total
    sim.close()
    part = partition(tiled, sphere["hist"], 2, None)
    sim, = tiled.build_seeded_rank_sims(tm, [], part, ranks=[1], **SIM)
    tiled_ctx = tiled.seed_histograms(sim, sphere["cfg"])
    assert int(sim._L.mpmhip_num_slots(sim._ctx)) == 0 and next_id(sim) == 0
    with pytest.raises(tm.mpm.MPMError, match="region is empty"):
        sim.seed_histograms(dict(type="sand", ppc=PPC, region=tm.mpm.LevelSet().add_sphere((0.5, 0.5, 0.5), 0.4 * DX)))
    sim.close()
    for got in (again, tiled_ctx):
        assert all(np.array_equal(got[0][a], hists[a]) for a in range(3)) and got[3] == total
        assert np.array_equal(got[1], lo) and np.array_equal(got[2], hi)


# ---------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", ["clipped_shell", "sphere_r12"])
def test_an_expression_and_a_plain_shape(tm, tiled, name):
    """K ranks against one ctx on the same device, every particle: both evaluate the region with the same code"""
    if name == "clipped_shell":  # (sphere - sphere) & plane
        region = shape_scenes(tm, 3)[name][0]
    else:
        region = tm.mpm.LevelSet().add_sphere((0.5, 0.5, 0.5), R12)
    cfg = dict(type="sand", region=region, ppc=PPC)
    one = make_sim(tm)
    hist = tiled.seed_histograms(one, cfg)
    one.add_particles(cfg)
    x, ids = seeded(one)
    one.close()
    assert len(x) > 10000 and np.array_equal(ids, np.arange(len(x))) and hist[3] == len(x)
    part = partition(tiled, hist, 8, None)
    sims = tiled.build_seeded_rank_sims(tm, [cfg], part, **SIM)  # (ctxs of the default capacity or less: the wrapper reserves)
    assert all(s.seed_counts[1] == len(x) for s in sims) and all(s.seed_counts[0] > 0 for s in sims)
    check_ranks_hold_the_one_ctx_particles(tiled, sims, part, x)
    for s in sims:
        s.close()


# ---------------------------------------------------------------------------------------------------- 4
def test_seeded_job_runs_as_the_seeded_one_ctx(tm, tiled, sphere):
    """sand on a plane, 8 ranks on the library's data plane, 11 substeps with migrations every 2: the tolerances of
    test_gpu_tiled.py::test_k_tiles_on_the_native_data_plane_reproduce_one_tile"""
    cfg = dict(sphere["cfg"], initial_velocity=(2.0, -3.0, 1.0))
    ls = lambda: tm.mpm.LevelSet(friction=0.4).add_plane((0, 1, 0), d=-0.31)
    n = len(sphere["x"])
    one = make_sim(tm, max_particles=n + 1024, reorder_interval=0)
    one.set_levelset(ls())
    one.add_particles(cfg)
    part = partition(tiled, sphere["hist"], 8, None)
    sims = tiled.build_seeded_rank_sims(tm, [cfg], part, levelset=ls(), max_particles=n + 1024, reorder_interval=0, **SIM)
    job = tiled.NativeVirtualJob([tiled.HipEngine(s, 0) for s in sims], part, migrate_interval=2)
    steps = 11
    job.run(steps)
    one.run_substeps(steps)
    ref, got = one.get_particles(), gather(sims)
    tot, st = job.totals(), job.state()
    print("totals %s, migrated out %s" % (tot, [t["migrated_out"] for t in st]))
    assert tot["error"] == 0 and tot["particles"] == n
    assert sum(t["migrated_out"] for t in st) > 0, "the scene must exercise migration"
    assert np.array_equal(got["id"], ref["id"]) and np.array_equal(got["id"], np.arange(n)) and np.array_equal(got["gid"], ref["gid"])
    assert np.abs(ref["x"] - sphere["x"]).max() > 1e-4  # it moved
    assert np.abs(got["x"] - ref["x"]).max() <= 1e-6
    assert rel_l2(got["v"], ref["v"]) <= 1e-4 and rel_l2(got["F"], ref["F"]) <= 1e-4 and rel_l2(got["B"], ref["B"]) <= 1e-3
    del job
    for s in sims + [one]:
        s.close()


# ---------------------------------------------------------------------------------------------------- 5
def test_emitter_on_a_resident_job(tm, tiled):
    """an r = 4 dx source sphere on the cut plane y = 32 cells of a two-rank job, its jet along -x and down across the cut: three
    frames of add_particles + 10 substeps (delta_t = 10 base_delta_t) against one ctx doing the same.  The shell a frame fills faces the
    jet's direction, half of it on either side of the cut."""
    part = tiled.Partition((RES,) * 3, (1, 2, 1), [[0, RES], [0, RES // 2, RES], [0, RES]], margin=2)
    cfg = dict(type="water", ppc=PPC, region=sbm.sampled_sphere(tm, (0.5, 0.5, 0.5), R4, DX), pd_source=True, delta_t=1e-3,
               initial_velocity=(-2.0, -1.0, 0.0))
    one = make_sim(tm, reorder_interval=0)
    sims = tiled.build_seeded_rank_sims(tm, [], part, reorder_interval=0, **SIM)
    job = tiled.NativeVirtualJob([tiled.HipEngine(s, 0) for s in sims], part, migrate_interval=2)
    total, replans = 0, 0
    for frame in range(3):
        one.add_particles(cfg)
        added = job.add_particles(cfg)
        total += added[0][1]
        print("frame %d: (here, job) = %s" % (frame, added))
        assert added[0][1] == added[1][1] > 0 and added[0][0] + added[1][0] == added[0][1]
        assert one.get_num_particles() == total == job.num_particles()
        if frame > 0:
            assert added[0][0] > 0 and added[1][0] > 0, "both ranks must take part in the frame"
        job.run(10)  # (raises if the advance fails: it begins with the planning scan, the plan is stale)
        one.run_substeps(10)
        st = job.state()
        assert all(t["replans"] > replans for t in st), st  # the halo boxes were cut again, around the new particles
        replans = max(t["replans"] for t in st)
        tot = job.totals()
        assert tot["error"] == 0 and tot["particles"] == total
    ref, got = one.get_particles(), gather(sims)
    assert np.array_equal(got["id"], ref["id"]) and np.array_equal(got["id"], np.arange(total))
    assert np.abs(got["x"] - ref["x"]).max() <= 1e-6
    assert rel_l2(got["v"], ref["v"]) <= 1e-4 and rel_l2(got["F"], ref["F"]) <= 1e-4 and rel_l2(got["B"], ref["B"]) <= 1e-3
    del job
    for s in sims + [one]:
        s.close()


# ---------------------------------------------------------------------------------------------------- 6
def test_capacity_on_one_rank(tm, tiled, sphere):
    L = tm.load()
    n_one = len(sphere["x"])
    part = partition(tiled, sphere["hist"], 2, None)
    sims = [tiled.build_seeded_rank_sims(tm, [], part, ranks=[r], max_particles=cap, **SIM)[0] for r, cap in ((0, 1 << 17), (1, 1024))]
    params, mat = tm.materials.group_params("sand", 1.0, 1.0)
    results = []
    for s in sims:
        gi = s._check(L.mpmhip_add_group(s._ctx, mat, params.ctypes.data_as(C.POINTER(C.c_float))))
        s._groups.append((mat, params))
        d, keep = s._seed_desc(dict(region=sphere["cfg"]["region"]), "sand", PPC)
        n = (C.c_int64 * 2)(-1, -1)
        results.append((L.mpmhip_seed_particles_brick(s._ctx, gi, C.byref(d), None, n), n[0], n[1], gi, d, keep))
    (rc0, here0, job0, _, _, _), (rc1, here1, job1, gi, d, keep) = results
    assert rc0 == 0 and rc1 == ECAPACITY and job0 == job1 == n_one
    assert here0 + here1 == n_one and here1 > 1024  # the short rank's own need
    assert int(L.mpmhip_num_slots(sims[1]._ctx)) == 0 and sims[1].get_num_particles() == 0 and next_id(sims[1]) == 0  # nothing was written
    assert int(L.mpmhip_num_slots(sims[0]._ctx)) == here0 and next_id(sims[0]) == n_one
    sims[1]._check(L.mpmhip_reserve(sims[1]._ctx, here1 + 16))
    n = (C.c_int64 * 2)(-1, -1)
    assert L.mpmhip_seed_particles_brick(sims[1]._ctx, gi, C.byref(d), None, n) == 0 and (n[0], n[1]) == (here1, n_one)
    assert next_id(sims[1]) == n_one
    check_ranks_hold_the_one_ctx_particles(tiled, sims, part, sphere["x"])
    for s in sims:
        s.close()


# ---------------------------------------------------------------------------------------------------- 7
def test_refusals(tm, tiled, sphere):
    MPMError, L = tm.mpm.MPMError, tm.load()
    cfg = dict(type="sand", ppc=PPC, region=sbm.sampled_sphere(tm, (0.5, 0.5, 0.5), R4, DX))
    sim = make_sim(tm)
    with pytest.raises(MPMError, match="needs a ctx with a partition"):
        sim.add_particles(dict(cfg, brick=True))
    d, keep = sim._seed_desc(dict(region=cfg["region"]), "sand", PPC)
    n = (C.c_int64 * 2)(-1, -1)
    assert L.mpmhip_seed_particles_brick(sim._ctx, 0, C.byref(d), None, n) == EINVAL and (n[0], n[1]) == (0, 0)
    sim.add_particles(cfg)  # (a substep needs particles)
    count = sim.get_num_particles()
    sim._check(L.mpmhip_substep_begin(sim._ctx))
    with pytest.raises(MPMError, match="inside a substep"):
        sim.add_particles(dict(cfg, brick=True))
    with pytest.raises(MPMError, match="inside a substep"):
        sim.seed_histograms(cfg)
    sim._check(L.mpmhip_substep_end(sim._ctx))
    sim.synchronize()
    assert sim.get_num_particles() == count
    # the counter is raised, never lowered
    assert next_id(sim) == count
    assert sim._check(L.mpmhip_set_next_id(sim._ctx, count - 5)) == count and next_id(sim) == count
    assert sim._check(L.mpmhip_set_next_id(sim._ctx, count + 7)) == count + 7 and next_id(sim) == count + 7
    sim.close()
    # the one-ctx calls still refuse a ctx with a partition; the brick call judges its other arguments as they do
    part = partition(tiled, sphere["hist"], 2, None)
    sim, = tiled.build_seeded_rank_sims(tm, [], part, ranks=[0], **SIM)
    with pytest.raises(MPMError, match="tiled ctx"):
        sim.add_particles(cfg)
    with pytest.raises(MPMError, match="tiled ctx"):
        sim.add_particles(dict(cfg, region=tm.mpm.Region(cfg["region"])))
    with pytest.raises(MPMError, match="ppc must be"):
        sim.add_particles(dict(cfg, ppc=0, brick=True))
    with pytest.raises(MPMError, match="unknown group 99"):
        sim._check(L.mpmhip_seed_particles_brick(sim._ctx, 99, C.byref(d), None, n))
    with pytest.raises(MPMError, match="region is empty"):
        sim.add_particles(dict(cfg, brick=True, region=tm.mpm.LevelSet().add_sphere((0.5, 0.5, 0.5), 0.4 * DX)))
    assert sim.get_num_particles() == 0 and next_id(sim) == 0
    sim.close()
