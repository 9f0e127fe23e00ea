"""GPU tests of the tiled (multi-GPU) path on ONE device: K "virtual ranks" = K libmpmhip ctx, each holding one
brick's particles, exchanges done as local copies (taichi_mpm_amd.tiled.VirtualTiledJob).  The kernels, halo boxes,
rank-ordered sums and the migration are exactly what a real multi-GPU run executes; only the transport differs
(RCCL all_to_all there).  The K-tile run must reproduce the 1-ctx run (SURVEY §8e "Test constraint").
"""
import numpy as np
import pytest

from tests.common import lattice_cube, make_state, rel_l2

pytestmark = pytest.mark.gpu

RES, DX, DT = 32, 1.0 / 32, 1e-4
PLANES = [(0.0, 1.0, 0.0, -0.3)]


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


def _sim(tm, s, sel, ids, cap):
    from taichi_mpm_amd.mpm import F_ID
    sim = tm.create_simulation3("mpm")
    sim.initialize(dict(res=(RES,) * 3, delta_x=DX, base_delta_t=DT, max_particles=cap, reorder_interval=0))
    ls = tm.mpm.LevelSet(friction=0.4)
    for p in PLANES:
        ls.add_plane(p[:3], d=p[3])
    sim.set_levelset(ls)
    names = {v: k for k, v in tm.MATERIAL_IDS.items()}
    # every rank registers every group in the same order (group ids travel with migrating particles)
    for gi in range(len(s.gtype)):
        m = sel & (s.gid == gi)
        sim.add_particles(dict(type=names[int(s.gtype[gi])], positions=s.x[m], velocities=s.v[m], F=s.F[m], B=s.B[m],
                               aux=s.aux[m], params=s.gparams[gi]))
    order = np.concatenate([np.nonzero(sel & (s.gid == gi))[0] for gi in range(len(s.gtype))])
    if len(order):
        sim.upload(F_ID, ids[order].astype(np.int32))
    else:
        sim._ensure_ctx()
    return sim


def _two_material_state():
    x = lattice_cube(RES, 9, 21, DX, jitter=0.2, seed=21)
    a = make_state(x, "jelly", DX, perturb_F=0.02, seed=22, vel_scale=8.0)
    b = make_state(x, "sand", DX, perturb_F=0.02, seed=23, vel_scale=8.0)
    half = x[:, 0] < x[:, 0].mean()
    s = a.copy()
    s.gparams = np.concatenate([a.gparams, b.gparams])
    s.gtype = np.concatenate([a.gtype, b.gtype])
    s.gid = np.where(half, 0, 1).astype(np.int32)
    s.F[~half] = b.F[~half]
    s.aux[~half] = b.aux[~half]
    return s


def _gather(sims):
    parts = [sim.get_particles(sort_by_id=False) for sim in sims]
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    order = np.argsort(out["id"], kind="stable")
    return {k: v[order] for k, v in out.items()}


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap_split"])
@pytest.mark.parametrize("world,dims", [(2, None), (4, None), (8, None), (3, (1, 3, 1))])
def test_k_tiles_reproduce_one_tile(tm, world, dims, overlap):
    from taichi_mpm_amd import tiled
    s = _two_material_state()
    n = s.n
    ids = np.arange(n)
    one = _sim(tm, s, np.ones(n, bool), ids, n + 1024)
    part = tiled.Partition.balanced((RES,) * 3, world, s.x, DX, margin=2, dims=dims)
    owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
    counts = np.bincount(owner, minlength=world)
    assert counts.min() > 0.6 * n / world, counts  # balanced cuts
    sims = [_sim(tm, s, owner == r, ids, n + 1024) for r in range(world)]
    job = tiled.VirtualTiledJob([tiled.HipEngine(sim, 0) for sim in sims], part, migrate_interval=2, overlap=overlap)

    # one P2G: every rank's node totals equal the single-ctx totals wherever the rank has mass of its own
    one.sort_particles_and_populate_grid()
    one.rasterize_optimized()
    g1 = one.get_grid(0)
    for r in job.ranks:
        r.e.begin()
    job._a2a([r.plan.recv for r in job.ranks], [r.plan.send for r in job.ranks], [r.plan.splits for r in job.ranks])
    for r in job.ranks:
        r.e.interior()  # (no-op unless the substep is split: then the interior blocks are rasterized here)
    for rank, sim in enumerate(sims):
        gr = sim.get_grid(0)
        (nlo, nhi) = part.node_box(rank)
        touched = gr[..., 3] > 0
        assert touched.any()
        idx = np.argwhere(touched)
        assert (idx >= np.array(nlo)).all() and (idx < np.array(nhi)).all()
        assert rel_l2(gr[touched][:, 3], g1[touched][:, 3]) <= 1e-6
        assert rel_l2(gr[touched][:, :3], g1[touched][:, :3]) <= 1e-5
    # ranks sharing a node hold the bit-identical total (rank-ordered sums)
    for a in range(world):
        for b in range(a + 1, world):
            ga, gb = sims[a].get_grid(0), sims[b].get_grid(0)
            both = (ga[..., 3] > 0) & (gb[..., 3] > 0)
            assert np.array_equal(ga[both], gb[both])
    for r in job.ranks:
        r.e.end()
        r.k += 1
    one.normalize_grid_and_apply_boundary_conditions()
    one.resample_optimized()

    steps = 11
    job.run(steps)  # migrations at k = 2, 4, ...
    one.run_substeps(steps)
    ref = one.get_particles()
    got = _gather(sims)
    assert sum(r.migrated_out for r in job.ranks) > 0, "the scene must exercise migration"
    assert len(got["id"]) == len(ref["id"]) == n
    assert np.array_equal(got["id"], ref["id"])
    assert np.array_equal(got["gid"], ref["gid"])
    # every particle sits on the rank that owns its base cell, or within the margin of it
    for rank, sim in enumerate(sims):
        p = sim.get_particles(sort_by_id=False)
        b = tiled.base_cells(p["x"], DX)
        lo, hi = part.brick(rank)
        assert (b >= np.array(lo) - part.margin).all() and (b < np.array(hi) + part.margin).all()
    assert np.abs(got["x"] - ref["x"]).max() <= 1e-6
    assert rel_l2(got["v"], ref["v"]) <= 1e-4
    assert rel_l2(got["F"], ref["F"]) <= 1e-4
    assert rel_l2(got["B"], ref["B"]) <= 1e-3
    for sim in sims + [one]:
        sim.close()


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap_split"])
def test_profiling_level_4_brackets_the_parts_of_a_tiled_substep(tm, overlap):
    """mpmhip_set_profiling(4): begin / interior / end of a tiled substep bracketed as wholes (include/mpmhip.h) — "p2g" holds
    the begin part, "grid" the interior part (only when the substep is split), "g2p" the end part; nothing is recorded inside
    a part, and the run is the one an unprofiled job does."""
    from taichi_mpm_amd import tiled
    s = _two_material_state()
    n, ids = s.n, np.arange(s.n)
    part = tiled.Partition.balanced((RES,) * 3, 2, s.x, DX, margin=2)
    owner = part.rank_of_cells(tiled.base_cells(s.x, DX))

    def run(level):
        sims = [_sim(tm, s, owner == r, ids, n + 1024) for r in range(2)]
        job = tiled.VirtualTiledJob([tiled.HipEngine(sim, 0) for sim in sims], part, migrate_interval=2, overlap=overlap)
        for sim in sims:
            sim.set_profiling(level)
            sim.profile(reset=True)
        job.run(6)
        profs = [sim.profile() for sim in sims]
        got = _gather(sims)
        for sim in sims:
            sim.close()
        return profs, got
    profs, got = run(4)
    _, plain = run(0)
    for p in profs:
        ph = p["phases"]
        assert p["substeps"] == 6 and ph["sort"] == 0.0
        assert ph["p2g"] > 0.0 and ph["g2p"] > 0.0 and (ph["grid"] > 0.0) == overlap
    assert np.array_equal(got["id"], plain["id"]) and np.abs(got["x"] - plain["x"]).max() <= 1e-6
    with pytest.raises(Exception):
        s0 = _sim(tm, s, owner == 0, ids, n + 1024)
        try:
            s0.set_profiling(5)
        finally:
            s0.close()


def test_c5_clusters_over_8_virtual_ranks_reproduce_one_ctx(tm):
    """BASELINE configs[4] on more than one GPU (reduced: 64^3 grid, 8 clusters of 12^3 cells x 8, water / Hencky-elastic
    alternating): the builders bench.py uses for `--config c5 --gpus 8` — every rank registers all 8 groups, balanced
    bricks over the union of the clusters — against the single-ctx builder, 11 substeps, K = 8 bricks"""
    import bench
    from taichi_mpm_amd import tiled
    cfg = dict(res=64, cells=12, material="water+elastic", clusters=(10, 38), desc="reduced c5")
    one = bench.build_sim(tm, cfg, 0)
    groups = tiled.scene_groups(cfg)
    assert len(groups) == 8 and {g[0] for g in groups} == {"water", "elastic"}
    part = tiled.scene_partition(cfg, 8, margin=2)
    assert part.dims == (2, 2, 2)
    engines, total = [], 0
    for r in range(8):
        sim, total = tiled.build_rank_sim(tm, cfg, part, r, 0, extra_cfg=dict(reorder_interval=0))
        assert sim.get_num_particles() > 0.5 * total / 8  # the cuts fall between the clusters
        engines.append(tiled.HipEngine(sim, 0))
    assert total == 8 * 12 ** 3 * 8 == one.get_num_particles()
    job = tiled.VirtualTiledJob(engines, part, migrate_interval=2, overlap=True)
    steps = 11
    job.run(steps)
    one.run_substeps(steps)
    ref, got = one.get_particles(), _gather([e.sim for e in engines])
    assert np.array_equal(got["id"], ref["id"]) and np.array_equal(got["gid"], ref["gid"])
    assert set(np.unique(got["gid"])) == set(range(8))
    assert np.abs(got["x"] - ref["x"]).max() <= 1e-6
    assert rel_l2(got["v"], ref["v"]) <= 1e-4
    el = ref["gid"] % 2 == 1  # water never updates F
    assert rel_l2(got["F"][el], ref["F"][el]) <= 1e-4 and np.abs(got["aux"] - ref["aux"]).max() <= 1e-4
    for e in engines:
        e.sim.close()
    one.close()


def test_adaptive_migration_schedule_on_the_device(tm):
    """no explicit interval: the scan's measured top speed (max |v|_inf dt / dx over the live particles) schedules
    the next migration; checked against numpy on the downloaded velocities, and the 4-brick run still reproduces the
    single-ctx run with far fewer scans than the CFL schedule would make"""
    from taichi_mpm_amd import tiled
    s = _two_material_state()
    n, world, steps = s.n, 4, 60
    ids = np.arange(n)
    one = _sim(tm, s, np.ones(n, bool), ids, n + 1024)
    part = tiled.Partition.balanced((RES,) * 3, world, s.x, DX, margin=2)
    owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
    sims = [_sim(tm, s, owner == r, ids, n + 1024) for r in range(world)]
    engines = [tiled.HipEngine(sim, 0) for sim in sims]
    job = tiled.VirtualTiledJob(engines, part, overlap=True)
    _, _, _, sp = engines[0].migration_scan()
    v0 = sims[0].get_particles(sort_by_id=False)["v"]
    assert abs(sp - np.abs(v0).max() * DT / DX) <= 1e-6 * sp and 0 < sp < 0.5
    scans = []
    plain = engines[0].migration_scan

    def counting_scan():
        scans.append(job.ranks[0].k)
        return plain()
    engines[0].migration_scan = counting_scan
    job.run(steps)
    one.run_substeps(steps)
    assert scans[0] == 2 and 2 <= len(scans) <= steps // 6, scans
    assert sum(r.migrated_out for r in job.ranks) > 0
    for rank, sim in enumerate(sims):  # nobody is beyond the margin of its brick (the library would have raised)
        b = tiled.base_cells(sim.get_particles(sort_by_id=False)["x"], DX)
        lo, hi = part.brick(rank)
        assert (b >= np.array(lo) - part.margin).all() and (b < np.array(hi) + part.margin).all()
    ref, got = one.get_particles(), _gather(sims)
    assert np.array_equal(got["id"], ref["id"]) and np.abs(got["x"] - ref["x"]).max() <= 2e-6
    assert rel_l2(got["v"], ref["v"]) <= 2e-4 and rel_l2(got["F"], ref["F"]) <= 2e-4
    for sim in sims + [one]:
        sim.close()


def test_migration_compacts_when_slots_run_out(tm):
    """leavers leave dead slots behind; a rank that keeps receiving and losing particles compacts its records at
    a later sort instead of running out of slots"""
    from taichi_mpm_amd import tiled
    x = lattice_cube(RES, 8, 20, DX, jitter=0.2, seed=31)
    s = make_state(x, "jelly", DX, perturb_F=0.0, seed=32, vel_scale=0.0)
    s.v[:] = (25.0, 0.0, 0.0)  # 0.08 cells per substep along x: a steady stream across both cuts
    s.B[:] = 0
    n = s.n
    part = tiled.Partition.balanced((RES,) * 3, 3, s.x, DX, margin=2, dims=(3, 1, 1))
    owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
    own = [int((owner == r).sum()) for r in range(3)]
    caps = [own[0] + 64, int(own[1] * 1.3), n]
    sims = [_sim(tm, s, owner == r, np.arange(n), caps[r]) for r in range(3)]
    for sim in sims:
        sim.set_levelset(tm.mpm.LevelSet())
    job = tiled.VirtualTiledJob([tiled.HipEngine(sim, 0) for sim in sims], part, migrate_interval=2)
    b = tiled.base_cells(s.x, DX)
    part.clip = (list(map(int, b.min(0) - 3)), list(map(int, b.max(0) + 6)))  # tight: the moving blob forces replans
    for r in job.ranks:
        r.replan()
    job.run(50)
    got = _gather(sims)
    assert all(r.replans >= 2 for r in job.ranks)  # the halo boxes followed the particles
    assert len(got["id"]) == n and np.array_equal(got["id"], np.arange(n))
    through = job.ranks[1].migrated_out
    assert through > 0.5 * own[1], (through, own)  # far more slots were used than the 30 % of slack
    assert int(sims[1]._L.mpmhip_num_slots(sims[1]._ctx)) <= caps[1]
    assert np.allclose(got["v"][:, 0], 25.0, rtol=1e-3)
    for sim in sims:
        sim.close()


# ------------------------------------------------------------------------------------------ the native data plane
def test_native_plan_equals_the_python_plan(tm):
    """mpmhip_tiled_setup derives the halo boxes from the partition itself (csrc/tiled_api.h: tn_plan); they equal the
    boxes taichi_mpm_amd.tiled.Partition computes for the callback path, and every box knows its offset in the PEER's buffers"""
    from taichi_mpm_amd import tiled
    s = _two_material_state()
    for world, dims in ((8, None), (3, (1, 3, 1)), (4, None)):
        part = tiled.Partition.balanced((RES,) * 3, world, s.x, DX, margin=2, dims=dims)
        owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
        sims = [_sim(tm, s, owner == r, np.arange(s.n), s.n + 1024) for r in range(world)]
        engines = [tiled.HipEngine(sim, 0) for sim in sims]
        job = tiled.NativeVirtualJob(engines, part, migrate_interval=2)
        offsets = {}
        for r in range(world):
            off = 0
            for peer, lo, hi in part.boxes(r):
                offsets[(r, peer)] = off
                off += int(np.prod([hi[a] - lo[a] for a in range(3)]))
        for r, e in enumerate(engines):
            got = tiled.native_plan(e)
            want = part.boxes(r)
            assert [(g[0], g[1], g[2]) for g in got] == [(p, list(lo), list(hi)) for p, lo, hi in want]
            assert [g[3] for g in got] == [offsets[(p, r)] for p, _, _ in want]
            st = tiled.native_state(e)
            assert st["halo_boxes"] == len(want) and st["wire"] == 3 and st["halo_nodes"] == sum(
                int(np.prod([hi[a] - lo[a] for a in range(3)])) for _, lo, hi in want)
        del job
        for sim in sims:
            sim.close()


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap_split"])
@pytest.mark.parametrize("world,dims", [(2, None), (4, None), (8, None), (3, (1, 3, 1))])
def test_k_tiles_on_the_native_data_plane_reproduce_one_tile(tm, world, dims, overlap):
    """the same comparison as test_k_tiles_reproduce_one_tile with NOTHING of the run in Python: plan, buffers, the
    per-substep loop, the halo exchange (peer writes + epoch flags, MPMHIP_WIRE_LOCAL), the migration (scan, table,
    records, import) and its schedule all run inside mpmhip_tiled_advance_group"""
    from taichi_mpm_amd import tiled
    s = _two_material_state()
    n, ids = s.n, np.arange(s.n)
    one = _sim(tm, s, np.ones(n, bool), ids, n + 1024)
    part = tiled.Partition.balanced((RES,) * 3, world, s.x, DX, margin=2, dims=dims)
    owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
    sims = [_sim(tm, s, owner == r, ids, n + 1024) for r in range(world)]
    engines = [tiled.HipEngine(sim, 0) for sim in sims]
    job = tiled.NativeVirtualJob(engines, part, migrate_interval=2, overlap=overlap)
    steps = 12
    job.run(5)
    job.run(steps - 5)  # (a second call continues the schedule)
    one.run_substeps(steps)
    ref, got = one.get_particles(), _gather(sims)
    st = job.state()
    assert all(t["substeps"] == steps and t["migrations"] == steps // 2 for t in st), st
    assert sum(t["migrated_out"] for t in st) > 0, "the scene must exercise migration"
    assert np.array_equal(got["id"], ref["id"]) and np.array_equal(got["gid"], ref["gid"])
    for rank, sim in enumerate(sims):
        b = tiled.base_cells(sim.get_particles(sort_by_id=False)["x"], DX)
        lo, hi = part.brick(rank)
        assert (b >= np.array(lo) - part.margin).all() and (b < np.array(hi) + part.margin).all()
    assert np.abs(got["x"] - ref["x"]).max() <= 1e-6
    assert rel_l2(got["v"], ref["v"]) <= 1e-4 and rel_l2(got["F"], ref["F"]) <= 1e-4 and rel_l2(got["B"], ref["B"]) <= 1e-3
    # the callback path refuses a ctx whose plan is the library's, and the other way round
    with pytest.raises(tm.mpm.MPMError, match="native plan"):
        engines[0].run_native(1, lambda: None, lambda: None)
    with pytest.raises(tm.mpm.MPMError, match="advance together"):
        sims[0]._check(sims[0]._L.mpmhip_tiled_advance(sims[0]._ctx, 1))
    for sim in sims + [one]:
        sim.close()


def test_halo_boxes_are_cut_to_each_ranks_own_occupancy(tm):
    """two blobs in two bricks, far apart, flying at each other: the planning scan in front of the first substep cuts every rank's node box
    to the nodes ITS particles can reach (the migration table carries every rank's bounds), so nothing is exchanged while the blobs
    are apart (until round 6: the slab around the cut across the job's whole bounding box, every substep); the boxes come back by
    re-plans before the blobs meet, and the collision agrees with the one-ctx run"""
    from taichi_mpm_amd import tiled
    from taichi_mpm_amd.mpm import F_ID
    res, dx = 64, 1.0 / 64
    xa = lattice_cube(res, 29, 35, dx, jitter=0.2, seed=41)
    xb = xa.copy()
    xa[:, 0] -= 17 * dx  # cells 12..18 in x
    xb[:, 0] += 17 * dx  # cells 46..52: 28 cells apart, more than the two occupancy slacks (12 cells each at margin 2)
    s = make_state(np.concatenate([xa, xb]), "jelly", dx, perturb_F=0.0, seed=42, vel_scale=0.0)
    s.v[:len(xa)] = (40.0, 0.0, 0.0)
    s.v[len(xa):] = (-40.0, 0.0, 0.0)
    s.B[:] = 0
    n, ids = s.n, np.arange(s.n)
    part = tiled.Partition.balanced((res,) * 3, 2, s.x, dx, margin=2, dims=(2, 1, 1))
    owner = part.rank_of_cells(tiled.base_cells(s.x, dx))
    assert np.array_equal(owner, (np.arange(n) >= len(xa)).astype(owner.dtype))  # one blob per brick

    def make(sel):
        sim = tm.create_simulation3("mpm")
        sim.initialize(dict(res=(res,) * 3, delta_x=dx, base_delta_t=DT, max_particles=n + 1024, reorder_interval=0, gravity=(0, 0, 0)))
        sim.set_levelset(tm.mpm.LevelSet())
        sim.add_particles(dict(type="jelly", positions=s.x[sel], velocities=s.v[sel], F=s.F[sel], B=s.B[sel], aux=s.aux[sel], params=s.gparams[0]))
        sim.upload(F_ID, ids[sel].astype(np.int32))
        return sim

    one = make(np.ones(n, bool))
    assert one.get_num_particles() == n
    sims = [make(owner == r) for r in range(2)]
    job = tiled.NativeVirtualJob([tiled.HipEngine(sim, 0) for sim in sims], part)
    assert all(t["halo_nodes"] > 0 for t in job.state())  # the set-up's plan: the job's bounding box
    job.run(1)
    st = job.state()
    assert all(t["halo_nodes"] == 0 and t["halo_boxes"] == 0 and t["replans"] == 1 and t["migrations"] == 0 for t in st), st
    seen, steps = [], 1
    while steps < 90:
        job.run(6)
        steps += 6
        seen.append(job.state()[0]["halo_nodes"])
    one.run_substeps(steps)
    assert seen[0] == 0 and max(seen) > 0, seen  # apart: nothing; the boxes are back before the blobs touch (and go again when they have bounced apart)
    st = job.state()
    assert all(t["replans"] >= 2 for t in st) and len({t["next_migration"] for t in st}) == 1, st
    ref, got = one.get_particles(), _gather(sims)
    assert np.array_equal(got["id"], ref["id"]) and len(ref["id"]) == n
    va = got["v"][:len(xa), 0]
    assert va.mean() < 20.0, float(va.mean())  # they DID collide (free flight would keep 40)
    assert np.abs(got["x"] - ref["x"]).max() <= 1e-6
    # (the blobs are nearly at rest by now: the velocities are compared on the scale they had, 40)
    assert np.abs(got["v"] - ref["v"]).max() <= 40.0 * 1e-5 and rel_l2(got["F"], ref["F"]) <= 1e-4
    for sim in sims + [one]:
        sim.close()


def test_native_migration_follows_a_moving_blob(tm):
    """the moving blob of test_migration_compacts_when_slots_run_out on the native data plane: adaptive schedule from the
    measured top speed, re-plans when the particles leave the clip box, compaction when slots run out — all inside the library"""
    from taichi_mpm_amd import tiled
    x = lattice_cube(RES, 8, 20, DX, jitter=0.2, seed=31)
    s = make_state(x, "jelly", DX, perturb_F=0.0, seed=32, vel_scale=0.0)
    s.v[:] = (25.0, 0.0, 0.0)
    s.B[:] = 0
    n = s.n
    part = tiled.Partition.balanced((RES,) * 3, 3, s.x, DX, margin=2, dims=(3, 1, 1))
    b = tiled.base_cells(s.x, DX)
    part.clip = (list(map(int, b.min(0) - 3)), list(map(int, b.max(0) + 6)))  # tight: the moving blob forces re-plans
    owner = part.rank_of_cells(b)
    own = [int((owner == r).sum()) for r in range(3)]
    caps = [own[0] + 64, int(own[1] * 1.3), n]
    sims = [_sim(tm, s, owner == r, np.arange(n), caps[r]) for r in range(3)]
    for sim in sims:
        sim.set_levelset(tm.mpm.LevelSet())
    job = tiled.NativeVirtualJob([tiled.HipEngine(sim, 0) for sim in sims], part, inbox_records=n)
    job.run(50)
    st = job.state()
    got = _gather(sims)
    assert all(t["replans"] >= 1 for t in st), st  # the halo boxes followed the particles
    assert 2 <= st[0]["migrations"] < 25 and len({t["next_migration"] for t in st}) == 1  # adaptive, the same on every rank
    assert len(got["id"]) == n and np.array_equal(got["id"], np.arange(n))
    assert st[1]["migrated_out"] > 0.5 * own[1]
    assert int(sims[1]._L.mpmhip_num_slots(sims[1]._ctx)) <= caps[1]
    assert np.allclose(got["v"][:, 0], 25.0, rtol=1e-3)
    for sim in sims:
        sim.close()


@pytest.mark.parametrize("world", [2, 8])
def test_energy_and_totals_of_k_virtual_ranks_equal_the_one_ctx_numbers(tm, world):
    """MPM<dim>::calculate_energy (src/mpm.cpp:1078-1110) of a tiled job: halo exchange after the rasterization, every node's kinetic
    energy counted by the lowest rank that holds mass on it, the ranks' shares summed over the wire (mpmhip_tiled_reduce) — equal to
    the one-ctx energy to 1e-6 relative; and the job's totals (live particles, error word)"""
    from taichi_mpm_amd import tiled
    x = lattice_cube(RES, 9, 21, DX, jitter=0.2, seed=31)
    a = make_state(x, "jelly", DX, perturb_F=0.03, seed=32, vel_scale=8.0)
    b = make_state(x, "elastic", DX, perturb_F=0.03, seed=33, vel_scale=8.0)
    half = x[:, 1] < x[:, 1].mean()
    s = a.copy()
    s.gparams = np.concatenate([a.gparams, b.gparams]); s.gtype = np.concatenate([a.gtype, b.gtype])
    s.gid = np.where(half, 0, 1).astype(np.int32)
    s.F[~half] = b.F[~half]
    one = _sim(tm, s, np.ones(s.n, bool), np.arange(s.n), s.n + 1024)
    part = tiled.Partition.balanced((RES,) * 3, world, s.x, DX, margin=2)
    owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
    sims = [_sim(tm, s, owner == r, np.arange(s.n), s.n + 1024) for r in range(world)]
    job = tiled.NativeVirtualJob([tiled.HipEngine(sim, 0) for sim in sims], part, migrate_interval=2)
    for steps in (0, 5):
        one.run_substeps(steps)
        job.run(steps)
        k1, p1 = one.calculate_energy()
        k2, p2 = job.calculate_energy()
        assert k1 > 0 and p1 > 0
        assert np.isclose(k2, k1, rtol=1e-6) and np.isclose(p2, p1, rtol=1e-6), (steps, k1, k2, p1, p2)
    tot = job.totals()
    assert tot["particles"] == one.get_num_particles() and tot["error"] == 0 and tot["active_blocks"] >= one.profile()["active_blocks"]
    rows = job.reduce([[r + 1.0, -r] for r in range(world)], "sum")
    assert all(row == [world * (world + 1) / 2.0, -world * (world - 1) / 2.0] for row in rows)
    assert job.reduce([[float(r)] for r in range(world)], "max")[0] == [world - 1.0]
    one.run_substeps(3)
    job.run(3)  # (the energy's exchange consumed epochs on every rank alike: the run goes on)
    got, ref = _gather(sims), one.get_particles()
    assert np.array_equal(got["id"], ref["id"]) and np.abs(got["x"] - ref["x"]).max() <= 1e-6
    del job
    for sim in sims + [one]:
        sim.close()


def test_native_rccl_binding_on_one_rank(tm):
    """librccl dlopen'ed by libmpmhip: unique id, ncclCommInitRank, the loopback self-test (all-gather + grouped send / receive
    to self) and a tiled_advance over MPMHIP_WIRE_RCCL with the one rank a 1-GPU box allows (no halo boxes: the substeps
    equal plain ones).  The two-rank case is test_two_ranks_over_rccl_match_one_ctx[native-*] (needs two GPUs)."""
    import ctypes as C

    from taichi_mpm_amd import _lib, tiled
    s = _two_material_state()
    one = _sim(tm, s, np.ones(s.n, bool), np.arange(s.n), s.n + 1024)
    sim = _sim(tm, s, np.ones(s.n, bool), np.arange(s.n), s.n + 1024)
    L = sim._L
    ident = (C.c_uint8 * _lib.COMM_ID_BYTES)()
    assert L.mpmhip_comm_unique_id(ident) == 0, L.mpmhip_last_error(None)
    assert any(ident)
    sim._check(L.mpmhip_comm_init(sim._ctx, ident, 0, 1))
    sim._check(L.mpmhip_comm_selftest(sim._ctx))
    part = tiled.Partition.balanced((RES,) * 3, 1, s.x, DX, margin=2)
    e = tiled.HipEngine(sim, 0)
    tiled.native_setup(e, part, 0, _lib.WIRE_RCCL)
    sim._check(L.mpmhip_tiled_advance(sim._ctx, 6))
    one.run_substeps(6)
    a, b = one.get_particles(), sim.get_particles()
    assert np.array_equal(a["id"], b["id"]) and np.abs(a["x"] - b["x"]).max() <= 1e-6 and rel_l2(a["F"], b["F"]) <= 1e-5
    assert tiled.native_state(e)["substeps"] == 6
    # the scalars of a job travel inside the library too (SURVEY 8(e) collective 3): ncclAllReduce, here over the one rank
    v = (C.c_double * 3)(1.5, -2.0, 7.0)
    sim._check(L.mpmhip_tiled_reduce(sim._ctx, v, 3, 0))
    assert list(v) == [1.5, -2.0, 7.0]
    sim._check(L.mpmhip_tiled_reduce(sim._ctx, v, 3, 1))
    assert list(v) == [1.5, -2.0, 7.0]
    tot = (C.c_int64 * 4)()
    sim._check(L.mpmhip_tiled_totals(sim._ctx, tot))
    assert tot[0] == len(b["id"]) and tot[1] > 0 and tot[2] == 0
    k1, p1, k2, p2 = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    assert L.mpmhip_calculate_energy(one._ctx, C.byref(k1), C.byref(p1)) in (0, -5)  # (-5: sand has no potential_energy(); kinetic valid)
    assert L.mpmhip_calculate_energy(sim._ctx, C.byref(k2), C.byref(p2)) in (0, -5)
    assert np.isclose(k1.value, k2.value, rtol=1e-6) and k1.value > 0
    sim._check(L.mpmhip_comm_destroy(sim._ctx))
    sim.close(); one.close()


# ------------------------------------------------------------------------------------------ two processes, one GPU
def _proc_worker(rank, world, port, steps, q):
    import os

    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import taichi_mpm_amd as tm
        from taichi_mpm_amd import tiled
        tm.load()
        s = _two_material_state()
        ids = np.arange(s.n)
        part = tiled.Partition.balanced((RES,) * 3, world, s.x, DX, margin=2)
        owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
        sim = _sim(tm, s, owner == rank, ids, s.n + 1024)
        job = tiled.TiledJob(tiled.HipEngine(sim, 0), part, tiled.StagedDistComm(dist), migrate_interval=2)
        job.run(steps)
        job.synchronize()
        p = sim.get_particles(sort_by_id=False)
        q.put((rank, job.r.migrated_out, {k: p[k] for k in ("x", "v", "F", "id", "gid")}))
        sim.close()
    finally:
        dist.destroy_process_group()


def test_two_processes_on_one_gpu_match_one_ctx(tm):
    """the distributed TiledJob (one process per rank, torch.distributed) with the HIP engine: two ranks share this
    GPU, device buffers staged through gloo — everything but the wire is what `bench.py --gpus 2` runs"""
    import socket

    import torch.multiprocessing as mp
    s = _two_material_state()
    steps = 12
    one = _sim(tm, s, np.ones(s.n, bool), np.arange(s.n), s.n + 1024)
    one.run_substeps(steps)
    ref = one.get_particles()
    one.close()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_proc_worker, args=(r, 2, port, steps, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1] + res[1][1] > 0  # migration happened
    got = {k: np.concatenate([r[2][k] for r in res]) for k in res[0][2]}
    order = np.argsort(got["id"], kind="stable")
    got = {k: v[order] for k, v in got.items()}
    assert np.array_equal(got["id"], ref["id"]) and np.array_equal(got["gid"], ref["gid"])
    assert np.abs(got["x"] - ref["x"]).max() <= 1e-6
    assert rel_l2(got["v"], ref["v"]) <= 1e-4 and rel_l2(got["F"], ref["F"]) <= 1e-4


def _native_worker(rank, world, port, steps, wire, overlap, device, q):
    import os

    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("MPMHIP_TILE_WAIT_S", "10")  # a peer that never arrives costs an error, not the box
    torch.cuda.set_device(device)
    dist.init_process_group("gloo", rank=rank, world_size=world)  # control plane only: 64 / 128 bytes once, barriers
    try:
        import taichi_mpm_amd as tm
        from taichi_mpm_amd import tiled
        tm.load()
        s = _two_material_state()
        part = tiled.Partition.balanced((RES,) * 3, world, s.x, DX, margin=2)
        owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
        from taichi_mpm_amd.mpm import F_ID
        sel, ids = owner == rank, np.arange(s.n)
        sim = tm.create_simulation3("mpm")
        sim.initialize(dict(res=(RES,) * 3, delta_x=DX, base_delta_t=DT, max_particles=s.n + 1024, reorder_interval=0, device=device))
        ls = tm.mpm.LevelSet(friction=0.4)
        for p in PLANES:
            ls.add_plane(p[:3], d=p[3])
        sim.set_levelset(ls)
        names = {v: k for k, v in tm.MATERIAL_IDS.items()}
        for gi in range(len(s.gtype)):
            m = sel & (s.gid == gi)
            sim.add_particles(dict(type=names[int(s.gtype[gi])], positions=s.x[m], velocities=s.v[m], F=s.F[m], B=s.B[m], aux=s.aux[m],
                                   params=s.gparams[gi]))
        order = np.concatenate([np.nonzero(sel & (s.gid == gi))[0] for gi in range(len(s.gtype))])
        sim.upload(F_ID, ids[order].astype(np.int32))
        job = tiled.NativeTiledJob(tiled.HipEngine(sim, device), part, rank, world, wire=wire, dist=dist, migrate_interval=2,
                                   overlap=overlap)
        job.run(steps)
        job.synchronize()
        # scalars of the whole job, reduced inside the library (mpmhip_tiled_reduce: rows + epochs over the IPC wire, ncclAllReduce)
        import ctypes as C
        ke, pe = C.c_double(), C.c_double()
        rc = sim._L.mpmhip_calculate_energy(sim._ctx, C.byref(ke), C.byref(pe))  # (-5: sand has no potential_energy(); kinetic valid)
        extra = {"energy_rc": int(rc), "kinetic": ke.value, "sum": job.reduce([rank + 1.0, 10.0 * (rank + 1)], "sum"),
                 "max": job.reduce([float(rank), -float(rank)], "max"), "min": job.reduce([float(rank)], "min"), "totals": job.totals()}
        job.run(2)  # (the epochs of the energy's exchange are part of the protocol: the run goes on)
        job.synchronize()
        dist.barrier()  # nobody unmaps an arena a peer may still write to
        p = sim.get_particles(sort_by_id=False)
        q.put((rank, job.state()[0], {k: p[k] for k in ("x", "v", "F", "id", "gid")}, extra))
        sim.close()
    finally:
        dist.destroy_process_group()


def _run_native_ranks(tm, wire, overlap, devices):
    import socket

    import torch.multiprocessing as mp
    s = _two_material_state()
    import ctypes as C
    steps, world = 12, len(devices)
    one = _sim(tm, s, np.ones(s.n, bool), np.arange(s.n), s.n + 1024)
    one.run_substeps(steps)
    ke, pe = C.c_double(), C.c_double()
    assert one._L.mpmhip_calculate_energy(one._ctx, C.byref(ke), C.byref(pe)) in (0, -5)
    n_live = one.get_num_particles()
    one.run_substeps(2)
    ref = one.get_particles()
    one.close()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_native_worker, args=(r, world, port, steps, wire, overlap, devices[r], q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(r[1]["substeps"] == steps + 2 and r[1]["migrations"] == (steps + 2) // 2 for r in res), [r[1] for r in res]
    for r in res:  # every rank holds the whole job's numbers
        x = r[3]
        assert x["energy_rc"] in (0, -5) and np.isclose(x["kinetic"], ke.value, rtol=1e-6), (x["kinetic"], ke.value)
        assert x["sum"] == [sum(range(1, world + 1)), 10.0 * sum(range(1, world + 1))]
        assert x["max"] == [world - 1.0, 0.0] and x["min"] == [0.0]
        assert x["totals"]["particles"] == n_live and x["totals"]["error"] == 0
    assert res[0][3]["kinetic"] == res[1][3]["kinetic"]  # reduced in rank order: bit-identical on every rank
    assert sum(r[1]["migrated_out"] for r in res) > 0  # migration happened
    got = {k: np.concatenate([r[2][k] for r in res]) for k in res[0][2]}
    order = np.argsort(got["id"], kind="stable")
    got = {k: v[order] for k, v in got.items()}
    assert np.array_equal(got["id"], ref["id"]) and np.array_equal(got["gid"], ref["gid"])
    assert np.abs(got["x"] - ref["x"]).max() <= 1e-6
    assert rel_l2(got["v"], ref["v"]) <= 1e-4 and rel_l2(got["F"], ref["F"]) <= 1e-4


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap_split"])
def test_two_processes_over_the_ipc_wire_match_one_ctx(tm, overlap):
    """MPMHIP_WIRE_IPC between two PROCESSES (sharing this GPU): each maps the other's receive arena with
    hipIpcOpenMemHandle; k_halo_pack writes the boxes straight into it and publishes the substep's epoch, the reader polls
    it; migration rows and records travel the same way.  Python moves 64 bytes per rank once (the handles, over gloo)."""
    _run_native_ranks(tm, "ipc", overlap, [0, 0])


@pytest.mark.parametrize("wire", ["rccl", "ipc"])
@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap_split"])
def test_two_ranks_on_two_gpus_over_the_native_wires_match_one_ctx(tm, wire, overlap):
    """the real wires: two processes, two GPUs — ncclSend / ncclRecv groups issued by the library, or peer writes over xGMI
    into IPC-mapped buffers.  Needs >= 2 GPUs: skipped on the 1-GPU boxes of the development pool."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    _run_native_ranks(tm, wire, overlap, [0, 1])


@pytest.mark.parametrize("nproc,bricks,hook,config", [(2, "2x1x1", "gloo", "c2"), (8, "2x2x2", "ipc", "c2"), (2, "2x1x1", "staged", "c2"),
                                                       (2, "2x1x1", "refuse", "c2"), (2, "2x1x1", "fallback", "c2"), (8, "2x2x2", "ipc", "c5"),
                                                       (2, "2x1x1", "ipc+both", "c2")])
def test_bench_multi_rank_path_end_to_end_on_one_gpu(tm, nproc, bricks, hook, config):
    """`bench.py --gpus N` exactly as the driver launches it (torch.distributed.run, one process per rank) on a box with fewer
    GPUs than ranks.  hook "ipc" (MPMHIP_BENCH_BACKEND=ipc): the ranks share this GPU and run the library's own data plane over
    the IPC wire — native loop, peer writes, native migration; "gloo": the round-3 Python path staged through gloo.  Without
    a hook the RCCL probe fails (two ranks on one device): the job then takes the library's IPC wire — still a native data plane
    ("fallback") — and, with that ruled out too (MPMHIP_NO_IPC_FALLBACK=1), must EXIT NON-ZERO ("refuse") rather than silently
    turn a scaling run into a host-staged one, unless --allow-staged is given ("staged").  Checks the ONE-JSON-line contract and the
    whole-job aggregation of the N > 1 path.  config c5 = BASELINE configs[4] (512^3 grid, 8 clusters, two materials) tiled over 8
    ranks, at a reduced cluster size (--cells 16)."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.pop("MPMHIP_BENCH_BACKEND", None)
    both = hook.endswith("+both")  # --wire both: the job is measured, re-wired (plan, arena, connection built again) and measured again
    hook = hook.split("+")[0]
    if hook in ("gloo", "ipc"):
        env["MPMHIP_BENCH_BACKEND"] = hook
    env.setdefault("MPMHIP_TILE_WAIT_S", "20")
    env.pop("MPMHIP_NO_IPC_FALLBACK", None)
    if hook in ("refuse", "staged"):
        env["MPMHIP_NO_IPC_FALLBACK"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", str(nproc), "--config", config,
           "--steps", "8", "--warmup", "4", "--full"] + (["--cells", "16"] if config == "c5" else []) + (["--allow-staged"] if hook == "staged" else []) + \
          (["--wire", "both"] if both else [])
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=root)
    if hook == "refuse":
        assert r.returncode != 0 and "refusing to fall back" in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
        assert not [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
        return
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == nproc and d["steps"] == 8 and d["warmup"] == 4 and d["scaling"] == "strong"
    assert d["config"]["particles"] == (1000000 if config == "c2" else 8 * 16 ** 3 * 8)  # all ranks' particles: whole-job aggregate
    assert ("REDUCED" in d["config"]["workload"]) == (config == "c5")
    assert d["value"] > 0 and d["unit"] == "particle-steps/s" and d["roofline"]["kernel"] in ("k_g2p", "k_p2g")
    assert bricks + " bricks" in d["config"]["parallelism"]
    if hook in ("ipc", "fallback"):
        assert d["config"]["wire"].startswith("IPC peer writes") and "library's own data plane" in d["config"]["parallelism"]
        assert ("RCCL probe failed" in d["config"]["wire"]) == (hook == "fallback")
    else:
        assert d["config"]["wire"].startswith("gloo") and ("probe failed" in d["config"]["wire"]) == (hook == "staged")
    ov = d["config"]["overlap_split"]  # both ways timed before the measurement, the faster one kept (bench.py)
    assert ov["kept"] in ("on", "off") and ov["ms_per_step_on"] > 0 and ov["ms_per_step_off"] > 0
    # one run answers the questions of a multi-GPU run: every rank's phase table (max / min / rank by rank), where ranks wait
    # (`exchange`), what the plan moves, migrations — and, on the native data plane, the job's totals reduced inside the library
    t = d["tiled"]
    assert len(t["per_rank"]) == nproc and set(t["max"]) >= {"sort", "p2g", "exchange", "grid", "g2p", "ms_per_step", "halo_bytes_per_substep"}
    assert all(t["max"][k] >= t["min"][k] >= 0 for k in t["max"]) and t["max"]["g2p"] > 0
    assert sum(r["particles"] for r in t["per_rank"]) == d["config"]["particles"]
    if hook in ("ipc", "fallback"):
        # (c5: the clusters never meet — every rank's halo boxes are cut to its own occupancy, so NOTHING is exchanged; until round 6
        # the boxes were cut to the job's bounding box only and 8 - 39 MB of empty slabs per rank travelled every substep)
        assert t["wire"] == "ipc" and (t["min"]["halo_bytes_per_substep"] > 0) == (config != "c5") and (t["max"]["halo_bytes_per_substep"] > 0) == (config != "c5")
        assert t["totals"]["particles"] == d["config"]["particles"] and t["totals"]["error"] == 0
    if both:
        o = t["other_wire"]
        assert "error" not in o, o
        assert o["wire"] == "ipc" and o["ms_per_step"] > 0 and len(o["per_rank"]) == nproc and o["min"]["halo_bytes_per_substep"] > 0
    else:
        assert "other_wire" not in t


def test_bench_tiled_job_over_rccl_single_rank(tm):
    """MPMHIP_FORCE_TILED=1: the tiled job (halo plan, migration scan, all_to_all / all_gather on DEVICE buffers) over a
    real RCCL communicator — with the one rank a 1-GPU box allows.  The transport probe must pick RCCL."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MPMHIP_FORCE_TILED="1")
    env.pop("MPMHIP_BENCH_BACKEND", None)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--config", "c2", "--steps", "8", "--warmup", "4",
                        "--no-cpu-baseline"], capture_output=True, text=True, env=env, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["config"]["particles"] == 1000000 and d["value"] > 0
    assert d["config"]["wire"].startswith("RCCL"), d["config"]["wire"]


def _rccl_worker(rank, world, port, steps, overlap, q):
    import os

    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    try:
        import taichi_mpm_amd as tm
        from taichi_mpm_amd import tiled
        tm.load()
        s = _two_material_state()
        ids = np.arange(s.n)
        part = tiled.Partition.balanced((RES,) * 3, world, s.x, DX, margin=2)
        owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
        from taichi_mpm_amd.mpm import F_ID
        sim = tm.create_simulation3("mpm")
        sim.initialize(dict(res=(RES,) * 3, delta_x=DX, base_delta_t=DT, max_particles=s.n + 1024, reorder_interval=0, device=rank))
        ls = tm.mpm.LevelSet(friction=0.4)
        for p in PLANES:
            ls.add_plane(p[:3], d=p[3])
        sim.set_levelset(ls)
        names = {v: k for k, v in tm.MATERIAL_IDS.items()}
        sel = owner == rank
        for gi in range(len(s.gtype)):
            m = sel & (s.gid == gi)
            sim.add_particles(dict(type=names[int(s.gtype[gi])], positions=s.x[m], velocities=s.v[m], F=s.F[m], B=s.B[m], aux=s.aux[m],
                                   params=s.gparams[gi]))
        order = np.concatenate([np.nonzero(sel & (s.gid == gi))[0] for gi in range(len(s.gtype))])
        sim.upload(F_ID, ids[order].astype(np.int32))
        job = tiled.TiledJob(tiled.HipEngine(sim, rank), part, tiled.DistComm(dist, torch.device("cuda", rank)), migrate_interval=2,
                             overlap=overlap)
        job.run(steps)
        job.synchronize()
        p = sim.get_particles(sort_by_id=False)
        q.put((rank, job.r.migrated_out, {k: p[k] for k in ("x", "v", "F", "id", "gid")}))
        sim.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
def test_two_ranks_over_rccl_match_one_ctx(tm, overlap):
    """the real wire: two processes, two GPUs, halo all-sum and migration over RCCL (DistComm.all_to_all[_async] with
    device buffers), exchange/compute overlap off and on, against the single-ctx run.  Needs >= 2 GPUs: skipped on the
    1-GPU boxes of the development pool, runs wherever the suite meets a multi-GPU node."""
    import socket

    import torch
    import torch.multiprocessing as mp
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    s = _two_material_state()
    steps = 12
    one = _sim(tm, s, np.ones(s.n, bool), np.arange(s.n), s.n + 1024)
    one.run_substeps(steps)
    ref = one.get_particles()
    one.close()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rccl_worker, args=(r, 2, port, steps, overlap, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    got = {k: np.concatenate([r[2][k] for r in res]) for k in res[0][2]}
    order = np.argsort(got["id"], kind="stable")
    got = {k: v[order] for k, v in got.items()}
    assert res[0][1] + res[1][1] > 0
    assert np.array_equal(got["id"], ref["id"]) and np.abs(got["x"] - ref["x"]).max() <= 1e-6
    assert rel_l2(got["v"], ref["v"]) <= 1e-4 and rel_l2(got["F"], ref["F"]) <= 1e-4
