"""GPU tests of re-cutting a running tiled job (include/mpmhip.h: "Re-cutting a running job"): the histogram of the live particles
against numpy, the redistribution behind new cuts (every particle on its owner, records bit for bit, rounds, the capacity rule),
job.rebalance() on the virtual job and on two processes over the IPC wire, and the physics against one ctx.  The scenes and helpers
are those of tests/test_gpu_tiled.py, copied."""
import ctypes as C

import numpy as np
import pytest

from tests.common import lattice_cube, make_state, rel_l2

pytestmark = pytest.mark.gpu

RES, DX, DT = 32, 1.0 / 32, 1e-4
PLANES = [(0.0, 1.0, 0.0, -0.3)]
FIELDS = ("x", "v", "F", "B", "aux", "gid", "id")


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


def _sim(tm, s, sel, ids, cap, **cfg):
    from taichi_mpm_amd.mpm import F_ID
    sim = tm.create_simulation3("mpm")
    sim.initialize(dict(dict(res=(RES,) * 3, delta_x=DX, base_delta_t=DT, max_particles=cap, reorder_interval=0), **cfg))
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


def _same_bits(a, b):
    return all(a[k].shape == b[k].shape and np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8))
               for k in FIELDS)


def _id_sets(sims):
    return [set(int(i) for i in sim.get_particles(sort_by_id=False)["id"]) for sim in sims]


# ------------------------------------------------------------------------------------------------ 1. the histogram
def _ulps_from_a_face(x, dx):
    """smallest distance of X - 0.5 (X = fl(x * fl(1 / dx)), tiled.base_cells' product) from an integer, in ulps of X"""
    X = np.asarray(x, np.float32) * np.float32(1.0 / dx)
    d = np.abs((X.astype(np.float64) - 0.5) - np.rint(X.astype(np.float64) - 0.5))
    return float((d / np.spacing(np.maximum(X, np.float32(1.0))).astype(np.float64)).min()) if X.size else np.inf


def _plain(tm, res, x, **cfg):
    sim = tm.create_simulation3("mpm")
    sim.initialize(dict(dict(res=res, delta_x=DX, base_delta_t=DT, max_particles=max(len(x), 1) + 64, reorder_interval=0), **cfg))
    sim.set_levelset(tm.mpm.LevelSet())
    if len(x):
        sim.add_particles(dict(type="jelly", positions=np.asarray(x, np.float32)))
    sim._ensure_ctx()
    return sim


def _uniform(seed, n, lo, hi):
    """n positions uniform over the cells [lo, hi) per axis"""
    rng = np.random.RandomState(seed)
    return ((np.asarray(lo) + rng.rand(n, 3) * (np.asarray(hi) - np.asarray(lo))) * DX).astype(np.float32)


def _check_histogram(sim, res):
    from taichi_mpm_amd import tiled
    x = sim.get_particles(sort_by_id=False)["x"]
    assert _ulps_from_a_face(x, DX) > 4.0, "the scene must hold no particle within 4 ulp of a cell face"
    b = np.clip(tiled.base_cells(x, DX), 0, np.asarray(res) - 1) if len(x) else np.zeros((0, 3), np.int32)
    hists, lo, hi, total = tiled.live_histograms(sim)
    assert total == len(x)
    for a in range(3):
        assert hists[a].dtype == np.int64 and np.array_equal(hists[a], np.bincount(b[:, a], minlength=res[a]))
    if len(x):
        assert np.array_equal(lo, b.min(0)) and np.array_equal(hi, b.max(0) + 1)
    else:
        assert not lo.any() and not hi.any()
    return hists, total


@pytest.fixture(scope="module")
def two_material_after_5(tm):
    s = _two_material_state()
    sim = _sim(tm, s, np.ones(s.n, bool), np.arange(s.n), s.n + 1024)
    sim.run_substeps(5)
    yield sim
    sim.close()


def test_histogram_of_the_two_material_state_and_of_its_dead_slots(tm, two_material_after_5):
    """~14 k particles after 5 substeps; then delete_particles_inside_level_set leaves dead slots between the live ones, which the
    histogram must not count; and the call moves nothing: the records before and after are the same bits"""
    sim = two_material_after_5
    before = sim.get_particles()
    _, total = _check_histogram(sim, (RES,) * 3)
    assert total == len(before["id"]) > 13000
    assert _same_bits(before, sim.get_particles())
    sim.set_levelset(tm.mpm.LevelSet().add_plane((1.0, 0.0, 0.0), d=-0.45))  # everything left of x = 0.45 is inside
    sim.general_action(dict(action="delete_particles_inside_level_set"))
    slots = int(sim._L.mpmhip_num_slots(sim._ctx))
    _, left = _check_histogram(sim, (RES,) * 3)
    assert 0 < left < total and slots > left  # dead slots were there to be skipped


# (add_particles ignores positions within 7 cells of the grid's faces, as the reference does: the scenes stay clear of them)
CASES = {
    "grid_24_40_32": dict(res=(24, 40, 32), n=5000, x=lambda: _uniform(51, 5000, (8, 8, 8), (16, 32, 24))),
    "1037_particles": dict(res=(RES,) * 3, n=1037, x=lambda: _uniform(52, 1037, (8, 8, 8), (24, 24, 24))),
    "1_particle": dict(res=(RES,) * 3, n=1, x=lambda: _uniform(53, 1, (8, 8, 8), (24, 24, 24))),
    "0_particles": dict(res=(RES,) * 3, n=0, x=lambda: np.zeros((0, 3), np.float32)),
    "4096_in_one_cell": dict(res=(RES,) * 3, n=4096, x=lambda: _uniform(54, 4096, (10.55, 17.55, 12.55), (11.45, 18.45, 13.45))),
    # base cell res - 1 along y: X in [res - 0.45, res - 0.05) — uploaded positions (clean_boundary off: such particles are legal)
    "last_cell": dict(res=(RES,) * 3, n=300, x=lambda: _uniform(55, 300, (8, 8, 8), (24, 24, 24)), cfg=dict(clean_boundary=False),
                      move_to=lambda: _uniform(56, 300, (20, 31.55, 20), (31.95, 31.95, 31.95))),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_histogram_against_numpy(tm, case):
    from taichi_mpm_amd.mpm import F_X
    c = CASES[case]
    sim = _plain(tm, c["res"], c["x"](), **c.get("cfg", {}))
    if "move_to" in c:
        sim.upload(F_X, c["move_to"]())
    hists, total = _check_histogram(sim, c["res"])
    assert total == c["n"]
    if case == "4096_in_one_cell":
        assert [int(h.max()) for h in hists] == [4096] * 3
    if case == "last_cell":
        assert hists[1][RES - 1] == 300
    sim.close()


def test_histograms_of_three_ranks_add_up_to_the_one_ctx_histogram(tm):
    from taichi_mpm_amd import tiled
    s = _two_material_state()
    n, ids = s.n, np.arange(s.n)
    part = tiled.Partition.balanced((RES,) * 3, 3, s.x, DX, margin=2, dims=(1, 3, 1))
    owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
    one = _sim(tm, s, np.ones(n, bool), ids, n + 64)
    sims = [_sim(tm, s, owner == r, ids, n + 64) for r in range(3)]
    job = tiled.NativeVirtualJob([tiled.HipEngine(sim, 0) for sim in sims], part, migrate_interval=2)
    rows = [tiled.live_histograms(sim) for sim in sims]  # (a ctx with a partition and a plan)
    want = tiled.live_histograms(one)
    for a in range(3):
        assert np.array_equal(sum(r[0][a] for r in rows), want[0][a])
    assert sum(r[3] for r in rows) == want[3] == n
    assert np.array_equal(np.min([r[1] for r in rows], 0), want[1]) and np.array_equal(np.max([r[2] for r in rows], 0), want[2])
    del job
    for sim in sims + [one]:
        sim.close()


# ------------------------------------------------------------------------------------------------ 2 / 4 / 5 / 9. the moving blob
def _blob(tm, caps=None, inbox_records=None, x_cuts=None):
    """the 3 x 1 x 1 job of test_native_migration_follows_a_moving_blob after its 50 substeps (caps: its own unless given; x_cuts:
    other cut planes than its balanced ones)"""
    from taichi_mpm_amd import tiled
    x = lattice_cube(RES, 8, 20, DX, jitter=0.2, seed=31)
    s = make_state(x, "jelly", DX, perturb_F=0.0, seed=32, vel_scale=0.0)
    s.v[:] = (25.0, 0.0, 0.0)
    s.B[:] = 0
    n = s.n
    part = tiled.Partition.balanced((RES,) * 3, 3, s.x, DX, margin=2, dims=(3, 1, 1))
    if x_cuts:
        part = tiled.Partition((RES,) * 3, (3, 1, 1), [x_cuts, [0, RES], [0, RES]], 2)
    b = tiled.base_cells(s.x, DX)
    part.clip = (list(map(int, b.min(0) - 3)), list(map(int, b.max(0) + 6)))
    owner = part.rank_of_cells(b)
    own = [int((owner == r).sum()) for r in range(3)]
    caps = caps or [own[0] + 64, int(own[1] * 1.3), n]
    sims = [_sim(tm, s, owner == r, np.arange(n), caps[r]) for r in range(3)]
    for sim in sims:
        sim.set_levelset(tm.mpm.LevelSet())
    engines = [tiled.HipEngine(sim, 0) for sim in sims]
    job = tiled.NativeVirtualJob(engines, part, inbox_records=n)
    job.run(50)
    if inbox_records:  # the same job set up again with a small inbox (what a re-cut's set-up keeps)
        job = tiled.NativeVirtualJob(engines, job.part, inbox_records=inbox_records)
    return job, sims, n


def _owners_after(sims, part):
    """(records by id, per-rank counts numpy expects under `part`)"""
    from taichi_mpm_amd import tiled
    got = _gather(sims)
    return got, np.bincount(part.rank_of_cells(tiled.base_cells(got["x"], DX)), minlength=part.world)


def _no_leaver_anywhere(job):
    for e in job.engines:
        counts, _, _, _ = e.migration_scan()
        assert not counts.any(), counts


@pytest.fixture(scope="module")
def blob_recut(tm):
    """case 2, run once: what the later cases compare with"""
    from taichi_mpm_amd import tiled
    job, sims, n = _blob(tm)
    before = _gather(sims)
    held = [sim.get_num_particles() for sim in sims]
    hists = [sum(tiled.live_histograms(sim)[0][a] for sim in sims) for a in range(3)]
    old_cuts = [list(c) for c in job.part.cuts]
    result = job.rebalance(force=True)
    out = dict(job=job, sims=sims, n=n, before=before, held=held, hists=hists, old_cuts=old_cuts, result=result, ids=_id_sets(sims))
    yield out
    for sim in sims:
        sim.close()


def test_recut_of_the_moving_blob(tm, blob_recut):
    B = blob_recut
    job, sims, result = B["job"], B["sims"], B["result"]
    assert result["recut"] and result["cuts"] == job.part.cuts != B["old_cuts"] and result["moved"] > 0 and result["rounds"] >= 1
    after, want = _owners_after(sims, job.part)
    assert [sim.get_num_particles() for sim in sims] == want.tolist()
    _no_leaver_anywhere(job)
    assert job.totals()["error"] == 0
    assert _same_bits(after, B["before"]) and len(after["id"]) == B["n"]
    assert result["imbalance_after"] < result["imbalance_before"]
    assert np.isclose(result["imbalance_before"], max(B["held"]) * 3 / B["n"]) and np.isclose(result["imbalance_after"], want.max() * 3 / B["n"])
    job.run(10)
    assert job.totals()["error"] == 0
    st = job.state()
    assert all(t["replans"] >= 1 and t["substeps"] == 10 for t in st), st  # the planning scan cut fresh boxes; the set-up restarted the counters
    assert job.substeps == 60
    got = _gather(sims)
    assert np.array_equal(got["id"], np.arange(B["n"])) and np.allclose(got["v"][:, 0], 25.0, rtol=1e-3)


def test_balanced_cuts_through_the_c_entry(tm, blob_recut):
    from taichi_mpm_amd import tiled
    L = tm.load()
    for a, parts in zip(range(3), (3, 1, 1)):
        h = np.ascontiguousarray(blob_recut["hists"][a], np.int64)
        for p in (parts, 2, 5, 16):
            out = (C.c_int32 * (p + 1))()
            assert L.mpmhip_balanced_cuts(RES, p, h.ctypes.data_as(C.POINTER(C.c_int64)), out) == 0
            assert list(out) == [int(c) for c in tiled.balanced_cuts(None, RES, p, hist=h)]
    assert blob_recut["result"]["cuts"][0] == [int(c) for c in tiled.balanced_cuts(None, RES, 3, hist=blob_recut["hists"][0])]
    assert L.mpmhip_balanced_cuts(4, 5, h.ctypes.data_as(C.POINTER(C.c_int64)), out) < 0  # more parts than cells


def test_rounds_with_a_small_inbox(tm, blob_recut):
    """case 2 with inbox_records = 256 (and slots to spare on every rank, so that every round offers the whole inbox): the rounds are
    what the host rule predicts for the table numpy derives, and the ranks end with the id sets of case 2"""
    from taichi_mpm_amd import tiled
    from tests.test_tiled_recut_cpu import I64, U32, host_lib
    job, sims, n = _blob(tm, caps=[n_ + 1024 for n_ in [blob_recut["n"]] * 3], inbox_records=256)
    holder = np.empty(n, np.int64)
    for r, ids in enumerate(_id_sets(sims)):
        holder[sorted(ids)] = r
    before = _gather(sims)
    result = job.rebalance(force=True)
    assert result["recut"] and result["cuts"] == blob_recut["result"]["cuts"]
    got, want = _owners_after(sims, job.part)
    owner = job.part.rank_of_cells(tiled.base_cells(got["x"], DX))
    table = np.zeros((3, 3), np.int64)
    np.add.at(table, (holder, owner), 1)
    np.fill_diagonal(table, 0)
    room = np.full(3, 256, np.uint32)
    predicted = int(host_lib().tr_rounds_needed(3, table.ctypes.data_as(I64), room.ctypes.data_as(U32)))
    assert result["rounds"] == predicted >= -(-int(table.sum(0).max()) // 256) and result["rounds"] > 1
    assert result["moved"] == table.sum()
    assert _id_sets(sims) == blob_recut["ids"] and [sim.get_num_particles() for sim in sims] == want.tolist()
    assert _same_bits(got, before)
    _no_leaver_anywhere(job)
    assert job.totals()["error"] == 0
    for sim in sims:
        sim.close()


def test_capacity_is_checked_before_anything_moves(tm):
    """the blob under cut planes that leave ranks 0 and 1 a sixth of it each: after the 50 substeps it has left them for rank 2, and a
    re-cut hands each rank a third back.  Rank 0 holds a quarter: it must grow."""
    from taichi_mpm_amd import _lib, tiled
    lop = [0, 10, 12, RES]

    def expect(sims):
        got = _gather(sims)
        new = tiled.Partition.balanced((RES,) * 3, 3, got["x"], DX, margin=2, dims=(3, 1, 1))
        owner = new.rank_of_cells(tiled.base_cells(got["x"], DX))
        return new, np.bincount(owner, minlength=3).tolist(), [set(int(i) for i in got["id"][owner == r]) for r in range(3)]

    # --- the C entries: set-up with the new cuts, then the redistribution
    n = 13824  # (the blob's particles)
    cap0 = n // 4
    job, sims, n_blob = _blob(tm, caps=[cap0, n + 1024, n + 1024], x_cuts=lop)
    assert n_blob == n
    L, K = sims[0]._L, 3
    held = [sim.get_num_particles() for sim in sims]
    new, need, ids = expect(sims)
    assert int(L.mpmhip_capacity(sims[0]._ctx)) == cap0 and held[0] < cap0 < need[0] and sum(need) == n
    job.synchronize()
    for r, e in enumerate(job.engines):
        tiled.native_setup(e, new, r, _lib.WIRE_LOCAL, None, False, n)
    arr = (C.c_void_p * K)(*[e.ctx for e in job.engines])
    assert L.mpmhip_tiled_connect_local(arr, K) == 0
    before = _id_sets(sims)
    info = (C.c_int64 * (4 * K))()
    assert L.mpmhip_tiled_redistribute_group(arr, K, info) == _lib.ECAPACITY
    assert "rank 0 " in L.mpmhip_last_error(sims[0]._ctx).decode()
    assert [int(v) for v in info] == [0, 0, 0, need[0]] + [0] * 8  # every rank refused; rank 0 needs room, nothing was sent
    assert all("rank 0 " in L.mpmhip_last_error(sim._ctx).decode() for sim in sims)
    assert _id_sets(sims) == before and [sim.get_num_particles() for sim in sims] == held  # nothing has moved
    assert L.mpmhip_reserve(sims[0]._ctx, need[0]) == 0
    assert L.mpmhip_tiled_redistribute_group(arr, K, info) == 0
    assert _id_sets(sims) == ids and [int(info[4 * r + 3]) for r in range(K)] == [0] * K
    assert sum(int(info[4 * r]) for r in range(K)) == sum(int(info[4 * r + 1]) for r in range(K)) == n - sum(len(a & b) for a, b in zip(before, ids))
    for sim in sims:
        sim.close()
    # --- job.rebalance does the same by itself
    job, sims, _ = _blob(tm, caps=[cap0, n + 1024, n + 1024], x_cuts=lop)
    new, need, ids = expect(sims)
    result = job.rebalance(force=True)
    assert result["recut"] and result["grew"] == [0] and result["cuts"] == new.cuts and _id_sets(sims) == ids
    assert int(L.mpmhip_capacity(sims[0]._ctx)) >= need[0] + need[0] // 8
    _no_leaver_anywhere(job)
    job.run(4)
    assert job.totals()["error"] == 0
    for sim in sims:
        sim.close()


# ------------------------------------------------------------------------------------------------ 3 / 6 / 7. physics, no-ops, determinism
def _lopsided(world):
    """bricks cut well off the particles' centre (cells 9 .. 21): a re-cut has something to move"""
    from taichi_mpm_amd import tiled
    dims = tiled.brick_dims(world)
    return tiled.Partition((RES,) * 3, dims, [[0, 12, RES] if d == 2 else [0, RES] for d in dims], 2)


def _run_with_a_recut(tm, world, halo_by_rccl=False, **cfg):
    from taichi_mpm_amd import tiled
    s = _two_material_state()
    n, ids = s.n, np.arange(s.n)
    part = _lopsided(world)
    owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
    sims = [_sim(tm, s, owner == r, ids, n + 1024, **cfg) for r in range(world)]
    job = tiled.NativeVirtualJob([tiled.HipEngine(sim, 0) for sim in sims], part, migrate_interval=2, halo_by_rccl=halo_by_rccl)
    job.run(6)
    result = job.rebalance(force=True)
    job.run(6)
    assert job.totals()["error"] == 0
    return job, sims, result


@pytest.fixture(scope="module")
def one_ctx_after_12(tm):
    s = _two_material_state()
    one = _sim(tm, s, np.ones(s.n, bool), np.arange(s.n), s.n + 1024)
    one.run_substeps(12)
    ref = one.get_particles()
    one.close()
    return ref


def _against_one_ctx(got, ref):
    assert np.array_equal(got["id"], ref["id"]) and np.array_equal(got["gid"], ref["gid"])
    assert np.abs(got["x"] - ref["x"]).max() <= 1e-6
    assert rel_l2(got["v"], ref["v"]) <= 1e-4 and rel_l2(got["F"], ref["F"]) <= 1e-4


@pytest.mark.parametrize("halo_by_rccl", [False, True], ids=["peer_writes", "halo_by_rccl"])
def test_a_recut_in_mid_run_leaves_the_physics_alone(tm, one_ctx_after_12, halo_by_rccl):
    job, sims, result = _run_with_a_recut(tm, 8, halo_by_rccl)
    assert result["recut"] and result["moved"] > 0 and result["imbalance_after"] < result["imbalance_before"]
    assert all(t["substeps"] == 6 for t in job.state()) and job.substeps == 12
    _against_one_ctx(_gather(sims), one_ctx_after_12)
    for sim in sims:
        sim.close()


def test_rebalance_is_a_no_op_on_a_balanced_job_and_on_one_rank(tm):
    from taichi_mpm_amd import tiled
    s = _two_material_state()
    n, ids = s.n, np.arange(s.n)
    # 2 bricks: balanced, below the default threshold.  4 bricks (2 x 2 x 1 cut from the marginal histograms: the jittered lattice leaves
    # them 1.18 apart): above it, but the live histograms give the cuts the job already has.  1 brick: nothing to cut.
    for world in (2, 4, 1):
        part = tiled.Partition.balanced((RES,) * 3, world, s.x, DX, margin=2)
        owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
        sims = [_sim(tm, s, owner == r, ids, n + 1024) for r in range(world)]
        job = tiled.NativeVirtualJob([tiled.HipEngine(sim, 0) for sim in sims], part, migrate_interval=2)
        job.run(4)
        state, cuts = job.state(), [list(c) for c in part.cuts]
        result = job.rebalance(force=(world == 1))
        assert result["recut"] is False and result["moved"] == 0 and result["cuts"] == cuts and result["grew"] == []
        assert result["imbalance_before"] == result["imbalance_after"] and (world == 4 or result["imbalance_before"] < 1.15)
        assert job.state() == state and job.part is part
        for sim in sims:
            sim.close()


def test_deterministic_mode_two_runs_end_byte_identical(tm):
    runs = []
    for _ in range(2):
        job, sims, result = _run_with_a_recut(tm, 8, deterministic=True)
        assert result["recut"]
        runs.append(_gather(sims))
        for sim in sims:
            sim.close()
    assert _same_bits(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------ 8. two processes over the IPC wire
def _ipc_worker(rank, world, port, device, q):
    import os

    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("MPMHIP_TILE_WAIT_S", "10")  # a peer that never arrives costs an error, not the box
    torch.cuda.set_device(device)
    dist.init_process_group("gloo", rank=rank, world_size=world)  # control plane only
    try:
        import taichi_mpm_amd as tm
        from taichi_mpm_amd import tiled
        tm.load()
        s = _two_material_state()
        part = _lopsided(world)
        owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
        sim = _sim(tm, s, owner == rank, np.arange(s.n), s.n + 1024, device=device)
        job = tiled.NativeTiledJob(tiled.HipEngine(sim, device), part, rank, world, wire="ipc", dist=dist, migrate_interval=2, overlap=False)
        job.run(6)
        result = job.rebalance(force=True)
        job.run(6)
        job.synchronize()
        totals = job.totals()
        dist.barrier()  # nobody unmaps an arena a peer may still write to
        p = sim.get_particles(sort_by_id=False)
        q.put((rank, result, totals, {k: p[k] for k in FIELDS}))
        sim.close()
    finally:
        dist.destroy_process_group()


def test_two_processes_over_the_ipc_wire_rebalance_like_the_virtual_job(tm, one_ctx_after_12):
    import socket

    import torch.multiprocessing as mp
    world = 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_ipc_worker, args=(r, world, port, 0, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    job, sims, want = _run_with_a_recut(tm, world)
    assert want["recut"] and want["moved"] > 0
    for r in res:
        assert r[1] == want and r[2]["error"] == 0 and r[2]["particles"] == len(one_ctx_after_12["id"])
    assert [set(int(i) for i in r[3]["id"]) for r in res] == _id_sets(sims)
    got = {k: np.concatenate([r[3][k] for r in res]) for k in FIELDS}
    order = np.argsort(got["id"], kind="stable")
    _against_one_ctx({k: v[order] for k, v in got.items()}, one_ctx_after_12)
    _against_one_ctx(_gather(sims), one_ctx_after_12)
    for sim in sims:
        sim.close()
