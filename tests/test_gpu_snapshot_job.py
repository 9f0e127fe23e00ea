"""GPU tests of the snapshot of a tiled job (include/mpmhip.h: "the snapshot of a whole tiled job"): ONE MPMHIP01 blob in canonical
form whatever the bricks — mpmhip_snapshot_save_group on K ctx against the canonical form of the one ctx that holds the same records,
a job that has stepped, re-cut and lost particles, the shapes at which the ranking and the ownership filter can go wrong (each saved
AND loaded into a 2 x 2 x 1 job through chunks of 1000 records), a round trip from 8 ranks to 3, capacity and refusals, the
deterministic mode, and two processes over the IPC wire.  The model is tests/snapshot_job_model.py.  Grid 32^3, dx = 1/32; the scenes
and helpers are those of tests/test_gpu_recut.py and tests/test_gpu_frame_job.py, copied."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import snapshot_job_model as model
from tests.common import lattice_cube, make_state, rel_l2

pytestmark = pytest.mark.gpu

RES, DX, DT = 32, 1.0 / 32, 1e-4
PLANES = [(0.0, 1.0, 0.0, -0.3)]
FIELDS = ("x", "v", "F", "B", "aux", "gid", "id")
EINVAL, ECAPACITY = -1, -4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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


def _against_one_ctx(got, ref):
    assert np.array_equal(got["id"], ref["id"]) and np.array_equal(got["gid"], ref["gid"])
    assert np.abs(got["x"] - ref["x"]).max() <= 1e-6
    assert rel_l2(got["v"], ref["v"]) <= 1e-4 and rel_l2(got["F"], ref["F"]) <= 1e-4


def _uniform(seed, n):
    rng = np.random.RandomState(seed)
    return ((8 + rng.rand(n, 3) * 16) * DX).astype(np.float32)


def _plain_sims(tm, rank_x, rank_ids, cap=None):
    """one ctx per rank holding jelly particles at rank_x[r] with the creation ids rank_ids[r] (tests/test_gpu_frame_job.py)"""
    from taichi_mpm_amd.mpm import F_ID, F_X
    sims = []
    for r, (x, ids) in enumerate(zip(rank_x, rank_ids)):
        sim = tm.create_simulation3("mpm")
        sim.initialize(dict(res=(RES,) * 3, delta_x=DX, base_delta_t=DT, max_particles=(cap or len(x)) + 64, reorder_interval=0,
                            clean_boundary=False))
        sim.set_levelset(tm.mpm.LevelSet())
        if len(x):
            sim.add_particles(dict(type="jelly", positions=_uniform(900 + r, len(x))))
            sim.upload(F_X, np.asarray(x, np.float32))
            sim.upload(F_ID, np.asarray(ids, np.int32))
        else:  # (the group table of a job is one: a rank without particles registers the group all the same)
            sim.add_particles(dict(type="jelly", positions=np.zeros((0, 3), np.float32)))
        sim._ensure_ctx()
        sims.append(sim)
    return sims


def _live(L):
    return int(L.mpmhip_debug_live_buffers())


def _msgs(sims):
    return " | ".join(s._L.mpmhip_last_error(s._ctx).decode() for s in sims)


def _one_blob(sim):
    """mpmhip_snapshot_save of one ctx: its slots as they lie, dead ones included"""
    n = int(sim._check(sim._L.mpmhip_snapshot_size(sim._ctx)))
    buf = np.empty(n, np.uint8)
    sim._check(sim._L.mpmhip_snapshot_save(sim._ctx, buf.ctypes.data_as(C.c_void_p), n))
    return buf.tobytes()


def _group_save(sims, capacity=None, fill=0xA5):
    """(rc, blob bytes or the untouched buffer, messages) of mpmhip_snapshot_size_group + mpmhip_snapshot_save_group"""
    L, K = sims[0]._L, len(sims)
    arr = (C.c_void_p * K)(*[s._ctx for s in sims])
    n, w = C.c_size_t(), C.c_size_t()
    rc = L.mpmhip_snapshot_size_group(arr, K, C.byref(n))
    if rc:
        return rc, None, _msgs(sims)
    cap = n.value if capacity is None else capacity(n.value)
    buf = np.full(max(n.value, 1), fill, np.uint8)
    rc = L.mpmhip_snapshot_save_group(arr, K, buf.ctypes.data_as(C.c_void_p), cap, C.byref(w))
    return rc, (buf[:w.value].tobytes() if rc == 0 else buf), _msgs(sims)


def _load_brick(sim, blob):
    b = np.frombuffer(blob, np.uint8)
    info = (C.c_int64 * 4)()
    rc = int(sim._L.mpmhip_snapshot_load_brick(sim._ctx, b.ctypes.data_as(C.c_void_p), b.size, info))
    return rc, [int(v) for v in info], sim._L.mpmhip_last_error(sim._ctx).decode()


def _model_job_blob(sims):
    """the model's assembly of the ranks' own records, each read from its rank's one-ctx blob"""
    blobs = [_one_blob(s) for s in sims]
    rows = [model.rows_of(b) for b in blobs]
    numbers = model.job_row_numbers([ids for ids, _ in rows])
    p0 = model.parse(blobs[0])
    head = p0["head"]
    nxt = max(int(model.head_field(model.parse(b)["head"], model.H_NEXT_PID, np.int32)) for b in blobs)
    head[model.H_NEXT_PID:model.H_NEXT_PID + 4] = np.array([nxt], np.int32).view(np.uint8)
    return model.assemble(head.tobytes(), p0["groups"], [(numbers[r], rows[r][1]) for r in range(len(sims))])


def _empty_sims(tm, count, cap, **cfg):
    """simulations that hold no particle: ctx and level set"""
    sims = []
    for _ in range(count):
        sim = tm.create_simulation3("mpm")
        sim.initialize(dict(dict(res=(RES,) * 3, delta_x=DX, base_delta_t=DT, max_particles=cap, reorder_interval=0), **cfg))
        ls = tm.mpm.LevelSet(friction=0.4)
        for p in PLANES:
            ls.add_plane(p[:3], d=p[3])
        sim.set_levelset(ls)
        sim._ensure_ctx()
        sims.append(sim)
    return sims


def _empty_job(tm, part, cap, **cfg):
    """a job of part.world ranks that hold no particle: ctx, level set, partition, data plane"""
    from taichi_mpm_amd import tiled
    sims = _empty_sims(tm, part.world, cap, **cfg)
    return tiled.NativeVirtualJob([tiled.HipEngine(sim, 0) for sim in sims], part, migrate_interval=2), sims


def _check_loaded_ranks(sims, part, blob, infos):
    """every rank's slots are exactly the records the model says it owns, in blob order; the header's clocks and next id the blob's"""
    src = model.parse(blob)
    live = int((model.ids_of(src["rg"]) >= 0).sum())
    lost = live - int(model.placeable(blob, DX).sum())
    kept = 0
    for r, sim in enumerate(sims):
        want = model.owned(blob, part, r, DX)
        got = model.parse(_one_blob(sim))
        assert infos[r] == [len(want), live, 0, lost], (r, infos[r], len(want), live, lost)
        assert int(sim._L.mpmhip_num_slots(sim._ctx)) == len(want) == sim.get_num_particles()
        for sec in ("rg", "rp", "rb"):
            assert np.array_equal(got[sec], src[sec][want]), (r, sec)
        assert got["groups"] == src["groups"]
        for off, dt in ((model.H_SUBSTEPS, np.int64), (model.H_NEXT_PID, np.int32), (model.H_T, np.float32), (model.H_REQUEST_T, np.float32),
                        (model.H_NDEAD, np.uint32)):
            want_v = 0 if off == model.H_NDEAD else model.head_field(src["head"], off, dt)
            assert model.head_field(got["head"], off, dt) == want_v, (r, off)
        kept += len(want)
    assert kept == live - lost
    return lost


# ------------------------------------------------------------------------------------------------ 1. K ctx, nothing stepped
@pytest.fixture(scope="module")
def one_ctx_blob(tm):
    """the two-material state in ONE ctx, ids in no order: its snapshot and the canonical form — computed once, shared, unchanged"""
    s = _two_material_state()
    ids = np.random.RandomState(11).permutation(s.n)
    one = _sim(tm, s, np.ones(s.n, bool), ids, s.n + 64)
    blob = _one_blob(one)
    one.close()
    return dict(s=s, ids=ids, blob=blob, canonical=model.canonical(blob))


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_k_ctx_save_the_canonical_blob_of_the_one_ctx(tm, one_ctx_blob, K):
    from taichi_mpm_amd import tiled
    s, ids = one_ctx_blob["s"], one_ctx_blob["ids"]
    assert s.n > 13000
    part = tiled.Partition.balanced((RES,) * 3, K, s.x, DX, margin=2)
    owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
    L = tm.load()
    sims = [_sim(tm, s, owner == r, ids, s.n + 64) for r in range(K)]
    before = _live(L)
    rc, got, msg = _group_save(sims)
    assert rc == 0, msg
    assert got == one_ctx_blob["canonical"]  # (the same bytes for every K: each equals the one canonical blob)
    assert _live(L) == before  # bitmap, prefix and the device image were DevBufs of the call
    for sim in sims:
        sim.close()


# ------------------------------------------------------------------------------------------------ 2. a job that has lived
def test_snapshot_of_a_job_that_stepped_recut_and_lost_particles(tm, tmp_path):
    from taichi_mpm_amd import tiled
    s = _two_material_state()
    n, world = s.n, 3
    ids = np.random.RandomState(5).permutation(n)
    part = tiled.Partition((RES,) * 3, (1, 3, 1), [[0, RES], [0, 11, 13, RES], [0, RES]], 2)
    owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
    sims = [_sim(tm, s, owner == r, ids, n + 1024) for r in range(world)]
    job = tiled.NativeVirtualJob([tiled.HipEngine(sim, 0) for sim in sims], part, migrate_interval=2)
    job.run(12)
    assert job.rebalance(force=True)["recut"]
    job.run(6)
    assert job.totals()["error"] == 0
    for sim in sims:  # everything left of x = 0.45 is inside: dead slots between live ones on every rank that reaches there
        sim.set_levelset(tm.mpm.LevelSet().add_plane((1.0, 0.0, 0.0), d=-0.45))
        sim.general_action(dict(action="delete_particles_inside_level_set"))
    held = [sim.get_particles(sort_by_id=False) for sim in sims]
    slots = [int(sim._L.mpmhip_num_slots(sim._ctx)) for sim in sims]
    assert any(sl > len(p["id"]) for sl, p in zip(slots, held)) and 0 < sum(len(p["id"]) for p in held) < n
    for p in held:
        assert len(p["id"]) > 1 and not np.all(np.diff(p["id"]) > 0)  # no rank's slots are in id order
    L = tm.load()
    before = _live(L)
    got = job.snapshot_bytes()
    assert _live(L) == before
    assert got == _model_job_blob(sims)
    # the file: one leading word, then the blob; a plain simulation loads it and holds exactly the job's particles
    job.frame_count = 7
    path = str(tmp_path / "job.snap")
    assert job.save_snapshot(path) is True
    raw = open(path, "rb").read()
    assert raw[:8] == np.array([7], np.int64).tobytes() and raw[8:] == got
    all_p = _gather(sims)
    fresh = tm.create_simulation3("mpm").initialize(dict(res=(RES,) * 3, delta_x=DX, base_delta_t=DT, max_particles=n + 64, reorder_interval=0))
    fresh.load_snapshot(path)
    assert fresh.frame == 7 and fresh.get_num_particles() == len(all_p["id"])
    assert _same_bits(fresh.get_particles(), all_p)
    fresh.close()
    for sim in sims:
        sim.close()


# ------------------------------------------------------------------------------------------------ 3. shapes of the ranking and the filter
CHUNK = 1000
PART4 = dict(dims=(2, 2, 1), cuts=[[0, 16, RES], [0, 15, RES], [0, RES]])


def _sparse(n):
    return (np.arange(n, dtype=np.int64) * 4001 % 2000003).astype(np.int32)


def _shape_cases():
    """name -> (rank positions, rank ids).  Positions lie in cells 5 .. 26."""
    rng = np.random.RandomState(7)
    sp = _sparse(500)
    own = rng.randint(0, 2, 500)
    cube = lattice_cube(RES, 5, 26, DX, jitter=0.2, seed=9)  # a 21^3-cell lattice cube: 74 k particles
    perm = rng.permutation(len(cube))
    half = len(cube) // 2 + 17

    def uni(rank_ids):
        return [_uniform(40 + r, len(i)) for r, i in enumerate(rank_ids)], rank_ids
    cases = {
        "sparse_ids_over_2_ranks": uni([rng.permutation(sp[own == 0]), rng.permutation(sp[own == 1])]),
        "a_rank_without_particles": uni([np.arange(300) * 2 + 1, [], np.arange(200) * 2]),
        "one_particle_in_the_job": uni([[], [12345]]),
        "no_particle_at_all": uni([[], []]),
        "more_than_65536_over_2_ranks": ([cube[perm[:half]], cube[perm[half:]]], [perm[:half], perm[half:]]),
        "one_rank_inside_one_word_its_neighbour_in_the_next": uni([np.arange(64, 96)[::-1], rng.permutation(np.arange(32, 64))]),
        "ids_at_the_word_edges": uni([[63, 0], [32, 31]]),
    }
    m = 32 * CHUNK  # a multiple of the chunk and of 256 (and no multiple of the 1024 records of a workgroup's span)
    for name, n in (("count_one_below_a_multiple", m - 1), ("count_at_a_multiple", m), ("count_one_above_a_multiple", m + 1)):
        p = rng.permutation(n)
        cases[name] = uni([p[:n // 3], p[n // 3:]])
    # one rank of the 2 x 2 x 1 job owns every record (cells 8 .. 14 on x and y), three end empty
    x = _uniform(61, 3000)
    x[:, :2] = ((8 + rng.rand(3000, 2) * 6.9) * DX).astype(np.float32)
    cases["one_rank_owns_all"] = ([x[:1700], x[1700:]], [rng.permutation(3000)[:1700] + 5, np.arange(1300) + 4000])
    # records exactly ON the cut planes x = 16 and y = 15 (X - 0.5 = the cut: the upper brick's), their neighbours one ulp below
    x = _uniform(62, 2400)
    x[:600, 0] = np.float32(16.5) * np.float32(DX)
    x[600:1200, 0] = np.nextafter(np.float32(16.5) * np.float32(DX), np.float32(0))
    x[1200:1800, 1] = np.float32(15.5) * np.float32(DX)
    x[1800:, 1] = np.nextafter(np.float32(15.5) * np.float32(DX), np.float32(0))
    p = rng.permutation(2400)
    cases["records_on_a_cut_plane"] = ([x[p[:1000]], x[p[1000:]]], [p[:1000], p[1000:]])
    return cases


@pytest.mark.parametrize("case", sorted(_shape_cases()) + ["one_ctx_blob_with_dead_slots"])
def test_shapes_at_which_the_ranking_and_the_filter_can_go_wrong(tm, monkeypatch, case):
    from taichi_mpm_amd import tiled
    L = tm.load()
    if case == "one_ctx_blob_with_dead_slots":
        ids = np.random.RandomState(3).permutation(5000).astype(np.int32)
        sims = _plain_sims(tm, [_uniform(63, 5000)], [ids])
        sims[0].set_levelset(tm.mpm.LevelSet().add_plane((1.0, 0.0, 0.0), d=-0.45))
        sims[0].general_action(dict(action="delete_particles_inside_level_set"))
        blob = _one_blob(sims[0])
        p = model.parse(blob)
        dead = model.ids_of(p["rg"]) < 0
        assert 500 < dead.sum() < 4500 and dead[:-1].any() and model.head_field(p["head"], model.H_NDEAD, np.uint32) == dead.sum()
        want = model.canonical(blob)
    else:
        rank_x, rank_ids = _shape_cases()[case]
        rank_ids = [np.asarray(i, np.int32) for i in rank_ids]
        sims = _plain_sims(tm, rank_x, rank_ids)
        blob = None
        want = _model_job_blob(sims)
    for x in [s.get_particles(sort_by_id=False)["x"] for s in sims]:
        assert not len(x) or (5 * DX <= x.min() and x.max() < 27 * DX)
    before = _live(L)
    rc, got, msg = _group_save(sims)
    assert rc == 0, msg
    assert _live(L) == before
    assert got == want
    if case == "no_particle_at_all":
        assert len(got) == 80 + len(model.parse(got)["groups"])
    if case == "more_than_65536_over_2_ranks":
        assert model.head_field(model.parse(got)["head"], model.H_NSLOTS, np.int64) > 65536
    n_live = int(model.head_field(model.parse(got)["head"], model.H_NSLOTS, np.int64))
    for sim in sims:
        sim.close()
    # ---- the load: the job's blob (or the one-ctx blob with its dead slots) into 2 x 2 x 1 ranks, 1000 records a chunk
    blob = blob or got
    monkeypatch.setenv("MPMHIP_SNAP_CHUNK", str(CHUNK))
    part = tiled.Partition((RES,) * 3, PART4["dims"], PART4["cuts"], 2)
    job, ranks = _empty_job(tm, part, n_live + 64, clean_boundary=False)
    before = _live(L)
    infos = []
    for sim in ranks:
        rc, info, msg = _load_brick(sim, blob)
        assert rc == 0, msg
        infos.append(info)
    assert _live(L) == before  # the staging buffer and the count words were DevBufs of the calls
    assert all(i[3] == 0 for i in infos)
    assert _check_loaded_ranks(ranks, part, blob, infos) == 0
    if case == "one_rank_owns_all":
        assert [i[0] for i in infos] == [3000, 0, 0, 0]
    if case == "records_on_a_cut_plane":
        assert all(i[0] > 0 for i in infos)
    # ... and the job that loaded it saves the same canonical blob.  (But for the header's b_stale: on a ctx that does not keep apic_b
    # a loaded record's apic_b counts as behind RecP.A, as after mpmhip_snapshot_load, while these records were never stepped.)
    rc, again, msg = _group_save(ranks)
    assert rc == 0, msg
    assert again[:model.H_B_STALE] == want[:model.H_B_STALE] and again[model.H_B_STALE + 4:] == want[model.H_B_STALE + 4:]
    for sim in ranks:
        sim.close()


def test_three_unplaceable_records_are_counted_and_nobody_keeps_them(tm, monkeypatch):
    from taichi_mpm_amd import tiled
    from taichi_mpm_amd.mpm import F_X
    x = _uniform(64, 2000)
    sims = _plain_sims(tm, [x], [np.arange(2000)])
    x[17] = (0.5, np.nan, 0.5)
    x[900] = (0.5, 0.5, np.float32(0.49) * np.float32(DX))  # below half a cell
    x[1999] = (np.inf, 0.5, 0.5)
    sims[0].upload(F_X, x)
    blob = _one_blob(sims[0])
    sims[0].close()
    monkeypatch.setenv("MPMHIP_SNAP_CHUNK", str(CHUNK))
    part = tiled.Partition((RES,) * 3, PART4["dims"], PART4["cuts"], 2)
    job, ranks = _empty_job(tm, part, 2064, clean_boundary=False)
    infos = []
    for sim in ranks:
        rc, info, msg = _load_brick(sim, blob)
        assert rc == 0, msg
        infos.append(info)
    assert all(i[3] == 3 and i[1] == 2000 for i in infos) and sum(i[0] for i in infos) == 1997
    assert _check_loaded_ranks(ranks, part, blob, infos) == 3
    with pytest.warns(UserWarning, match="3 live particles"):
        out = job.load_snapshot(np.array([0], np.int64).tobytes() + blob)
    assert out["unplaceable"] == 3 and out["total"] == 2000 and sum(out["kept"]) == 1997 and out["grew"] == []
    for sim in ranks:
        sim.close()


# ------------------------------------------------------------------------------------------------ 4. round trip across rank counts
@pytest.fixture(scope="module")
def one_ctx_after_12(tm):
    s = _two_material_state()
    one = _sim(tm, s, np.ones(s.n, bool), np.arange(s.n), s.n + 1024)
    one.run_substeps(12)
    ref = one.get_particles()
    one.close()
    return ref


def _lopsided(world):
    from taichi_mpm_amd import tiled
    dims = tiled.brick_dims(world)
    return tiled.Partition((RES,) * 3, dims, [[0, 12, RES] if d == 2 else [0, RES] for d in dims], 2)


def _save_load_run(tm, path, src_world, dst_world, **cfg):
    """a job of src_world ranks runs 6 substeps and saves; a job of dst_world ranks, cut from the file's histograms, loads it and
    runs 6 more.  -> (saved blob, loading job, its sims, what load_snapshot returned, replans before the run)"""
    from taichi_mpm_amd import tiled
    s = _two_material_state()
    n, ids = s.n, np.arange(s.n)
    part = _lopsided(src_world)
    owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
    sims = [_sim(tm, s, owner == r, ids, n + 1024, **cfg) for r in range(src_world)]
    job = tiled.NativeVirtualJob([tiled.HipEngine(sim, 0) for sim in sims], part, migrate_interval=2)
    job.run(6)
    job.frame_count = 3
    assert job.save_snapshot(path)
    saved = job.snapshot_bytes()
    assert open(path, "rb").read()[8:] == saved
    for sim in sims:
        sim.close()
    # the restart recipe: histograms of the file -> bricks -> rank simulations without particles -> the job -> load
    ranks = [_sim(tm, s, np.zeros(n, bool), ids, n + 1024, **cfg) for _ in range(dst_world)]
    hists, lo, hi, total = tiled.snapshot_histograms(ranks[0], path)
    assert total == n and ranks[0].get_num_particles() == 0
    new = tiled.Partition.from_histograms((RES,) * 3, dst_world, hists, lo, hi, 2)
    job2 = tiled.NativeVirtualJob([tiled.HipEngine(sim, 0) for sim in ranks], new, migrate_interval=2)
    out = job2.load_snapshot(path)
    return saved, job2, ranks, out, hists


def test_round_trip_from_8_ranks_to_3(tm, tmp_path, one_ctx_after_12):
    from taichi_mpm_amd import tiled
    saved, job, ranks, out, hists = _save_load_run(tm, str(tmp_path / "job.snap"), 8, 3)
    n = len(one_ctx_after_12["id"])
    assert out["total"] == n == sum(out["kept"]) and out["unplaceable"] == 0 and out["grew"] == [] and all(k > 0 for k in out["kept"])
    assert max(out["kept"]) < 0.5 * n  # the bricks were cut from the file's own histograms
    assert job.frame_count == 3
    assert job.snapshot_bytes() == saved  # (before anything downloads apic_b: a ctx that does not keep it rebuilds it for the download)
    b = tiled.base_cells(_gather(ranks)["x"], DX)
    for a in range(3):
        assert np.array_equal(hists[a], np.bincount(b[:, a], minlength=RES))
    before = job.state()
    assert all(t["substeps"] == 0 and t["replans"] == 0 for t in before)
    job.run(6)  # (begins with the planning scan: the plan went stale with the load)
    assert job.totals()["error"] == 0
    assert all(t["replans"] >= 1 and t["substeps"] == 6 for t in job.state()), job.state()
    _against_one_ctx(_gather(ranks), one_ctx_after_12)
    for sim in ranks:
        sim.close()


# ------------------------------------------------------------------------------------------------ 5. capacity and refusals
def test_a_rank_too_small_is_refused_untouched_and_grown_by_the_job(tm, one_ctx_blob):
    from taichi_mpm_amd import tiled
    blob, s = one_ctx_blob["canonical"], one_ctx_blob["s"]
    part = tiled.Partition.balanced((RES,) * 3, 2, s.x, DX, margin=2)
    want = [model.owned(blob, part, r, DX) for r in range(2)]
    assert min(len(w) for w in want) > 5000
    small = _plain_sims(tm, [_uniform(65, 50)], [np.arange(50) + 7], cap=936)[0]  # rank 0: 50 particles of its own, room for 1000
    ranks = [small] + _empty_sims(tm, 1, s.n + 64)
    job = tiled.NativeVirtualJob([tiled.HipEngine(sim, 0) for sim in ranks], part, migrate_interval=2)
    cap = int(small._L.mpmhip_capacity(small._ctx))
    assert cap < len(want[0])
    was = _one_blob(small)
    rc, info, msg = _load_brick(small, blob)
    assert rc == ECAPACITY and "capacity" in msg and info == [0, s.n, len(want[0]), 0], (rc, info, msg)
    assert _one_blob(small) == was and int(small._L.mpmhip_capacity(small._ctx)) == cap  # particles, groups and clocks as before
    out = job.load_snapshot(np.array([4], np.int64).tobytes() + blob)
    assert out["grew"] == [0] and out["kept"] == [len(w) for w in want] and out["total"] == s.n and job.frame_count == 4
    assert int(small._L.mpmhip_capacity(small._ctx)) >= len(want[0]) + len(want[0]) // 8
    _check_loaded_ranks(ranks, part, blob, [[len(w), s.n, 0, 0] for w in want])
    for sim in ranks:
        sim.close()


def test_refusals_leave_the_ctx_and_the_destination_alone(tm, one_ctx_blob):
    from taichi_mpm_amd import tiled
    blob = one_ctx_blob["canonical"]
    part = tiled.Partition((RES,) * 3, (2, 1, 1), [[0, 16, RES], [0, RES], [0, RES]], 2)
    sims = _plain_sims(tm, [_uniform(66, 300), _uniform(67, 200)], [np.arange(300), np.arange(300, 500)], cap=20000)
    L = tm.load()
    # a ctx without a partition
    was = _one_blob(sims[0])
    rc, info, msg = _load_brick(sims[0], blob)
    assert rc == EINVAL and "no partition" in msg and info == [0, 0, 0, 0] and _one_blob(sims[0]) == was
    for r, sim in enumerate(sims):
        tiled.set_partition(sim, part, r)
    # a blob of another res, dx, dt; a truncated blob
    b = bytearray(blob)
    for off, value, what in ((model.H_RES + 8, np.array([2 * RES], np.int32), "grid"), (model.H_DX, np.array([DX / 2], np.float32), "delta_x"),
                             (model.H_DT, np.array([2 * DT], np.float32), "base_delta_t")):
        bad = bytearray(b)
        bad[off:off + 4] = value.tobytes()
        rc, info, msg = _load_brick(sims[0], bytes(bad))
        assert rc == EINVAL and what in msg and _one_blob(sims[0]) == was, (what, rc, msg)
    for cut in (len(blob) - 1, 80 + 40, 79, 3):
        rc, info, msg = _load_brick(sims[0], blob[:cut])
        assert rc == EINVAL and "truncated" in msg and _one_blob(sims[0]) == was, (cut, rc, msg)
    # a blob with a rigid tail (a 16^3 scene: the ctx is of that grid)
    rigid = np.fromfile(os.path.join(GOLDEN, "snapshot_rigid3d_in.bin"), np.uint8)[8:].tobytes()
    sim16 = tm.create_simulation3("mpm").initialize(dict(res=(16,) * 3, delta_x=1.0 / 16, base_delta_t=1e-4, max_particles=4096))
    sim16._ensure_ctx()
    tiled.set_partition(sim16, tiled.Partition((16,) * 3, (1, 1, 1), [[0, 16]] * 3, 2), 0)
    rc, info, msg = _load_brick(sim16, rigid)
    assert rc == EINVAL and "rigid" in msg and sim16.get_num_particles() == 0, (rc, msg)
    hist = np.zeros(16, np.int64)
    lp = C.POINTER(C.c_int64)
    rb = np.frombuffer(rigid, np.uint8)
    assert L.mpmhip_snapshot_histogram(sim16._ctx, rb.ctypes.data_as(C.c_void_p), rb.size, hist.ctypes.data_as(lp), None, None, None, None, None) == EINVAL
    sim16.close()
    # saving: a short dst; a rank whose group table differs
    rc, buf, msg = _group_save(sims, capacity=lambda n: n - 1)
    assert rc == ECAPACITY and "too small" in msg and (buf == 0xA5).all()
    rc, good, msg = _group_save(sims)
    assert rc == 0 and good == _model_job_blob(sims)
    sims[1].add_particles(dict(type="sand", positions=np.zeros((0, 3), np.float32)))  # a second group on rank 1 alone
    sims[1]._ensure_ctx()
    rc, buf, msg = _group_save(sims)
    assert rc == EINVAL and "group table of rank 1" in msg and (buf == 0xA5).all(), (rc, msg)
    for sim in sims:
        sim.close()


# ------------------------------------------------------------------------------------------------ 6. deterministic mode
def test_deterministic_mode_two_runs_of_save_load_run_end_byte_identical(tm, tmp_path):
    runs = []
    for k in range(2):
        saved, job, ranks, out, _ = _save_load_run(tm, str(tmp_path / ("job%d.snap" % k)), 4, 3, deterministic=True)
        job.run(6)
        assert job.totals()["error"] == 0
        runs.append((saved, _gather(ranks)))
        for sim in ranks:
            sim.close()
    assert runs[0][0] == runs[1][0]
    assert _same_bits(runs[0][1], runs[1][1])


# ------------------------------------------------------------------------------------------------ 7. two processes over the IPC wire
def _ipc_worker(rank, world, port, device, q, path):
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
        job.synchronize()
        before = int(sim._L.mpmhip_debug_live_buffers())
        wrote = job.save_snapshot(path)
        leaked = int(sim._L.mpmhip_debug_live_buffers()) - before
        mine = _one_blob(sim)
        dist.barrier()  # (rank 0 has written the file)
        out = job.load_snapshot(path)
        job.run(2)
        err = job.totals()["error"]
        dist.barrier()  # nobody unmaps an arena a peer may still write to
        q.put((rank, wrote, leaked, mine, out, err, sim.get_num_particles()))
        sim.close()
    finally:
        dist.destroy_process_group()


def test_two_processes_over_the_ipc_wire_write_one_file_and_load_it(tm, tmp_path):
    import socket

    import torch.multiprocessing as mp
    world = 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    path = str(tmp_path / "job.snap")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_ipc_worker, args=(r, world, port, 0, q, path)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert [r[1] for r in res] == [True, False] and [r[2] for r in res] == [0, 0]  # rank 0 wrote, rank 1 did not; nothing is left allocated
    assert os.listdir(str(tmp_path)) == ["job.snap"]
    blobs = [r[3] for r in res]
    rows = [model.rows_of(b) for b in blobs]
    assert all(len(ids) > 0 for ids, _ in rows) and sum(len(ids) for ids, _ in rows) > 13000
    numbers = model.job_row_numbers([ids for ids, _ in rows])
    p0 = model.parse(blobs[0])
    head = p0["head"]
    nxt = max(int(model.head_field(model.parse(b)["head"], model.H_NEXT_PID, np.int32)) for b in blobs)
    head[model.H_NEXT_PID:model.H_NEXT_PID + 4] = np.array([nxt], np.int32).view(np.uint8)
    want = model.assemble(head.tobytes(), p0["groups"], [(numbers[r], rows[r][1]) for r in range(world)])
    raw = open(path, "rb").read()
    assert raw[:8] == np.array([0], np.int64).tobytes() and raw[8:] == want
    n = sum(len(ids) for ids, _ in rows)
    assert all(r[4]["total"] == n and sum(r[4]["kept"]) == n and r[4]["unplaceable"] == 0 for r in res)
    assert res[0][4]["kept"] == res[1][4]["kept"] and all(k > 0 for k in res[0][4]["kept"])  # every rank reports the job's counts
    assert [r[5] for r in res] == [0, 0] and sum(r[6] for r in res) == n
