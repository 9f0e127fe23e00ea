"""GPU tests of the frame of a tiled job (include/mpmhip.h: "the frame of a tiled job"): ONE .bgeo file of all ranks' particles in
ascending creation id, the ids ranked on the device (csrc/k_frame.h) — mpmhip_bgeo_encode_group on K ctx against the file of the one
ctx that holds the same records, a job that has stepped, re-cut and lost particles, the shapes at which the ranking can go wrong,
the refusals, a seeded job, visualize(), and two processes over the IPC wire.  Grid 32^3, dx = 1/32; the scenes and helpers are those
of tests/test_gpu_recut.py, copied."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import bgeo as obgeo
from tests import bgeo_reader
from tests.common import lattice_cube, make_state

pytestmark = pytest.mark.gpu

RES, DX, DT = 32, 1.0 / 32, 1e-4
PLANES = [(0.0, 1.0, 0.0, -0.3)]
FIELDS = ("x", "v", "F", "B", "aux", "gid", "id")
EINVAL, ECAPACITY = -1, -4


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


def _group(sims, verbose, capacity=None, fill=0xA5):
    """(rc, image bytes or the untouched buffer, message on ctx 0) of mpmhip_bgeo_size_group + mpmhip_bgeo_encode_group"""
    L, K = sims[0]._L, len(sims)
    arr = (C.c_void_p * K)(*[s._ctx for s in sims])
    n, w = C.c_size_t(), C.c_size_t()
    rc = L.mpmhip_bgeo_size_group(arr, K, int(verbose), C.byref(n))
    if rc:
        return rc, None, " | ".join(L.mpmhip_last_error(s._ctx).decode() for s in sims)
    cap = n.value if capacity is None else capacity(n.value)
    buf = np.full(max(n.value, 1), fill, np.uint8)
    rc = L.mpmhip_bgeo_encode_group(arr, K, int(verbose), buf.ctypes.data_as(C.c_void_p), cap, C.byref(w))
    msgs = " | ".join(L.mpmhip_last_error(s._ctx).decode() for s in sims)
    return rc, (buf[:w.value].tobytes() if rc == 0 else buf), msgs


def _live(L):
    return int(L.mpmhip_debug_live_buffers())


def _oracle_plain(p):
    return obgeo.encode(p["x"], p["v"], p["id"], False)


def _plain_sims(tm, rank_x, rank_ids, cap=None):
    """one ctx per rank holding jelly particles at rank_x[r] with the creation ids rank_ids[r].  add_particles ignores positions
    within 7 cells of the grid's faces, as the reference does: the particles are created inside and the positions uploaded
    (clean_boundary off: such particles are legal; nothing here steps)"""
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
        sim._ensure_ctx()
        sims.append(sim)
    return sims


def _uniform(seed, n):
    rng = np.random.RandomState(seed)
    return ((8 + rng.rand(n, 3) * 16) * DX).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. K ctx, nothing stepped
@pytest.fixture(scope="module")
def one_ctx_files(tm):
    """the two-material state in ONE ctx: its plain and verbose files — computed once, shared, left unchanged"""
    s = _two_material_state()
    one = _sim(tm, s, np.ones(s.n, bool), np.arange(s.n), s.n + 64)
    out = dict(s=s, plain=one.bgeo_bytes(False), verbose=one.bgeo_bytes(True))
    one.close()
    return out


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_k_ctx_encode_the_file_of_the_one_ctx(tm, one_ctx_files, K):
    """~14 k particles dealt to K ctx by brick, ids uploaded: the records are the same bits, so must the files be"""
    from taichi_mpm_amd import tiled
    s = one_ctx_files["s"]
    assert s.n > 13000
    part = tiled.Partition.balanced((RES,) * 3, K, s.x, DX, margin=2)
    owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
    L = tm.load()
    sims = [_sim(tm, s, owner == r, np.arange(s.n), s.n + 64) for r in range(K)]
    before = _live(L)
    for verbose in (False, True):
        rc, got, msg = _group(sims, verbose)
        assert rc == 0, msg
        assert got == one_ctx_files["verbose" if verbose else "plain"]
    assert _live(L) == before  # bitmap, prefix and rows were DevBufs of the calls
    for sim in sims:
        sim.close()


# ------------------------------------------------------------------------------------------------ 2. a job that has lived
def test_frame_of_a_job_that_stepped_recut_and_lost_particles(tm):
    from taichi_mpm_amd import tiled
    s = _two_material_state()
    n, world = s.n, 3
    ids = np.random.RandomState(5).permutation(n)  # (uploaded ids in no order at all: no rank's slots can be in id order)
    # three bricks along y, cut well off the particles' centre (cells 9 .. 21): the re-cut has something to move, and the plane
    # x = 0.45 below takes particles from every rank
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
        assert len(p["id"]) > 1 and not np.all(np.diff(p["id"]) > 0)  # no rank's slots are in id order: the ordering work is real
    L = tm.load()
    before = _live(L)
    all_p = _gather(sims)
    assert job.bgeo_bytes(False) == _oracle_plain(all_p)
    # verbose: every row is the row the one-ctx encoder writes for that particle on its own rank
    got = job.bgeo_bytes(True)
    assert _live(L) == before
    width = 4 * 23
    rows, rid = [], []
    for sim in sims:
        img = sim.bgeo_bytes(True)
        d = bgeo_reader.parse(img)
        head, _ = tiled.frame_envelope(d["n"], 1)
        rows.append(np.frombuffer(img, np.uint8)[len(head):len(head) + d["n"] * width].reshape(d["n"], width))
        rid.append(d["data"]["index"].ravel().astype(np.int64))
    rows, rid = np.concatenate(rows), np.concatenate(rid)
    order = np.argsort(rid, kind="stable")
    assert np.array_equal(rid[order], all_p["id"])
    head, tail = tiled.frame_envelope(len(rid), 1)
    assert got == head + rows[order].tobytes() + tail
    for sim in sims:
        sim.close()


# ------------------------------------------------------------------------------------------------ 3. shapes of the ranking
def _sparse(n):
    return (np.arange(n, dtype=np.int64) * 4001 % 2000003).astype(np.int32)  # the set of test_bgeo_sparse_ids_take_the_sort_path


def _shape_cases():
    rng = np.random.RandomState(7)
    sp = _sparse(500)
    own = rng.randint(0, 2, 500)
    cube = lattice_cube(RES, 5, 26, DX, jitter=0.2, seed=9)  # a 21^3-cell lattice cube: 74 k particles
    perm = rng.permutation(len(cube))
    half = len(cube) // 2 + 17
    return {
        "sparse_ids_over_2_ranks": (None, [rng.permutation(sp[own == 0]), rng.permutation(sp[own == 1])]),
        "a_rank_without_particles": (None, [np.arange(300) * 2 + 1, [], np.arange(200) * 2]),
        "one_particle_in_the_job": (None, [[], [12345]]),
        "no_particle_at_all": (None, [[], []]),
        "more_than_65536_over_2_ranks": (cube, [perm[:half], perm[half:]]),
        "one_rank_inside_one_word_its_neighbour_in_the_next": (None, [np.arange(64, 96)[::-1], rng.permutation(np.arange(32, 64))]),
        "ids_at_the_word_edges": (None, [[63, 0], [32, 31]]),
    }


@pytest.mark.parametrize("case", sorted(_shape_cases()))
def test_shapes_at_which_the_ranking_can_go_wrong(tm, case):
    positions, rank_ids = _shape_cases()[case]
    rank_ids = [np.asarray(i, np.int32) for i in rank_ids]
    if positions is not None:  # the ids index them
        rank_x = [positions[i] for i in rank_ids]
        assert sum(len(i) for i in rank_ids) > 65536
    else:
        rank_x = [_uniform(40 + r, len(i)) for r, i in enumerate(rank_ids)]
    sims = _plain_sims(tm, rank_x, rank_ids)
    L = tm.load()
    before = _live(L)
    rc, got, msg = _group(sims, False)
    assert rc == 0, msg
    assert _live(L) == before
    want = _oracle_plain(_gather(sims))
    assert got == want
    if case == "no_particle_at_all":
        assert got == sims[0].bgeo_bytes(False)  # the empty one-ctx file
    for sim in sims:
        sim.close()


# ------------------------------------------------------------------------------------------------ 4. errors
def test_an_id_held_twice_a_short_buffer_and_a_rigid_ctx_are_refused(tm):
    from tests import cpic_scenes as cs
    L = tm.load()
    sims = _plain_sims(tm, [_uniform(1, 100), _uniform(2, 50)], [np.arange(100), np.arange(100, 150)])
    before = _live(L)
    rc, buf, msg = _group(sims, False, capacity=lambda n: n - 1)  # one byte short
    assert rc == ECAPACITY and "bgeo image needs" in msg and (buf == 0xA5).all()
    rc, got, msg = _group(sims, False)
    assert rc == 0 and got == _oracle_plain(_gather(sims))
    ids1 = np.arange(100, 150).astype(np.int32)
    ids1[7] = 42  # rank 0 holds 42
    sims[1].upload(tm.mpm.F_ID, ids1)
    rc, buf, msg = _group(sims, False)
    assert rc == EINVAL and "creation id 42 " in msg and "twice" in msg
    assert (buf == 0xA5).all()  # the destination is untouched
    assert _live(L) == before
    for sim in sims:
        sim.close()
    # a ctx with a rigid body in the group
    sims = _plain_sims(tm, [_uniform(3, 100)], [np.arange(100)])
    rigid = tm.create_simulation3("mpm").initialize(dict(res=(RES,) * 3, delta_x=DX, base_delta_t=DT, max_particles=4096))
    rigid.add_particles(dict(type="rigid", mesh=cs.plate(), codimensional=True, initial_position=(0.5, 0.5, 0.5)))
    rigid.add_particles(dict(type="jelly", positions=_uniform(4, 64)))
    rigid._ensure_ctx()
    rc, _, msg = _group(sims + [rigid], False)
    assert rc == EINVAL and "rigid" in msg
    other = tm.create_simulation3("mpm").initialize(dict(res=(RES, RES, 2 * RES), delta_x=DX, base_delta_t=DT, max_particles=4096))
    other._ensure_ctx()
    rc, _, msg = _group(sims + [other], False)
    assert rc == EINVAL and "res" in msg
    for sim in sims + [rigid, other]:
        sim.close()


# ------------------------------------------------------------------------------------------------ 5. a seeded job
def test_seeded_job_writes_the_file_of_the_seeded_one_ctx(tm):
    from taichi_mpm_amd import tiled
    SIM = dict(res=(RES,) * 3, delta_x=DX, base_delta_t=DT)
    cfg = dict(type="sand", ppc=8.0, region=tm.mpm.LevelSet().add_sphere((0.5, 0.5, 0.5), 6 * DX))
    one = tm.create_simulation3("mpm").initialize(dict(SIM))
    hists, lo, hi, total = tiled.seed_histograms(one, cfg)
    one.add_particles(cfg)
    want = one.bgeo_bytes()
    assert one.get_num_particles() == total > 4000
    one.close()
    part = tiled.Partition.from_histograms((RES,) * 3, 4, hists, lo, hi, 2)
    sims = tiled.build_seeded_rank_sims(tm, [cfg], part, **SIM)
    assert all(s.seed_counts[0] > 0 for s in sims)
    job = tiled.NativeVirtualJob([tiled.HipEngine(s, 0) for s in sims], part, migrate_interval=2)
    assert job.bgeo_bytes() == want  # the ids are job-wide by construction
    for s in sims:
        s.close()


# ------------------------------------------------------------------------------------------------ 6. visualize()
def test_visualize_writes_numbered_frames_of_the_job(tm, tmp_path):
    from taichi_mpm_amd import tiled
    s = _two_material_state()
    part = tiled.Partition.balanced((RES,) * 3, 2, s.x, DX, margin=2)
    owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
    frames = str(tmp_path / "frames")
    sims = [_sim(tm, s, owner == r, np.arange(s.n), s.n + 1024, frame_directory=frames, verbose_bgeo=True) for r in range(2)]
    job = tiled.NativeVirtualJob([tiled.HipEngine(sim, 0) for sim in sims], part, migrate_interval=2)
    assert job.frame_directory == frames and job.verbose_bgeo is True and job.frame_count == 0
    job.run(2)
    f1 = job.visualize()
    job.run(2)
    f2 = job.visualize()
    assert [os.path.basename(f1), os.path.basename(f2)] == ["0001.bgeo", "0002.bgeo"] and job.frame_count == 2
    assert sorted(os.listdir(frames)) == ["0001.bgeo", "0002.bgeo"]
    assert open(f2, "rb").read() == job.bgeo_bytes() == job.bgeo_bytes(True) != open(f1, "rb").read()
    d = bgeo_reader.parse(open(f2, "rb").read())
    assert d["n"] == s.n and np.array_equal(d["data"]["index"].ravel(), np.arange(s.n))
    job.frame_directory = None
    with pytest.raises(tm.mpm.MPMError, match="frame_directory"):
        job.visualize()
    for sim in sims:
        sim.close()


# ------------------------------------------------------------------------------------------------ the three steps of a rank per process
def test_the_three_collective_free_steps_on_one_ctx_and_their_refusals(tm):
    """mpmhip_live_id_top -> mpmhip_id_bitmap -> mpmhip_bgeo_rows_ranked in this process: two ctx play two ranks, numpy plays the
    control group (top = max, the bitmaps or-ed), tiled.assemble_frame places the rows; then what the calls refuse"""
    from taichi_mpm_amd import tiled
    from tests import frame_rank_model as model
    L = tm.load()
    rng = np.random.RandomState(3)
    ids = rng.permutation(np.arange(700) * 3)
    rank_ids = [ids[:300], ids[300:]]
    sims = _plain_sims(tm, [_uniform(70 + r, len(i)) for r, i in enumerate(rank_ids)], rank_ids)
    before = _live(L)
    tops = [int(L.mpmhip_live_id_top(s._ctx)) for s in sims]
    assert tops == [model.live_id_top(i) for i in rank_ids]
    top = max(tops)
    words, lives = [], []
    for s in sims:
        w, n = np.zeros((top + 31) // 32, np.uint32), C.c_int64()
        assert L.mpmhip_id_bitmap(s._ctx, top, w.ctypes.data_as(C.c_void_p), C.byref(n)) == 0
        words.append(w)
        lives.append(int(n.value))
    assert lives == [300, 400] and all(np.array_equal(w, model.bitmap(i, top)[0]) for w, i in zip(words, rank_ids))
    union = words[0] | words[1]

    def rows_of(s, n, verbose, bitmap=union, cap=None):
        width = 4 * (23 if verbose else 12)
        rows, idx, wr = np.full((n, width), 0xA5, np.uint8), np.full(n, 0xA5A5A5A5, np.uint32), C.c_int64(-1)
        rc = L.mpmhip_bgeo_rows_ranked(s._ctx, int(verbose), top, bitmap.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p),
                                       idx.ctypes.data_as(C.c_void_p), n if cap is None else cap, C.byref(wr))
        return rc, rows, idx, int(wr.value)
    for verbose in (False, True):
        parts = []
        for s, n, i in zip(sims, lives, rank_ids):
            rc, rows, idx, wr = rows_of(s, n, verbose)
            assert rc == 0 and wr == n
            assert np.array_equal(np.sort(idx), np.sort(model.job_rows(rank_ids)[len(parts)])) and np.all(np.diff(idx.astype(np.int64)) > 0)
            parts.append((idx, rows))
        head, tail = tiled.frame_envelope(700, verbose)
        rc, want, msg = _group(sims, verbose)
        assert rc == 0, msg
        assert tiled.assemble_frame(head, tail, parts, 4 * (23 if verbose else 12)) == want
    # refusals
    rc, rows, idx, wr = rows_of(sims[0], 300, False, cap=299)
    assert rc == ECAPACITY and (rows == 0xA5).all()
    rc, rows, idx, wr = rows_of(sims[0], 300, False, bitmap=words[1])  # a job bitmap that lacks this rank's ids
    assert rc == EINVAL and "missing from the job's bitmap" in L.mpmhip_last_error(sims[0]._ctx).decode() and (rows == 0xA5).all()
    w, n = np.zeros((top + 31) // 32, np.uint32), C.c_int64()
    assert L.mpmhip_id_bitmap(sims[1]._ctx, tops[0] - 40 if tops[0] < tops[1] else tops[1] - 40, w.ctypes.data_as(C.c_void_p), C.byref(n)) == EINVAL
    assert "top = " in L.mpmhip_last_error(sims[1]._ctx).decode()
    twice = np.asarray(rank_ids[0], np.int32).copy()
    twice[5] = twice[9]
    sims[0].upload(tm.mpm.F_ID, twice)
    assert L.mpmhip_id_bitmap(sims[0]._ctx, top, w.ctypes.data_as(C.c_void_p), C.byref(n)) == EINVAL
    assert "creation id %d is held twice" % twice[9] in L.mpmhip_last_error(sims[0]._ctx).decode()
    assert _live(L) == before
    for s in sims:
        s.close()


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
        part = tiled.Partition((RES,) * 3, tiled.brick_dims(world), [[0, 12, RES] if d == 2 else [0, RES] for d in tiled.brick_dims(world)], 2)
        owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
        sim = _sim(tm, s, owner == rank, np.arange(s.n), s.n + 1024, device=device)
        job = tiled.NativeTiledJob(tiled.HipEngine(sim, device), part, rank, world, wire="ipc", dist=dist, migrate_interval=2, overlap=False)
        job.run(6)
        job.synchronize()
        before = int(sim._L.mpmhip_debug_live_buffers())
        wrote = job.write_partio(path)
        leaked = int(sim._L.mpmhip_debug_live_buffers()) - before
        dist.barrier()  # nobody unmaps an arena a peer may still write to
        p = sim.get_particles(sort_by_id=False)
        q.put((rank, wrote, leaked, {k: p[k] for k in ("x", "v", "id")}))
        sim.close()
    finally:
        dist.destroy_process_group()


def test_two_processes_over_the_ipc_wire_write_one_file(tm, tmp_path):
    import socket

    import torch.multiprocessing as mp
    world = 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    path = str(tmp_path / "job.bgeo")
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
    assert os.listdir(str(tmp_path)) == ["job.bgeo"]
    got = {k: np.concatenate([r[3][k] for r in res]) for k in ("x", "v", "id")}
    assert all(len(r[3]["id"]) > 0 for r in res) and len(got["id"]) > 13000
    order = np.argsort(got["id"], kind="stable")
    assert open(path, "rb").read() == _oracle_plain({k: v[order] for k, v in got.items()})
