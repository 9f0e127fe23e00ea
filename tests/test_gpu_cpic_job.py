"""CPIC rigid bodies on a tiled job (include/mpmhip.h: "Bodies on a job"): every rank holds all bodies, the ranks' impulse rows are
summed in rank order twice a substep.  The yardstick is the ONE-ctx run of the same scene, which tests/test_gpu_cpic.py holds against
the reference; a job is compared with another run of the job only where bit-equality is the claim.

Scenes: tests/cpic_scenes.py at RES = 32 (block_of_particles: 3 456 particles in cells 10..22, DT = 1e-4), at most 12 substeps,
migrate_interval = 2, so the migration check runs every other substep.  Cuts at cell 16: the free box of the two-body scene spans
cells 12.8 - 19.2 in x around it.  The scene's own velocities (0.3 m/s) carry no record across a cut in 12 substeps — measured: 0
migrated on 2 and on 8 ranks —, so test_coloured_records_that_cross_a_cut_keep_their_colour adds a drift that does.

Tolerances: the project's own for CPIC substeps (docstring of tests/test_gpu_cpic.py) — ids and gids equal, x abs 5e-6, v rel-L2
2e-4, F 1e-4, colour words differing in at most 5 particles, body pose atol 2e-6, body velocities 2e-4 of max(|.|, 1e-2)."""
import numpy as np
import pytest

from tests import cpic_scenes as cs

pytestmark = pytest.mark.gpu
N_SUB = 12
FIELDS = ("x", "v", "F", "B", "aux", "gid", "id", "states")


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


# ------------------------------------------------------------------------------------------------ scenes
def _scripted_plate():
    f32, s, p0 = np.float32, cs.SCRIPT, (0.58, 0.56, 0.55)
    return dict(type="rigid", mesh=cs.plate(0.12), codimensional=True, friction=0.4,
                scripted_position=lambda t: [f32(p0[k]) + f32(s["vel"][k]) * f32(t) + f32(s["amp"][k]) * f32(np.sin(f32(s["omega"]) * f32(t))) for k in range(3)],
                scripted_rotation=lambda t: [f32(s["e0"][k]) + f32(s["rate"][k]) * f32(t) for k in range(3)])


def two_bodies():
    """the scene of test_two_bodies_at_once_match_the_live_reference: a free box (body 1) and a scripted plate (body 2) in sand"""
    x, v = cs.block_of_particles()
    box = dict(cs.BODIES["box"], type="rigid", initial_position=(0.42, 0.47, 0.46))
    return dict(bodies=[box, _scripted_plate()], material="sand", x=x, v=v, cfg=dict(res=(cs.RES,) * 3, penalty=1e3), res=cs.RES, planes=None,
                joints=[])


def two_bodies_with_a_joint():
    return dict(two_bodies(), joints=[dict(type="rotation", obj0=1, obj1=2)])


def falls_alone():
    """the scene of test_a_body_that_touches_nothing_just_falls"""
    x = (np.stack(np.meshgrid(*[np.arange(20, 26) + 0.5] * 3, indexing="ij"), -1).reshape(-1, 3) / 64).astype(np.float32)
    body = dict(type="rigid", mesh=cs.box(), codimensional=False, initial_position=(0.5, 0.7, 0.5), initial_angular_velocity=(0.0, 3.0, 0.0))
    return dict(bodies=[body], material="jelly", x=x, v=np.zeros_like(x), cfg=dict(res=(64,) * 3, delta_x=1 / 64), res=64,
                planes=None, joints=[], default_gravity=True)


def box_on_levelset():
    """the scene of test_rigid_body_levelset_collision_matches_the_live_reference with friction, restitution = 0.4, 0.5"""
    x, v = cs.block_of_particles(lo=12, hi=18)
    x = x + np.float32([0.0, 0.20, 0.0])
    body = dict(type="rigid", mesh=cs.box(), codimensional=False, density=300.0, friction=0.4, restitution=0.5, initial_position=(0.5, 0.47, 0.5),
                initial_rotation=(12.0, 20.0, 31.0), initial_velocity=(0.6, -1.5, 0.3), initial_angular_velocity=(2.0, -1.0, 3.0))
    return dict(bodies=[body], material="jelly", x=x, v=v, cfg=dict(res=(cs.RES,) * 3, rigid_body_levelset_collision=True), res=cs.RES,
                planes=[((0, 1, 0), -0.3), ((-1, 0, 0), 0.66)], joints=[])


def next_id(sim):
    return sim._check(sim._L.mpmhip_set_next_id(sim._ctx, 0))  # (never lowers the counter: 0 reads it)


def build(tm, scene, sel=None, extra=0, **more):
    """one ctx of the scene holding the particles `sel` (all of them: the one-ctx run); the bodies first, so that every ctx numbers
    their boundary particles alike and the material particles' ids begin at the same number"""
    from oracle import oracle as orc
    from taichi_mpm_amd.mpm import F_ID
    x, v = scene["x"], scene["v"]
    sel = np.ones(len(x), bool) if sel is None else sel
    cfg = dict(dict(delta_x=cs.DX, base_delta_t=cs.DT, gravity=(0, -10, 0), max_particles=len(x) + 64 + extra, reorder_interval=0), **scene["cfg"])
    if scene.get("default_gravity"):  # (the scene of test_a_body_that_touches_nothing_just_falls sets none)
        cfg.pop("gravity")
    cfg.update(more)
    sim = tm.create_simulation3("mpm").initialize(cfg)
    if scene["planes"]:
        ls = tm.mpm.LevelSet(friction=0.3)
        for n, d in scene["planes"]:
            ls.add_plane(n, d=d)
        sim.set_levelset(ls)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (two bodies without rigid_body_collision: the scene's own)
        rids = [int(sim.add_particles(dict(b))) for b in scene["bodies"]]
    for j in scene["joints"]:
        sim.add_articulation(dict(j))
    base = next_id(sim)
    gp = orc.group_params(scene["material"], cs.MASS, cs.VOL)[0]
    sim.add_particles(dict(type=scene["material"], positions=x[sel], velocities=v[sel], params=gp))
    if sel.any():
        sim.upload(F_ID, (base + np.flatnonzero(sel)).astype(np.int32))
    else:
        sim._ensure_ctx()
    return sim, rids


def partition(tiled, res, world):
    dims = {2: (2, 1, 1), 8: (2, 2, 2)}[world]
    return tiled.Partition((res,) * 3, dims, [[0, res // 2, res] if d == 2 else [0, res] for d in dims], 2)


def build_job(tm, scene, world, halo_by_rccl=False, **more):
    from taichi_mpm_amd import tiled
    part = partition(tiled, scene["res"], world)
    owner = part.rank_of_cells(tiled.base_cells(scene["x"], 1.0 / scene["res"]))
    sims = [build(tm, scene, owner == r, **more)[0] for r in range(world)]
    job = tiled.NativeVirtualJob([tiled.HipEngine(sim, 0) for sim in sims], part, migrate_interval=2, halo_by_rccl=halo_by_rccl)
    return job, sims


def gather(sims):
    parts = [sim.get_particles(sort_by_id=False) for sim in sims]
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    order = np.argsort(out["id"], kind="stable")
    return {k: v[order] for k, v in out.items()}


def body_vectors(get, rids):
    return [cs.rigid_vector(get(rid)) for rid in rids]


def run_one(tm, scene, n=N_SUB, **more):
    sim, rids = build(tm, scene, **more)
    sim.run_substeps(n)
    out = dict(p=sim.get_particles(sort_by_id=True), bodies=body_vectors(sim.get_rigid_state, rids), rids=rids)
    sim.close()
    return out


def run_job(tm, scene, world, n=N_SUB, halo_by_rccl=False, **more):
    job, sims = build_job(tm, scene, world, halo_by_rccl, **more)
    job.run(n)
    assert job.totals()["error"] == 0
    rids = list(range(1, len(scene["bodies"]) + 1))
    out = dict(p=gather(sims), bodies=body_vectors(job.get_rigid_state, rids), digests=job.rigid_digests(),
               rank_states=[sim.get_particles(sort_by_id=False)["states"].astype(np.uint32) for sim in sims],
               rank_bodies=[body_vectors(sim.get_rigid_state, rids) for sim in sims], migrated=job.totals()["migrated"])
    for sim in sims:
        sim.close()
    return out


def against_one_ctx(got, one):
    """the tolerances of the module docstring"""
    h, r = got["p"], one["p"]
    assert np.array_equal(h["id"], r["id"]) and np.array_equal(h["gid"], r["gid"])
    print("x %.3g  v %.3g  F %.3g  colours %d" % (np.abs(h["x"] - r["x"]).max(), rel_l2(h["v"], r["v"]), rel_l2(h["F"], r["F"]),
                                                  (h["states"].astype(np.uint32) != r["states"].astype(np.uint32)).sum()))
    assert np.abs(h["x"] - r["x"]).max() <= 5e-6
    assert rel_l2(h["v"], r["v"]) <= 2e-4
    assert rel_l2(h["F"], r["F"]) <= 1e-4
    assert (h["states"].astype(np.uint32) != r["states"].astype(np.uint32)).sum() <= 5
    for a, b in zip(one["bodies"], got["bodies"]):
        print("pose %.3g  velocities %.3g of %.3g" % (np.abs(b[0:7] - a[0:7]).max(), np.abs(b[7:13] - a[7:13]).max(), np.abs(a[7:13]).max()))
        np.testing.assert_allclose(b[0:7], a[0:7], rtol=0, atol=2e-6)
        np.testing.assert_allclose(b[7:13], a[7:13], rtol=0, atol=2e-4 * max(np.abs(a[7:13]).max(), 1e-2))


def same_bits(a, b):
    return all(a["p"][k].shape == b["p"][k].shape and np.ascontiguousarray(a["p"][k]).tobytes() == np.ascontiguousarray(b["p"][k]).tobytes()
               for k in FIELDS) and all(x.tobytes() == y.tobytes() for x, y in zip(a["bodies"], b["bodies"]))


# computed once, shared, left unchanged
@pytest.fixture(scope="module")
def one_two_bodies(tm):
    return run_one(tm, two_bodies())


@pytest.fixture(scope="module")
def jobs_two_bodies(tm):
    """the jobs of the two-body scene the tests below share: (world, mode) -> result"""
    cache = {}

    def get(world, mode):
        key = (world, mode)
        if key not in cache:
            cache[key] = run_job(tm, two_bodies(), world, halo_by_rccl=(mode == "det_rccl"), **(dict(deterministic=True) if mode != "default" else {}))
        return cache[key]
    return get


# ------------------------------------------------------------------------------------------------ 1. two bodies across the cuts
@pytest.mark.parametrize("world", [2, 8])
def test_two_bodies_across_the_cuts_match_one_ctx(tm, one_two_bodies, jobs_two_bodies, world):
    one = one_two_bodies
    st = one["p"]["states"].astype(np.uint32)
    assert ((st & 0xC) != 0).sum() > 300 and ((st & 0x30) != 0).sum() > 300  # both bodies colour particles in the one-ctx result
    got = jobs_two_bodies(world, "default")
    for mask in (0xC, 0x30):  # ... and in the job, coloured particles of each body live on at least 2 ranks
        holders = sum(1 for s in got["rank_states"] if ((s & mask) != 0).any())
        assert holders >= 2, (hex(mask), holders)
    print("records migrated:", got["migrated"])
    against_one_ctx(got, one)


def test_coloured_records_that_cross_a_cut_keep_their_colour(tm):
    """The velocities of block_of_particles (0.3 m/s) move no record across a cut in 12 substeps.  Here the block drifts at 3 m/s along
    x, 0.115 cells in 12 substeps: records next to the cut at 16 change ranks, coloured ones among them, and the job still is the one
    ctx within the same tolerances (the colour word travels in RecG.pad)."""
    scene = two_bodies()
    scene["v"] = scene["v"] + np.float32([3.0, 0.0, 0.0])
    one = run_one(tm, scene)
    job, sims = build_job(tm, scene, 2)
    before =[set(int(i) for i in sim.get_particles(sort_by_id=False)["id"]) for sim in sims]
    job.run(N_SUB)
    tot = job.totals()
    assert tot["error"] == 0 and tot["migrated"] > 0
    p1 = sims[1].get_particles(sort_by_id=False)
    arrived = np.array([int(i) not in before[1] for i in p1["id"]])
    print("records migrated: %d, arrived on rank 1: %d, coloured among them: %d" % (tot["migrated"], arrived.sum(), (p1["states"][arrived] != 0).sum()))
    assert (p1["states"][arrived] != 0).sum() > 0
    got = dict(p=gather(sims), bodies=body_vectors(job.get_rigid_state, [1, 2]))
    assert len(set(job.rigid_digests())) == 1
    for sim in sims:
        sim.close()
    against_one_ctx(got, one)


# ------------------------------------------------------------------------------------------------ 2. replicas stay one
@pytest.mark.parametrize("mode", ["default", "deterministic"])
@pytest.mark.parametrize("world", [2, 8])
def test_replicas_stay_one(jobs_two_bodies, world, mode):
    got = jobs_two_bodies(world, mode)
    assert len(got["digests"]) == world and len(set(got["digests"])) == 1, got["digests"]
    for bodies in got["rank_bodies"]:  # (the records behind the digests: every rank's state of every body, bit for bit)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(bodies, got["rank_bodies"][0]))


# ------------------------------------------------------------------------------------------------ 3. deterministic mode
def test_deterministic_two_runs_end_byte_identical(tm, jobs_two_bodies):
    a = jobs_two_bodies(8, "deterministic")
    b = run_job(tm, two_bodies(), 8, deterministic=True)
    assert same_bits(a, b)


def test_deterministic_halo_by_rccl_gives_the_bits_of_the_peer_write_job(jobs_two_bodies, one_two_bodies):
    a, b = jobs_two_bodies(8, "deterministic"), jobs_two_bodies(8, "det_rccl")
    assert same_bits(a, b)
    against_one_ctx(a, one_two_bodies)


# ------------------------------------------------------------------------------------------------ 4. a body that touches nothing
def test_a_body_that_touches_nothing_falls_as_on_one_ctx(tm):
    one, got = run_one(tm, falls_alone()), run_job(tm, falls_alone(), 2)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one["bodies"], got["bodies"]))  # all rows are zero: bit for bit
    assert (got["p"]["states"] == 0).all() and (one["p"]["states"] == 0).all()
    assert len(set(got["digests"])) == 1
    assert abs(got["bodies"][0][8] - (-10.0 * N_SUB * 1e-4)) < 1e-6  # it fell


# ------------------------------------------------------------------------------------------------ 5. a joint and a level set
@pytest.mark.parametrize("name", ["joint", "levelset"])
def test_a_joint_and_a_level_set_match_one_ctx(tm, name):
    scene = two_bodies_with_a_joint() if name == "joint" else box_on_levelset()
    one, got = run_one(tm, scene), run_job(tm, scene, 2)
    against_one_ctx(got, one)
    assert len(set(got["digests"])) == 1
    if name == "joint":  # the joint acts: the free box does not move as without it
        free = run_one(tm, two_bodies())
        assert free["bodies"][0][7:13].tobytes() != one["bodies"][0][7:13].tobytes()


# ------------------------------------------------------------------------------------------------ 6. two processes over the IPC wire
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
        scene = two_bodies()
        part = partition(tiled, scene["res"], world)
        owner = part.rank_of_cells(tiled.base_cells(scene["x"], 1.0 / scene["res"]))
        sim, rids = build(tm, scene, owner == rank, device=device, deterministic=True)
        job = tiled.NativeTiledJob(tiled.HipEngine(sim, device), part, rank, world, wire="ipc", dist=dist, migrate_interval=2, overlap=False)
        job.run(N_SUB)
        job.synchronize()
        totals, digests = job.totals(), job.rigid_digests()
        dist.barrier()  # nobody unmaps an arena a peer may still write to
        p = sim.get_particles(sort_by_id=False)
        q.put((rank, totals, digests, {k: p[k] for k in FIELDS}, body_vectors(sim.get_rigid_state, rids)))
        sim.close()
    finally:
        dist.destroy_process_group()


def test_two_processes_over_the_ipc_wire_give_the_bits_of_the_virtual_job(jobs_two_bodies):
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
    want = jobs_two_bodies(2, "deterministic")
    got = {k: np.concatenate([r[3][k] for r in res]) for k in FIELDS}
    order = np.argsort(got["id"], kind="stable")
    ipc = dict(p={k: v[order] for k, v in got.items()}, bodies=res[0][4])
    assert all(r[1]["error"] == 0 for r in res)
    assert same_bits(ipc, want)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(res[0][4], res[1][4]))
    assert res[0][2] == res[1][2] and len(set(res[0][2])) == 1  # every rank sees every rank's digest, all equal


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_what_a_job_with_bodies_refuses(tm, tmp_path):
    from taichi_mpm_amd import tiled
    from taichi_mpm_amd.mpm import MPMError
    L = tm.load()
    live0 = L.mpmhip_debug_live_buffers()
    scene = two_bodies()
    part = partition(tiled, scene["res"], 2)
    # the callback path
    sim, _ = build(tm, scene)
    with pytest.raises(MPMError, match="callback path"):
        tiled.VirtualTiledJob([tiled.HipEngine(sim, 0), tiled.HipEngine(sim, 0)], part)
    with pytest.raises(MPMError, match="callback path"):
        tiled.TiledJob(tiled.HipEngine(sim, 0), part, None)
    tiled.set_partition(sim, part, 0)  # (a partition alone is accepted)
    buf = tiled.HipEngine(sim, 0).alloc(64)
    hb = (tiled._lib.HaloBox * 1)()
    hb[0].lo[:], hb[0].hi[:], hb[0].peer = (15, 0, 0), (16, 2, 2), 1
    hb[0].send = hb[0].recv = buf.data_ptr()
    assert L.mpmhip_set_halo(sim._ctx, 1, hb) == -1 and b"callback path" in L.mpmhip_last_error(sim._ctx)
    assert L.mpmhip_tiled_run(sim._ctx, 1, 0, tiled._lib.EXCHANGE_FN(lambda u, p: 0), None) == -1 and b"callback path" in L.mpmhip_last_error(sim._ctx)
    sim.close()
    # rigid_body_collision on a tiled ctx
    sim, _ = build(tm, scene, rigid_body_collision=True)
    with pytest.raises(MPMError, match="rigid_body_collision is not supported on a tiled"):
        tiled.native_setup(tiled.HipEngine(sim, 0), part, 0, tiled._lib.WIRE_LOCAL, 2)
    sim.run_substeps(1)  # (the ctx steps on as the one ctx it still is)
    sim.close()
    # ranks that do not hold the same bodies
    a, b = build(tm, scene)[0], build(tm, dict(scene, bodies=scene["bodies"][:1]))[0]
    with pytest.raises(MPMError, match="rank 1 holds 1 rigid bodies"):
        tiled.NativeVirtualJob([tiled.HipEngine(a, 0), tiled.HipEngine(b, 0)], part, migrate_interval=2)
    a.close(), b.close()
    # the job itself
    job, sims = build_job(tm, scene, 2)
    job.run(2)
    before = gather(sims), job.rigid_digests(), job.state()
    with pytest.raises(MPMError, match="before mpmhip_tiled_setup"):  # a body added after the set-up
        sims[0].add_particles(dict(type="rigid", mesh=cs.plate(0.05), codimensional=True, initial_position=(0.3, 0.3, 0.5)))
    with pytest.raises(MPMError, match="asynchronous stepping"):
        sims[0].enable_async()
    job.frame_directory = str(tmp_path)
    for call in (job.rebalance, lambda: job.rebalance(force=True), job.bgeo_bytes, job.visualize, lambda: job.save_snapshot(str(tmp_path / "s.bin")),
                 lambda: job.load_snapshot(b"\0" * 4096), job.snapshot_bytes):
        with pytest.raises(MPMError, match="rigid bodies"):
            call()
    with pytest.raises(MPMError, match="rigid bodies"):
        job.calculate_energy()
    after = gather(sims), job.rigid_digests(), job.state()
    assert all(before[0][k].tobytes() == after[0][k].tobytes() for k in FIELDS) and before[1:] == after[1:]  # state untouched
    job.set_overlap(True)  # accepted and ignored
    job.run(2)
    assert job.totals()["error"] == 0 and len(set(job.rigid_digests())) == 1
    for s in sims:
        s.close()
    assert L.mpmhip_debug_live_buffers() == live0


# ------------------------------------------------------------------------------------------------ 8. emitter
def test_an_emitter_on_a_job_with_bodies_adds_what_one_ctx_adds(tm):
    scene = two_bodies()
    emit = dict(type="sand", ppc=8.0, region=tm.mpm.LevelSet().add_sphere((0.5, 0.78, 0.5), 3.0 * cs.DX))
    one, _ = build(tm, scene, extra=8192)
    n0 = one.get_num_particles()
    one.add_particles(dict(emit))
    added = one.get_num_particles() - n0
    one.close()
    assert added > 300
    job, sims = build_job(tm, scene, 8, extra=8192)
    job.run(2)
    job.sync_next_id()
    counts = job.add_particles(dict(emit))
    assert all(jobwide == added for _, jobwide in counts) and sum(here for here, _ in counts) == added
    job.run(2)  # (the planning scan wraps the boxes round the new particles; the bodies go on)
    assert job.totals()["error"] == 0 and job.totals()["particles"] == n0 + added and len(set(job.rigid_digests())) == 1
    for s in sims:
        s.close()
