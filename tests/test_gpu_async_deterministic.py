"""The deterministic mode of the asynchronous steppers, 3D and 2D (csrc/k_async.h: k_async_gather_ordered, k_async_file_ordered,
k_async_load_ordered, k_async_export_ordered; csrc/async_api.h): with `deterministic` on, a resident stepper is a function of its
configuration, its level set and the calls it receives — the store is in filing order, working sets / views / exported rows in
store order, and everything read from them is byte-identical between runs and across launch sizes (MPMHIP_ASYNC_WGS).
Scenes: the 3D two-stiffness scene of tests/test_gpu_async.py, the 2D one of tests/test_gpu_async2d.py at RES2.
Models: tests/async_order_model.py (checked on the host by tests/test_async_order_cpu.py)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from tests.async_order_model import INVALID, async_block_of, pooled_store
from tests.common import lattice_cube, make_state, rel_l2

pytestmark = pytest.mark.gpu
KW = dict(unit_delta_t=2e-6, max_units=1024)
RES3 = 32
RES2 = 32   # the 2D scene scaled down (two squares of 6 cells): its blocks still step with two sizes, 256 and 1024 units
ID_COL = {3: 26, 2: 14}


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


@contextlib.contextmanager
def _async_wgs(n):
    """MPMHIP_ASYNC_WGS in the environment while a session begins (that is when it is read), restored afterwards"""
    old = os.environ.get("MPMHIP_ASYNC_WGS")
    if n is None:
        os.environ.pop("MPMHIP_ASYNC_WGS", None)
    else:
        os.environ["MPMHIP_ASYNC_WGS"] = str(n)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("MPMHIP_ASYNC_WGS", None)
        else:
            os.environ["MPMHIP_ASYNC_WGS"] = old


def _scene(dim):
    """[(material, add_particles config)] : the soft body, then the stiff one"""
    if dim == 3:
        dx = 1.0 / RES3
        xa = lattice_cube(RES3, 9, 15, dx, jitter=0.2, seed=1)
        xb = lattice_cube(RES3, 15, 21, dx, jitter=0.2, seed=2)
        sa = make_state(xa, "elastic", dx, perturb_F=0.01, vel_scale=0.5)  # soft: E = 5e3
        sb = make_state(xb, "sand", dx, perturb_F=0.01, vel_scale=0.5)     # stiff
        return [dict(type=m, positions=s.x, velocities=s.v, F=s.F, B=s.B, aux=s.aux, params=s.gparams[0]) for s, m in ((sa, "elastic"), (sb, "sand"))]
    import taichi_mpm_amd as tm
    from tests.golden.make_golden import mpm2d_state
    res = RES2
    dx = 1.0 / res
    vol = dx * dx / 4
    k = res / 128.0
    lo, cells = (int(30 * k), int(40 * k)), int(24 * k)
    xa, va, Fa, Ba = mpm2d_state(res, lo=lo, cells=cells, seed=3)
    xb, vb, Fb, Bb = mpm2d_state(res, lo=(lo[0] + cells, lo[1]), cells=cells, seed=4)
    gpa, _ = tm.group_params("elastic", 400 * vol, vol)
    gpb, _ = tm.group_params("sand", 400 * vol, vol)
    return [dict(type="elastic", positions=xa, velocities=0.3 * va, F=Fa, B=Ba, params=gpa),
            dict(type="sand", positions=xb, velocities=0.3 * vb, F=Fb, B=Bb, params=gpb)]


def _sim(tm, dim, det, wgs=None, **extra):
    """a fresh asynchronous simulation with its ctx created (the session begun) under MPMHIP_ASYNC_WGS = wgs"""
    res = RES3 if dim == 3 else RES2
    make = tm.create_simulation3 if dim == 3 else tm.create_simulation2
    sim = make("async_mpm").initialize(dict(res=(res,) * dim, delta_x=1.0 / res, deterministic=det, **KW, **extra))
    sim.set_levelset(tm.mpm.LevelSet(friction=0.4).add_plane((0, 1, 0), d=-0.2))
    with _async_wgs(wgs):
        sim._ensure_ctx()
    return sim


def _ids(rows, dim):
    return np.ascontiguousarray(rows[:, ID_COL[dim]]).view(np.int32)


# ------------------------------------------------------------------------------------------ 1. the forms
@pytest.mark.parametrize("dim", [3, 2])
def test_the_mode_selects_the_ordered_forms_and_the_default_the_plain_ones(tm, dim):
    soft = _scene(dim)[0]
    sims = {}
    for det in (True, False):
        sim = sims[det] = _sim(tm, dim, det)
        assert sim.async_forms() == [-1, -1, -1, -1]  # nothing launched in this session yet
        sim.add_particles(soft)
        sim.step(2e-3)
        sim.get_pool_particles()
        sim.bgeo_bytes()
        assert sim.async_forms() == [int(det)] * 4, (dim, det)
    sim = sims[True]
    sim.set_deterministic(False)
    sim.step(2e-3)
    assert sim.async_forms()[:2] == [0, 0]  # the next gather and the next filing: by arrival again
    sim.get_pool_particles()
    sim.bgeo_bytes()
    assert sim.async_forms() == [0, 0, 0, 0]
    sim.set_deterministic(True)  # ... and back, on the resident stepper
    sim.step(2e-3)
    sim.get_pool_particles()
    sim.bgeo_bytes()
    assert sim.async_forms() == [1, 1, 1, 1]
    for s in sims.values():
        s.close()


# ------------------------------------------------------------------------------------------ 2. pooled order against a model
def _batches(dim, res):
    """1000, 1024 and 1500 positions (the chunk of the ordered kernels is 1024), five of each below half a cell along one axis:
    async_block_of drops those"""
    rng = np.random.default_rng(100 + dim)
    out = []
    for n in (1000, 1024, 1500):
        x = rng.uniform(8.0 / res, 1 - 8.0 / res, (n, dim)).astype(np.float32)
        x[rng.choice(n, 5, replace=False), rng.integers(0, dim, 5)] = np.float32(0.3 / res)
        out.append(x)
    return out


@pytest.mark.parametrize("mode", ["ordered", "ordered_wgs3", "default"])
@pytest.mark.parametrize("dim", [3, 2])
def test_pooled_batches_lie_in_upload_order(tm, dim, mode):
    """before any step (the substep's own deletions stay out of it): the id column of the raw rows of download_pools = the
    creation ids of the kept particles in upload order, the block column = async_block_of; with the mode off only as sets"""
    res = RES3 if dim == 3 else RES2
    batches = _batches(dim, res)
    sim = _sim(tm, dim, mode != "default", wgs=3 if mode == "ordered_wgs3" else None, max_particles=2048)
    L, ctx, fp = sim._L, sim._ctx, C.POINTER(C.c_float)
    add_group, add, pool = ((L.mpmhip_add_group, L.mpmhip_add_particles, L.mpmhip_async_pool_particles) if dim == 3 else
                            (L.mpmhip2d_add_group, L.mpmhip2d_add_particles, L.mpmhip2d_async_pool_particles))
    vol = (1.0 / res) ** dim / 2 ** dim
    gp, mat = tm.group_params("elastic", 400 * vol, vol)
    gp = np.ascontiguousarray(gp, np.float32)
    sim._check(add_group(ctx, mat, gp.ctypes.data_as(fp)))
    for x in batches:  # (through the C ABI: the Python layer would drop the positions near the boundary itself)
        sim._check(add(ctx, 0, len(x), x.ctypes.data_as(fp), None, None, None, None))
        sim._check(pool(ctx))
    rows, blk = sim.download_pools()
    want_ids, want_blk = pooled_store(batches, res, dim)
    assert len(want_ids) == 1000 + 1024 + 1500 - 15
    got_ids = _ids(rows, dim).astype(np.int64)
    if mode == "default":
        assert sim.async_forms()[1::2] == [0, 0]
        assert sorted(zip(got_ids.tolist(), blk.tolist())) == sorted(zip(want_ids.tolist(), want_blk.tolist()))
    else:
        assert sim.async_forms()[1::2] == [1, 1]
        assert np.array_equal(got_ids, want_ids)
        assert np.array_equal(blk.astype(np.int64), want_blk)
        assert np.array_equal(rows[:, :dim], np.concatenate(batches)[want_ids])  # ... and every row is its particle's
    sim.close()


# ------------------------------------------------------------------------------------------ 3. run against run, across launch sizes
def _run_script(tm, dim, wgs, path):
    """the soft body, a step, the stiff body, a step, then steps until the store has been compacted; everything the mode promises"""
    soft, stiff = _scene(dim)
    sim = _sim(tm, dim, True, wgs=wgs)
    sim.add_particles(soft)
    sim.step(2e-3)
    sim.add_particles(stiff)
    sim.step(2e-3)
    steps = 2
    while sim._state()[6] < 1 and steps < 20:
        sim.step(2e-3)
        steps += 1
    st = sim._state()
    assert st[6] >= 1, "the store was never compacted: %r" % (st,)
    rows, blk = sim.download_pools()
    out = dict(rows=rows.tobytes(), blk=blk.tobytes(), n=len(blk), bgeo=sim.bgeo_bytes(), update_counter=sim.update_counter,
               current_t_int=sim.current_t_int, steps=steps, compactions=st[6], forms=sim.async_forms())
    out.update({"table_" + k: np.asarray(v).tobytes() for k, v in sim.block_table().items()})
    sim.save_snapshot(path)
    out["snapshot"] = open(path, "rb").read()
    sim.close()
    return out


@pytest.fixture(scope="module")
def three_runs(tm, tmp_path_factory):
    cache = {}

    def get(dim):
        if dim not in cache:
            d = tmp_path_factory.mktemp("det%dd" % dim)
            cache[dim] = [_run_script(tm, dim, wgs, str(d / ("run%d.snap" % i))) for i, wgs in enumerate((None, None, 3))]
        return cache[dim]
    return get


@pytest.mark.parametrize("dim", [3, 2])
def test_three_runs_of_one_script_give_the_same_bytes_whatever_the_launch_size(three_runs, dim):
    a, b, c = three_runs(dim)
    assert a["forms"] == [1, 1, 1, 1] and a["n"] > 0
    if dim == 3:
        assert a["n"] > 2 * 1024  # the store spans several chunks of the ordered kernels
    for name, other in (("second run", b), ("MPMHIP_ASYNC_WGS=3", c)):
        for k in a:
            assert a[k] == other[k], "%s differs: %s" % (name, k)


# ------------------------------------------------------------------------------------------ 4. the working set is in store order
@pytest.mark.parametrize("dim", [3, 2])
def test_a_view_of_the_pools_lists_them_in_store_order(tm, dim):
    soft, stiff = _scene(dim)
    sim = _sim(tm, dim, True, wgs=3)
    sim.add_particles(soft)
    sim.add_particles(stiff)
    for steps in range(1, 9):  # 3D: until an id sits in more than one pool (the 2D scene never gets there: its order is checked without)
        sim.step(2.5e-3)
        rows, blk = sim.download_pools()
        ids = _ids(rows, dim)
        if len(ids) > len(np.unique(ids)) or (dim == 2 and steps == 2):
            break
    print("dim %d: %d containers, %d ids after %d steps" % (dim, len(ids), len(np.unique(ids)), steps))
    if dim == 3:
        assert len(ids) > len(np.unique(ids)), "the scene must hold an id in more than one pool"
    p = sim.get_particles(sort_by_id=False)  # load_pools: k_async_load_ordered
    assert sim.async_forms()[2:] == [1, 1]
    assert np.array_equal(p["id"], ids)  # (same sequence: duplicates of an id in the same relative order as well)
    if dim == 3:
        got = np.concatenate([p["x"], p["v"], p["F"], p["B"], p["aux"][:, None]], 1)
        assert np.array_equal(got, rows[:, :25]) and np.array_equal(p["gid"], np.ascontiguousarray(rows[:, 25]).view(np.int32))
        # a pool container was filed by its position and has not moved since: the view's blocks follow from its positions
        assert np.array_equal(async_block_of(p["x"], RES3, 3), blk.astype(np.int64))
    else:
        got = np.concatenate([p["x"], p["v"], p["F"], p["B"], p["aux"][:, None]], 1)
        assert np.array_equal(got, rows[:, :13])
        vb = np.zeros(len(ids), np.int32)
        assert int(sim._check(sim._L.mpmhip2d_async_view_blocks(sim._ctx, len(vb), vb.ctypes.data_as(C.POINTER(C.c_int32))))) == len(vb)
        assert np.array_equal(vb, blk)
    assert (blk.astype(np.int64) != INVALID).all()
    sim.close()


# ------------------------------------------------------------------------------------------ 5. the physics did not move
def test_the_mode_matches_the_reference_async_stepper_3d(tm):
    """tests/test_gpu_async.py::test_async_stepping_matches_the_reference_async_stepper's assertions, in the mode"""
    from oracle import refmpm as ref
    if not ref.available():
        pytest.skip("oracle/_ref/libmpm_ref.so did not travel to this box")
    ref.set_threads(1)
    r = ref.AsyncSim(RES3, 1.0 / RES3, shapes=[(0, 0, 0, 1, 0, -0.2)], friction=0.4, **KW)
    sim = _sim(tm, 3, True)
    for cfg in _scene(3):
        gp = cfg["params"]
        r.add_particles(cfg["type"], gp[0], gp[1], cfg["positions"], cfg["velocities"], cfg["F"], cfg["B"], cfg["aux"])
        sim.add_particles(cfg)
    for _ in range(2):
        r.step(2.5e-3)
        sim.step(2.5e-3)
    assert sim.async_forms()[:2] == [1, 1]
    assert sim.current_t_int == r.time_int()
    assert sim.update_counter == r.update_counter()
    a, b = sim.get_pool_particles(), r.download()
    assert np.array_equal(a["id"], b["id"])
    assert len(np.unique(b["limits"][:, 0])) >= 2, "the scene must step with at least two block step sizes"
    assert np.array_equal(a["continuous"], b["limits"][:, 0]) and np.array_equal(a["particle_t"], b["limits"][:, 3])
    assert np.abs(a["x"] - b["x"]).max() <= 1e-6
    assert rel_l2(a["v"], b["v"]) <= 5e-4 and rel_l2(a["F"], b["F"]) <= 1e-4
    sim.close(); r.close()


def test_the_mode_matches_the_reference_async_stepper_2d(tm):
    """tests/test_gpu_async2d.py::test_async_stepping_2d_matches_the_reference_async_stepper's assertions, in the mode"""
    from oracle import refmpm as ref
    if not ref.available():
        pytest.skip("oracle/_ref/libmpm_ref.so did not travel to this box")
    ref.set_threads(1)
    r = ref.AsyncSim(RES2, 1.0 / RES2, dim=2, shapes=[(0, 0, 0, 1, 0, -0.2)], friction=0.4, **KW)
    sim = _sim(tm, 2, True)
    for cfg in _scene(2):
        gp = cfg["params"]
        r.add_particles(cfg["type"], gp[0], gp[1], cfg["positions"], cfg["velocities"], cfg["F"], cfg["B"], None)
        sim.add_particles(cfg)
    for _ in range(2):
        r.step(2.5e-3)
        sim.step(2.5e-3)
    assert sim.async_forms()[:2] == [1, 1]
    assert sim.current_t_int == r.time_int()
    assert sim.update_counter == r.update_counter()
    assert (sim.min_delta_t_int, sim.max_delta_t_int) != (1, 1)
    a, b = sim.get_pool_particles(), r.download()
    assert np.array_equal(a["id"], b["id"])
    assert len(np.unique(b["limits"][:, 0])) >= 2, "the scene must step with at least two block step sizes"
    assert np.array_equal(a["continuous"], b["limits"][:, 0]) and np.array_equal(a["particle_t"], b["limits"][:, 3])
    assert np.abs(a["x"] - b["x"]).max() <= 1e-6
    assert rel_l2(a["v"], b["v"]) <= 5e-4 and rel_l2(a["F"], b["F"]) <= 1e-4 and rel_l2(a["B"], b["B"]) <= 2e-3
    want, mm = r.blocks()
    tab = sim.block_table()
    blk = (want["coord"][:, 0] >> 3) * tab["nb"][1] + (want["coord"][:, 1] >> 4)
    assert np.array_equal(tab["count"][blk], want["count"]) and np.array_equal(tab["continuous"][blk], want["continuous"])
    assert (sim.min_delta_t_int, sim.max_delta_t_int) == tuple(int(v) for v in mm)
    sim.close(); r.close()


# ------------------------------------------------------------------------------------------ 6. snapshot round trip in the mode
@pytest.mark.parametrize("dim", [3, 2])
def test_a_snapshot_restart_continues_bit_for_bit(tm, tmp_path, dim):
    a = _sim(tm, dim, True)
    for cfg in _scene(dim):
        a.add_particles(cfg)
    a.step(2.5e-3)
    path = str(tmp_path / "async.snap")
    a.save_snapshot(path)
    b = _sim(tm, dim, True)
    b.load_snapshot(path)
    a.step(2.5e-3)
    b.step(2.5e-3)
    assert a.current_t_int == b.current_t_int and a.update_counter == b.update_counter
    (ra, ba), (rb, bb) = a.download_pools(), b.download_pools()
    assert len(ba) > 0 and ra.tobytes() == rb.tobytes() and ba.tobytes() == bb.tobytes()
    a.close(); b.close()
