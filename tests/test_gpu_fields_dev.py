"""GPU tests of the device-pointer field calls (include/mpmhip.h: mpmhip_download_dev, mpmhip_upload_dev, mpmhip_download_grid_dev;
csrc/k_fields.h, csrc/fields_api.h) and of the torch-tensor API on top of them (Simulation3D.get_particle_tensors,
set_particle_tensors, get_grid_tensor).

The yardstick is the host path of the same ctx (mpmhip_download / mpmhip_upload / mpmhip_download_grid), so every comparison is
BITWISE: np.array_equal on the uint32 view of every field.  Destinations are torch tensors with GUARD rows of a sentinel behind the
expected count; every test asserts the guards (and every tensor it did not ask for) still hold the sentinel.

Shapes: the kernels take a lane per slot in workgroups of W = 256 and scan the workgroup totals 256 per trip, so the scenes are
1 particle, W - 1, W and W + 1 slots, and one of 74 088 slots (> 256 * 256: the scan takes a second trip) in which
delete_particles_inside_level_set has killed a ball in the middle without a sort — dead slots inside and across workgroup borders —
and the same after 3 substeps (records compacted and permuted by the sort, B recovered from the affine matrix: keep_apic_b is off).

Not covered: the in-substep refusal on a PARTITIONED ctx (mpmhip_substep_begin works on a plain ctx too, which is what test 9 uses)."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests.common import lattice_cube, make_state, mixed_state

pytestmark = pytest.mark.gpu

W = 256  # FIELDS_WG of csrc/fields_launch.h
GUARD = 5
FIELDS = ("x", "v", "B", "F", "aux", "gid", "id", "states")
INDEX = {k: i for i, k in enumerate(FIELDS)}  # MPMHIP_F_*
WIDTH = dict(x=3, v=3, B=9, F=9, aux=1, gid=1, id=1, states=1)
INTS = ("gid", "id", "states")
F_SENTINEL, I_SENTINEL = -777.25, -7777777
EINVAL, ECAPACITY = -1, -4
RES, DX, DT = 48, 1.0 / 48, 1e-4


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ------------------------------------------------------------------------------------------------ scenes
def _build(tm, s, **cfg):
    sim = tm.create_simulation3("mpm")
    sim.initialize(dict(dict(res=(RES,) * 3, delta_x=DX, base_delta_t=DT, max_particles=s.n + 64), **cfg))
    sim.set_levelset(tm.mpm.LevelSet())
    names = {v: k for k, v in tm.MATERIAL_IDS.items()}
    for gi in range(len(s.gtype)):
        m = s.gid == gi
        sim.add_particles(dict(type=names[int(s.gtype[gi])], positions=s.x[m], velocities=s.v[m], F=s.F[m], B=s.B[m], aux=s.aux[m],
                               params=s.gparams[gi]))
    sim._ensure_ctx()
    return sim


def _kill_ball(tm, sim, radius=0.12):
    """delete_particles_inside_level_set with a ball in the middle, no sort behind it: dead slots between the live ones"""
    before = sim.get_num_particles()
    sim.set_levelset(tm.mpm.LevelSet().add_sphere((0.5, 0.5, 0.5), radius))
    sim.general_action(dict(action="delete_particles_inside_level_set"))
    sim.set_levelset(tm.mpm.LevelSet())
    live, slots = sim.get_num_particles(), int(sim._L.mpmhip_num_slots(sim._ctx))
    assert 0 < live < before and slots > live
    return live


@pytest.fixture(scope="module")
def small_state():
    """W + 1 particles; the scenes of 1, W - 1 and W take its first rows"""
    x = lattice_cube(RES, 20, 24, DX, jitter=0.2, seed=3)[:W + 1]
    return make_state(x, "jelly", DX, perturb_F=0.02, seed=4)


@pytest.fixture(scope="module")
def big_state():
    x = lattice_cube(RES, 14, 35, DX, jitter=0.2, seed=5)
    assert len(x) > W * 256
    return mixed_state(x, ("jelly", "sand"), DX, seed=6, perturb_F=0.02)


@pytest.fixture(scope="module")
def mid_state():
    """5 832 particles: 23 workgroups, the scene of the upload twins"""
    return mixed_state(lattice_cube(RES, 19, 28, DX, jitter=0.2, seed=7), ("jelly", "sand"), DX, seed=8, perturb_F=0.02)


@pytest.fixture(scope="module")
def big_dead(tm, big_state):
    sim = _build(tm, big_state)
    _kill_ball(tm, sim)
    yield sim
    sim.close()


@pytest.fixture(scope="module")
def big_stepped(tm, big_state):
    sim = _build(tm, big_state)
    _kill_ball(tm, sim)
    sim.run_substeps(3)
    sim.synchronize()
    yield sim
    sim.close()


# ------------------------------------------------------------------------------------------------ helpers
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _host(sim):
    """the eight fields through mpmhip_download, in slot order"""
    return sim.get_particles(sort_by_id=False)


def _by_id(p):
    order = np.argsort(p["id"], kind="stable")
    return {k: v[order] for k, v in p.items()}


def _dest(torch, n, names=FIELDS):
    out = {}
    for k in names:
        shape = (n + GUARD,) if WIDTH[k] == 1 else (n + GUARD, WIDTH[k])
        out[k] = (torch.full(shape, I_SENTINEL, dtype=torch.int32, device="cuda") if k in INTS
                  else torch.full(shape, F_SENTINEL, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()  # (the library works on the ctx's own stream)
    return out


def _table(tensors, names):
    t = (C.c_void_p * 8)()
    for k in names:
        t[INDEX[k]] = tensors[k].data_ptr()
    return t


def _untouched(t, first=0):
    sentinel = I_SENTINEL if t.dtype.is_floating_point is False else F_SENTINEL
    return bool((t[first:] == sentinel).all().item())


def _download_dev(torch, sim, names, order, n, capacity=None):
    """(return value, all eight destination tensors) of one mpmhip_download_dev that asks for `names`"""
    dest = _dest(torch, n)
    got = sim._L.mpmhip_download_dev(sim._ctx, _table(dest, names), n if capacity is None else capacity, order)
    return int(got), dest


def _check_download(torch, sim, order, names=FIELDS):
    ref = _host(sim)
    if order == 1:
        ref = _by_id(ref)
    n = len(ref["id"])
    got, dest = _download_dev(torch, sim, names, order, n)
    assert got == n, (got, n, sim._L.mpmhip_last_error(sim._ctx))
    for k in FIELDS:
        if k in names:
            assert _untouched(dest[k], n), "guard rows of %s" % k
            assert _same(dest[k][:n].cpu().numpy(), ref[k]), "field %s, order %d" % (k, order)
        else:
            assert _untouched(dest[k]), "%s was not asked for" % k
    return n


def _error(sim):
    return sim._L.mpmhip_last_error(sim._ctx).decode()


# ------------------------------------------------------------------------------------------------ 1, 2. download, both orders
@pytest.mark.parametrize("n", [1, W - 1, W, W + 1])
def test_slot_and_id_order_on_one_and_two_workgroups(tm, torch, small_state, n):
    s = small_state
    sub = type(s)(s.x[:n], s.v[:n], s.B[:n], s.F[:n], s.aux[:n], s.gid[:n], s.gparams, s.gtype)
    sim = _build(tm, sub)
    assert int(sim._L.mpmhip_num_slots(sim._ctx)) == n
    assert _check_download(torch, sim, 0) == n
    assert _check_download(torch, sim, 1) == n
    sim.close()


def test_slot_order_with_dead_slots_inside_and_across_workgroups(torch, big_dead):
    sim = big_dead
    slots = int(sim._L.mpmhip_num_slots(sim._ctx))
    assert slots > W * 256  # the scan of the workgroup totals takes more than one trip
    n = _check_download(torch, sim, 0)
    dead = np.ones(slots, np.int64)
    dead[_host(sim)["id"]] = 0  # (no sort yet: slot = creation id)
    w = np.add.reduceat(dead, np.arange(0, slots, W))
    assert n < slots and ((w > 0) & (w < W)).sum() > 8  # the ball's dead slots share workgroups with live ones


def test_slot_order_after_substeps_recovers_b(torch, big_stepped):
    _check_download(torch, big_stepped, 0)


def test_id_order_with_gaps_in_the_ids(torch, big_dead):
    ids = _host(big_dead)["id"]
    assert ids.max() + 1 > len(ids)  # the deletion left gaps
    _check_download(torch, big_dead, 1)


def test_id_order_after_the_sort_permuted_the_slots(torch, big_stepped):
    ids = _host(big_stepped)["id"]
    assert not np.array_equal(ids, np.sort(ids))
    _check_download(torch, big_stepped, 1)


# ------------------------------------------------------------------------------------------------ 3. subsets
@pytest.mark.parametrize("names", [(k,) for k in FIELDS] + [("x", "id", "F"), ("v", "B", "aux", "states")], ids="+".join)
@pytest.mark.parametrize("order", [0, 1])
def test_subsets_leave_the_other_tensors_alone(torch, big_stepped, names, order):
    _check_download(torch, big_stepped, order, names)


# ------------------------------------------------------------------------------------------------ 4. capacity
@pytest.mark.parametrize("order", [0, 1])
def test_capacity_is_judged_before_anything_is_written(torch, big_dead, order):
    sim = big_dead
    n = sim.get_num_particles()
    got, dest = _download_dev(torch, sim, FIELDS, order, n, capacity=n - 1)
    assert got == ECAPACITY and "alive" in _error(sim)
    assert all(_untouched(dest[k]) for k in FIELDS)
    got, dest = _download_dev(torch, sim, FIELDS, order, n, capacity=n)
    assert got == n and all(_untouched(dest[k], n) for k in FIELDS)


# ------------------------------------------------------------------------------------------------ 5. upload parity
def _twin(tm, mid_state):
    """a deterministic scene that has taken 2 substeps and then lost a ball: dead slots between sorted records"""
    sim = _build(tm, mid_state, deterministic=True)
    sim.run_substeps(2)
    _kill_ball(tm, sim, radius=0.06)
    return sim


def _new_values(p, names, seed):
    """new values for the fields `names`, rows in the order of p"""
    rng = np.random.default_rng(seed)
    n = len(p["id"])
    out = {}
    for k in names:
        if k == "x":
            out[k] = (p["x"] + rng.uniform(-0.2, 0.2, (n, 3)) * DX).astype(np.float32)
        elif k == "v":
            out[k] = rng.normal(0, 0.5, (n, 3)).astype(np.float32)
        elif k in ("B", "F"):
            out[k] = (p[k] + rng.normal(0, 0.01, (n, 9))).astype(np.float32)
        elif k == "aux":
            out[k] = (p["aux"] + np.float32(0.01)).astype(np.float32)
        elif k == "states":
            out[k] = rng.integers(0, 4, n).astype(np.int32)
        elif k == "id":
            ids = (rng.permutation(n) * 3 + 5).astype(np.int32)
            ids[n // 2] = -9  # stored as 0
            out[k] = ids
    return out


CASES = [(k,) for k in ("x", "v", "B", "F", "aux", "states", "id")] + [("x", "v", "F")]


@pytest.mark.parametrize("names", CASES, ids="+".join)
@pytest.mark.parametrize("order", [0, 1])
def test_upload_matches_the_host_upload_on_a_twin(tm, torch, mid_state, names, order):
    a, b = _twin(tm, mid_state), _twin(tm, mid_state)
    pa, pb = _host(a), _host(b)
    assert all(_same(pa[k], pb[k]) for k in FIELDS)
    n = len(pa["id"])
    rows = _by_id(pa) if order == 1 else pa  # what row r of the call speaks of
    vals = _new_values(rows, names, seed=11 + order)
    rank = np.argsort(np.argsort(pa["id"], kind="stable"), kind="stable") if order == 1 else np.arange(n)
    for k in names:  # twin A: the host call, field by field, its rows in slot order
        a.upload(INDEX[k], vals[k][rank])
    src = {k: torch.from_numpy(vals[k]).cuda() for k in names}
    torch.cuda.synchronize()
    bytes0, live0 = b._L.mpmhip_host_particle_bytes(b._ctx), int(b._L.mpmhip_debug_live_buffers())
    assert b._L.mpmhip_upload_dev(b._ctx, _table(src, names), n, order) == 0, _error(b)
    assert b._L.mpmhip_host_particle_bytes(b._ctx) == bytes0 and int(b._L.mpmhip_debug_live_buffers()) == live0
    pa, pb = _host(a), _host(b)
    for k in FIELDS:
        assert _same(pa[k], pb[k]), "field %s after the upload of %s" % (k, "+".join(names))
    if "id" in names:
        assert pb["id"].min() == 0 and (pb["id"] == 0).sum() == 1  # the negative id
        assert a._L.mpmhip_set_next_id(a._ctx, 0) == b._L.mpmhip_set_next_id(b._ctx, 0) == int(vals["id"].max()) + 1
    a.run_substeps(3)
    b.run_substeps(3)
    pa, pb = _host(a), _host(b)
    assert len(pa["id"]) == len(pb["id"]) > 0
    for k in FIELDS:
        assert _same(pa[k], pb[k]), "field %s 3 substeps after the upload of %s" % (k, "+".join(names))
    a.close()
    b.close()


def test_upload_never_lowers_the_id_counter(tm, torch, small_state):
    sim = _build(tm, small_state)
    n = small_state.n
    assert sim._L.mpmhip_set_next_id(sim._ctx, 0) == n
    src = dict(id=torch.arange(n, dtype=torch.int32, device="cuda") // 2)  # largest id n // 2: below the counter (and not unique)
    torch.cuda.synchronize()
    assert sim._L.mpmhip_upload_dev(sim._ctx, _table(src, ("id",)), n, 0) == 0, _error(sim)
    assert sim._L.mpmhip_set_next_id(sim._ctx, 0) == n
    sim.close()


def test_upload_refuses_gid_and_a_wrong_count(tm, torch, small_state):
    sim = _build(tm, small_state)
    n = small_state.n
    before = _host(sim)
    src = _dest(torch, n)
    assert sim._L.mpmhip_upload_dev(sim._ctx, _table(src, ("gid",)), n, 0) == EINVAL and "cannot be uploaded" in _error(sim)
    assert sim._L.mpmhip_upload_dev(sim._ctx, _table(src, ("x", "gid")), n, 1) == EINVAL
    for order in (0, 1):
        assert sim._L.mpmhip_upload_dev(sim._ctx, _table(src, ("x",)), n - 1, order) == EINVAL and "holds %d particles" % n in _error(sim)
    after = _host(sim)
    assert all(_same(before[k], after[k]) for k in FIELDS)
    sim.close()


# ------------------------------------------------------------------------------------------------ 6. round trip through torch
def test_round_trip_of_an_edit_across_substeps(tm, torch, mid_state):
    a, b = _twin(tm, mid_state), _twin(tm, mid_state)
    t = a.get_particle_tensors(("v", "id"))
    v = t["v"] * 0.5
    v[:, 1] += 0.25
    a.set_particle_tensors(dict(v=v))
    # the twin: the same numbers through get_particles / upload, its rows in slot order
    ids = b.get_particles(sort_by_id=False)["id"]
    assert np.array_equal(np.sort(ids), t["id"].cpu().numpy())
    from taichi_mpm_amd.mpm import F_V
    b.upload(F_V, v.cpu().numpy()[np.argsort(np.argsort(ids, kind="stable"), kind="stable")])
    a.run_substeps(2)
    b.run_substeps(2)
    pa, pb = a.get_particles(), b.get_particles()
    for k in FIELDS:
        assert _same(pa[k], pb[k]), k
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 7. duplicate ids
def test_duplicate_ids_refuse_id_order_only(tm, torch, small_state):
    from taichi_mpm_amd.mpm import F_ID
    sim = _build(tm, small_state)
    n = small_state.n
    ids = np.arange(n, dtype=np.int32)
    ids[17] = ids[200]
    sim.upload(F_ID, ids)
    before = _host(sim)
    got, dest = _download_dev(torch, sim, FIELDS, 1, n)
    assert got == EINVAL and "not unique" in _error(sim)
    assert all(_untouched(dest[k]) for k in FIELDS)
    src = {k: torch.zeros_like(dest[k][:n]) for k in ("x", "v", "id")}
    torch.cuda.synchronize()
    assert sim._L.mpmhip_upload_dev(sim._ctx, _table(src, ("x", "v", "id")), n, 1) == EINVAL and "not unique" in _error(sim)
    after = _host(sim)
    assert all(_same(before[k], after[k]) for k in FIELDS)
    with pytest.raises(tm.mpm.MPMError, match="not unique"):
        sim.get_particle_tensors()
    assert _check_download(torch, sim, 0) == n  # slot order does not need the ids
    sim.close()


# ------------------------------------------------------------------------------------------------ 8. host bytes, buffer lifetime
def test_no_host_copy_and_no_buffer_left_behind(tm, torch, big_stepped):
    sim, L = big_stepped, big_stepped._L
    sim.sort_particles_and_populate_grid()
    sim.rasterize_optimized()
    sim.get_grid(0)  # (the ctx's dense staging array comes with the first grid call of either kind and stays)
    n = sim.get_num_particles()
    dest = _dest(torch, n)
    grid = torch.empty((RES + 1,) * 3 + (4,), dtype=torch.float32, device="cuda")
    gc.collect()
    bytes0, live0 = L.mpmhip_host_particle_bytes(sim._ctx), int(L.mpmhip_debug_live_buffers())
    for order in (0, 1):
        assert L.mpmhip_download_dev(sim._ctx, _table(dest, FIELDS), n, order) == n
        assert (L.mpmhip_host_particle_bytes(sim._ctx), int(L.mpmhip_debug_live_buffers())) == (bytes0, live0)
    assert L.mpmhip_download_grid_dev(sim._ctx, 0, grid.data_ptr()) == 0
    assert (L.mpmhip_host_particle_bytes(sim._ctx), int(L.mpmhip_debug_live_buffers())) == (bytes0, live0)
    src = {k: dest[k][:n].contiguous() for k in ("states", "aux")}  # (what the rows hold already, id order: nothing changes)
    torch.cuda.synchronize()
    assert L.mpmhip_upload_dev(sim._ctx, _table(src, ("states", "aux")), n, 1) == 0, _error(sim)
    assert (L.mpmhip_host_particle_bytes(sim._ctx), int(L.mpmhip_debug_live_buffers())) == (bytes0, live0)


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_argument_refusals_touch_nothing(tm, torch, small_state):
    sim = _build(tm, small_state)
    L = sim._L
    n = small_state.n
    before = _host(sim)
    dest = _dest(torch, n)
    full, none = _table(dest, FIELDS), (C.c_void_p * 8)()
    cases = [(None, 0, "NULL"), (none, 0, "no field"), (none, 1, "no field"), (full, 2, "order"), (full, -1, "order")]
    for table, order, word in cases:
        assert L.mpmhip_download_dev(sim._ctx, table, n, order) == EINVAL and word in _error(sim), (order, word, _error(sim))
        assert L.mpmhip_upload_dev(sim._ctx, table, n, order) == EINVAL and word in _error(sim), (order, word, _error(sim))
    assert L.mpmhip_download_dev(None, full, n, 0) == EINVAL and L.mpmhip_upload_dev(None, full, n, 0) == EINVAL
    assert L.mpmhip_download_grid_dev(sim._ctx, 2, dest["x"].data_ptr()) == EINVAL
    assert L.mpmhip_download_grid_dev(sim._ctx, 0, None) == EINVAL
    # inside a substep (mpmhip_substep_begin ... mpmhip_substep_end work on a ctx without a partition too)
    up = _table(dest, ("x", "v"))
    assert L.mpmhip_substep_begin(sim._ctx) == 0
    assert L.mpmhip_download_dev(sim._ctx, full, n, 0) == EINVAL and "inside a substep" in _error(sim)
    assert L.mpmhip_upload_dev(sim._ctx, up, n, 1) == EINVAL and "inside a substep" in _error(sim)
    assert L.mpmhip_substep_end(sim._ctx) == 0
    sim.synchronize()
    assert all(_untouched(dest[k]) for k in FIELDS)
    after = _host(sim)  # (the substep itself ran: the particles moved, none was lost)
    assert np.array_equal(np.sort(after["id"]), before["id"]) and not _same(after["x"], before["x"])
    assert _check_download(torch, sim, 1) == n
    sim.close()


def test_a_resident_asynchronous_session_is_refused(tm, torch):
    res = 16
    sim = tm.create_simulation3("async_mpm").initialize(dict(res=(res,) * 3, delta_x=1.0 / res, unit_delta_t=2e-6, max_units=1024))
    rng = np.random.default_rng(3)
    x = ((res / 2 - 0.9 + 1.8 * rng.random((300, 3))) / res).astype(np.float32)  # the two middle cells per axis
    sim.add_particles(dict(type="elastic", positions=x, velocities=np.zeros_like(x)))
    sim.step(1e-3)
    dest = _dest(torch, 300)
    assert sim._L.mpmhip_download_dev(sim._ctx, _table(dest, FIELDS), 300, 0) == EINVAL and "asynchronous" in _error(sim)
    assert sim._L.mpmhip_upload_dev(sim._ctx, _table(dest, ("x",)), 300, 1) == EINVAL and "asynchronous" in _error(sim)
    assert all(_untouched(dest[k]) for k in FIELDS)
    sim.close()


# ------------------------------------------------------------------------------------------------ 10. the Python API
def test_python_api_tensors(tm, torch, big_stepped):
    sim = big_stepped
    for by_id in (True, False):
        ref = sim.get_particles(sort_by_id=by_id)
        n = len(ref["id"])
        t = sim.get_particle_tensors(sort_by_id=by_id)
        assert tuple(t) == FIELDS
        for k in FIELDS:
            assert t[k].device == torch.device("cuda", sim.device) and t[k].is_contiguous()
            assert t[k].dtype == (torch.int32 if k in INTS else torch.float32)
            assert tuple(t[k].shape) == ((n,) if WIDTH[k] == 1 else (n, WIDTH[k]))
            assert _same(t[k].cpu().numpy(), ref[k]), k
    ref = sim.get_particles()
    t = sim.get_particle_tensors(fields=("F", "id"))
    assert tuple(t) == ("F", "id") and _same(t["F"].cpu().numpy(), ref["F"]) and _same(t["id"].cpu().numpy(), ref["id"])
    with pytest.raises(tm.mpm.MPMError, match="'mass'"):
        sim.get_particle_tensors(fields=("x", "mass"))


def test_python_api_set_makes_strided_tensors_contiguous(tm, torch, small_state):
    a, b = _build(tm, small_state, deterministic=True), _build(tm, small_state, deterministic=True)
    n = small_state.n
    wide = torch.arange(n * 6, dtype=torch.float32, device="cuda").reshape(n, 6) * 1e-3
    v = wide[:, ::2]  # (n, 3), strided
    assert not v.is_contiguous()
    a.set_particle_tensors(dict(v=v, aux=torch.full((n, 1), 0.5, dtype=torch.float32, device="cuda")), sort_by_id=False)
    from taichi_mpm_amd.mpm import F_AUX, F_V
    b.upload(F_V, v.cpu().numpy())
    b.upload(F_AUX, np.full(n, 0.5, np.float32))
    pa, pb = _host(a), _host(b)
    assert all(_same(pa[k], pb[k]) for k in FIELDS)
    with pytest.raises(tm.mpm.MPMError, match="holds %d particles" % n):
        a.set_particle_tensors(dict(v=v[:-1].contiguous()))
    a.close()
    b.close()


@pytest.mark.parametrize("which", [0, 1])
def test_python_api_grid_tensor(tm, torch, mid_state, which):
    sim = _build(tm, mid_state)
    sim.sort_particles_and_populate_grid()
    sim.rasterize_optimized()
    if which == 1:
        sim.normalize_grid_and_apply_boundary_conditions()
    ref = sim.get_grid(which)
    g = sim.get_grid_tensor(which)
    assert g.dtype == torch.float32 and tuple(g.shape) == (RES + 1,) * 3 + (4,) and g.device == torch.device("cuda", sim.device)
    assert np.abs(ref[..., 3]).max() > 0 and _same(g.cpu().numpy(), ref)
    sim.close()


# ------------------------------------------------------------------------------------------------ 11. the example
def test_the_torch_force_field_example(tm, capsys):
    from examples import torch_force_field
    out = torch_force_field.main(frames=2, res=32)
    assert out["particles"] > 0 and len(out["mean_speed"]) == 2 and all(np.isfinite(out["mean_speed"]))
    assert out["host_particle_bytes_of_the_tensor_calls"] == 0
    text = capsys.readouterr().out
    assert "particles" in text and "mpmhip_host_particle_bytes" in text
