"""Every table the sort (csrc/k_sort.h) builds, read back through mpmhip_debug_sort_info / mpmhip_debug_sort_array and held against
the numpy model of tests/sort_model.py: slot liveness, block bitmap and prefix, active-block list, block and cell starts, the sorted
index (a permutation of the live slots, cell by cell; ascending creation id inside a cell in the deterministic mode), neighbour rows,
owner list and the chunk table of the packed G2P walk.  All integers: every comparison is exact.  The scenes (tests/sort_scenes.py)
are built for the edges of the kernels — chunk, batch and tile boundaries, the size classes of the in-cell ordering, the side array
of crowded cells, the low faces of the domain — and tests/test_sort_model_cpu.py checks without a GPU that each still reaches its edge
and that the comparator rejects the faults a subtly wrong kernel would leave."""
import ctypes as C

import numpy as np
import pytest

from tests import kernel_forms as kf
from tests import sort_model as sm
from tests import sort_scenes as sc

pytestmark = pytest.mark.gpu

DT = 1e-4
_SCENES = {}


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


def scene_of(name):
    """(scene, model of its slots in upload order), built once and never changed"""
    if name not in _SCENES:
        s = sc.SCENES[name]()
        _SCENES[name] = (s, sc.model_of(s))
    return _SCENES[name]


def make_sim(tm, scene, deterministic=True, v=None):
    """a ctx holding the scene's particles in upload order (past the Python layer's near-boundary filter, as the device has its own)"""
    sim = tm.create_simulation3("mpm").initialize(dict(res=scene["res"], delta_x=scene["dx"], base_delta_t=DT, deterministic=deterministic,
                                                       clean_boundary=scene["clean_boundary"]))
    n = len(scene["x"])
    sim._ensure_ctx(extra=n)
    vol = scene["dx"] ** 3 / 8
    params, mat = tm.mpm.group_params("jelly", 400.0 * vol, vol)
    sim._groups.append((mat, params))
    sim._check(sim._L.mpmhip_add_group(sim._ctx, mat, params.ctypes.data_as(C.POINTER(C.c_float))))
    if n:
        sim._upload_new(0, scene["x"], scene["v"] if v is None else v, None, None, None)
    sim._n_added = n
    return sim


def read_view(sim):
    info = (C.c_int64 * 16)()
    sim._check(sim._L.mpmhip_debug_sort_info(sim._ctx, info))
    view = dict(zip(sm.INFO, (int(w) for w in info)))
    for which, name in enumerate(sm.ARRAYS):
        need = -int(sim._L.mpmhip_debug_sort_array(sim._ctx, which, None, 0))
        assert need >= 0 and need % 4 == 0, (name, need)
        a = np.zeros(need // 4, np.int32 if name == "slot_id" else np.uint32)
        if need:
            assert sim._check(sim._L.mpmhip_debug_sort_array(sim._ctx, which, a.ctypes.data_as(C.c_void_p), need)) == need
        view[name] = a
    return view


def slot_model(sim, scene, view):
    """the model of the slots as the ctx holds them now: the live records come down in slot order, the view says which slots they are"""
    got = sim.get_particles(sort_by_id=False)
    live = view["slot_id"] >= 0
    assert np.array_equal(got["id"], view["slot_id"][live])
    x, v = np.zeros((len(live), 3), np.float32), np.zeros((len(live), 3), np.float32)
    x[live], v[live] = got["x"], got["v"]
    return sm.model(view["slot_id"], x, v, scene["res"], scene["dx"], scene["clean_boundary"]), got


def check_tables(sim, name, deterministic, moved=False, upload_order=False):
    """assert_tables of the last sort against the model of the slots; unless the particles `moved` since the upload also against the
    scene itself: the device deleted exactly the particles the model of the UPLOAD deletes and changed nothing else, and while the
    slots are still in `upload_order` the tables are the ones of that model"""
    scene, M0 = scene_of(name)
    view = read_view(sim)
    M, got = slot_model(sim, scene, view)
    if not moved:
        assert np.array_equal(np.sort(got["id"]), np.nonzero(M0["live"])[0])
        assert np.array_equal(got["x"], scene["x"][got["id"]])
        if upload_order:
            sm.assert_tables(view, M0, deterministic)
    sm.assert_tables(view, M, deterministic)
    if view["n_sorted"] == 0:
        assert view["act_start"].tolist() == [0] and view["cell_start"].tolist() == [0] and view["n_active"] == 0
    return view


def sort_and_check(tm, monkeypatch, name, env=None, deterministic=True, intervals=("0", None), sorts=1, expect=None):
    """the scene under the knobs `env` (and its own), once with the upload order kept in the slots (MPMHIP_REORDER_INTERVAL=0) and once with
    the default interval (physical reorder behind the first sort, k_identity_perm); `sorts` sorts, the last one checked; expect: values
    the view has to report (which form ran).  Returns the views before the last sort (None when there was one sort) and after it."""
    scene, _ = scene_of(name)
    for k, v in dict(scene["env"], **(env or {})).items():
        monkeypatch.setenv(k, v)
    out = []
    for interval in intervals:
        if interval is None:
            monkeypatch.delenv("MPMHIP_REORDER_INTERVAL", raising=False)
        else:
            monkeypatch.setenv("MPMHIP_REORDER_INTERVAL", interval)
        sim = make_sim(tm, scene, deterministic)
        before = None
        for i in range(sorts):
            if i == sorts - 1 and i > 0:
                before = read_view(sim)
            sim.sort_particles_and_populate_grid()
        view = check_tables(sim, name, deterministic, upload_order=interval == "0")
        for k, want in (expect or {}).items():
            assert view[k] == want, (k, view[k], want)
        assert view["cell_order"] == (int((env or {}).get("MPMHIP_CELL_ORDER", "1")) if deterministic else -1)
        assert view["n_slots"] == (len(scene["x"]) if interval == "0" else view["n_sorted"])
        sim.close()
        out.append((before, view))
    return out


FORMS = [(v1, walk, ct) for v1 in ("0", "1") for walk in ("2", "0") for ct in ("16", "32", "64")]


def form_env(v1, walk, ct):
    return {"MPMHIP_SORT_V1": v1, "MPMHIP_GRID_WALK": walk, "MPMHIP_CT_BLOCKS": ct}


def form_expect(v1, walk, ct):
    return {"keyed": int(v1 == "0"), "list": int(walk == "2"), "list_valid": int(walk == "2"), "ct": int(ct)}


@pytest.mark.parametrize("v1,walk,ct", FORMS)
@pytest.mark.parametrize("name", [n for n in sc.PRODUCT_SCENES if n != "hash"])
def test_every_form_of_the_sort_builds_the_model_s_tables(tm, monkeypatch, name, v1, walk, ct):
    """{keyed front, four launches} x {cell table with the owner list, plain} x {16, 32, 64 blocks per chunk}, deterministic mode"""
    for _, view in sort_and_check(tm, monkeypatch, name, form_env(v1, walk, ct), expect=form_expect(v1, walk, ct)):
        assert view["ids_cached"] == 1


@pytest.mark.parametrize("v1,walk,ct", FORMS)
def test_every_form_of_the_sort_with_the_lds_hash_ranks(tm, monkeypatch, v1, walk, ct):
    """the hash scene sorted twice: the first sort's run statistics put the second on mode 1 of rank_body (asserted from the view taken
    before it); with the upload order kept every batch of that sort holds about a thousand distinct cells"""
    env = dict(form_env(v1, walk, ct), MPMHIP_RANK_RUNS_MUL="3")
    for before, view in sort_and_check(tm, monkeypatch, "hash", env, sorts=2, expect=form_expect(v1, walk, ct)):
        assert before["rank_mode"] == 1


def test_the_hash_scene_with_the_multiplier_at_zero_ranks_by_runs(tm, monkeypatch):
    for before, view in sort_and_check(tm, monkeypatch, "hash", {"MPMHIP_RANK_RUNS_MUL": "0"}, sorts=2):
        assert before["rank_mode"] == 0 and view["rank_mode"] == 0


@pytest.mark.parametrize("v1", ["0", "1"])
def test_many_blocks_with_two_workgroups_per_scan(tm, monkeypatch, v1):
    """MPMHIP_SCAN_GRID=2: the four chunks of the block table and the chunks of the cell table are taken in later rounds of next_chunk"""
    sort_and_check(tm, monkeypatch, "many_blocks", {"MPMHIP_SCAN_GRID": "2", "MPMHIP_SORT_V1": v1}, expect={"keyed": int(v1 == "0")})


@pytest.mark.parametrize("name", sc.PRODUCT_SCENES)
def test_without_the_deterministic_mode_every_cell_holds_its_slots(tm, monkeypatch, name):
    sort_and_check(tm, monkeypatch, name, deterministic=False, sorts=2 if name == "hash" else 1)


@pytest.mark.parametrize("name", sc.PRODUCT_SCENES)
def test_the_lane_per_cell_form_of_the_ordering(tm, monkeypatch, name):
    sort_and_check(tm, monkeypatch, name, {"MPMHIP_CELL_ORDER": "0"})


@pytest.mark.parametrize("v1", ["0", "1"])
@pytest.mark.parametrize("name", ["runs", "runs_shuffled", "hash"])
def test_a_three_bit_rank_field_sends_the_crowded_cells_to_the_side_array(tm, monkeypatch, name, v1):
    sort_and_check(tm, monkeypatch, name, {"MPMHIP_TEST_SMALL_RANK": "1", "MPMHIP_SORT_V1": v1}, sorts=2 if name == "hash" else 1)


@pytest.mark.parametrize("name", ["runs", "ragged"])
def test_ordering_by_the_ids_of_the_records(tm, monkeypatch, name):
    """the COMPACT = false instantiations of the in-cell ordering: the keys come from a G2P that ran with the mode off (no cached ids),
    then the mode is switched on and the next sort has to gather the ids from the records"""
    scene, _ = scene_of(name)
    for form in ("1", "0"):
        monkeypatch.setenv("MPMHIP_CELL_ORDER", form)
        sim = make_sim(tm, scene, deterministic=False)
        sim.substep()
        sim.set_deterministic(True)
        sim.sort_particles_and_populate_grid()
        view = check_tables(sim, name, deterministic=True, moved=True)
        assert view["ids_cached"] == 0 and view["cell_order"] == int(form)
        sim.close()


def moving(scene, seed):
    """velocities that carry particles across cell, block and chunk boundaries within a few substeps — a quarter of a cell per substep
    in a random direction — and the particles of the last three cells in front of the high z wall through it, 0.7 cells per substep
    (together: a particle alone in its cells keeps its velocity, one in a crowd takes the crowd's)"""
    rng = np.random.default_rng(seed)
    n, dx = len(scene["x"]), scene["dx"]
    v = (rng.normal(0.0, 0.25, (n, 3)) * dx / DT).astype(np.float32)
    wall = scene["res"][2] - 7.0 if scene["clean_boundary"] else scene["res"][2] - 0.5
    with np.errstate(invalid="ignore"):
        v[scene["x"][:, 2] / dx > wall - 3.0] = (0.0, 0.0, 0.7 * dx / DT)
    bad = ~np.isfinite(scene["v"])
    v[bad] = scene["v"][bad]
    return v


@pytest.mark.parametrize("name", ["ragged", "many_blocks"])
def test_the_keys_and_flags_g2p_writes_sort_like_those_of_k_build_keys(tm, monkeypatch, name):
    """every sort but the first consumes the keys and block flags the last G2P wrote: three substeps, the state comes down, the sort
    runs on G2P's keys, and its tables must be the model's of that state (the model derives the keys as k_build_keys would).  Once per
    G2P walk; the packed walk reads chunk_blk of every substep's sort, and its particles must equal the per-block walk's bit for bit."""
    scene, _ = scene_of(name)
    for k, v in scene["env"].items():
        monkeypatch.setenv(k, v)
    v = moving(scene, 171)
    out = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("MPMHIP_G2P_PACKED", knob)
        sim = make_sim(tm, scene, deterministic=True, v=v)
        for _ in range(3):
            kf.assert_runs(sim, kf.packed("jelly") if knob == "1" else kf.g2p("jelly"))
            sim.substep()
        down = sim.get_particles(sort_by_id=False)
        sim.sort_particles_and_populate_grid()
        view = check_tables(sim, name, deterministic=True, moved=True)
        after = sim.get_particles(sort_by_id=False)
        for f in ("id", "x", "v"):
            assert np.array_equal(down[f], after[f]), f  # the sort moved nothing: the model above is the model of the downloaded state
        assert 0 < view["n_sorted"] < view["n_slots"]  # some left the domain in the last G2P: dead slots inside the live range
        out[knob] = sim.get_particles()
        sim.close()
    assert len(out["0"]["id"]) < sc.model_of(scene)["n_sorted"]
    for f in ("id", "x", "v", "F"):
        assert np.array_equal(out["0"][f], out["1"][f]), f


@pytest.mark.parametrize("name", ["runs", "many_blocks"])
def test_the_transfer_kernels_read_the_same_from_both_forms_of_the_sort(tm, monkeypatch, name):
    """one deterministic substep from the default form and from the four launches with the plain cell table: bit for bit"""
    scene, _ = scene_of(name)
    v = moving(scene, 181)
    out = []
    for env in ({}, {"MPMHIP_SORT_V1": "1", "MPMHIP_GRID_WALK": "0"}):
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        sim = make_sim(tm, scene, deterministic=True, v=v)
        sim.substep()
        out.append(sim.get_particles())
        sim.close()
    for f in ("id", "x", "v", "F"):
        assert np.array_equal(out[0][f], out[1][f]), f


def test_five_bits_of_rank_at_kbits_seven_without_the_test_knob(tm, monkeypatch):
    """260^3: the keyed sort's packed word keeps 5 bits of rank, so cells of 32 and more use the side array in production"""
    monkeypatch.delenv("MPMHIP_TEST_SMALL_RANK", raising=False)
    scene, _ = scene_of("side_array_real")
    sim = make_sim(tm, scene)
    sim.sort_particles_and_populate_grid()
    keyed = read_view(sim)["keyed"]
    sim.close()
    if not keyed:
        pytest.skip("the key-indexed counter table of a 260^3 grid (537 MB) did not fit in an eighth of the free device memory")
    sort_and_check(tm, monkeypatch, "side_array_real", expect={"keyed": 1, "kbits": 7})


def test_a_grid_beyond_the_keyed_block_space_takes_the_four_launches(tm, monkeypatch):
    sort_and_check(tm, monkeypatch, "big_grid", expect={"keyed": 0, "kbits": 8, "nbw": (1 << 24) // 32})


@pytest.mark.parametrize("name", ["non_cubic", "non_cubic_no_margin"])
def test_a_grid_with_three_different_axes(tm, monkeypatch, name):
    for v1 in ("0", "1"):
        sort_and_check(tm, monkeypatch, name, {"MPMHIP_SORT_V1": v1})


@pytest.mark.parametrize("name", ["empty", "one", "all_dead"])
def test_degenerate_particle_sets(tm, monkeypatch, name):
    for v1 in ("0", "1"):
        for _, view in sort_and_check(tm, monkeypatch, name, {"MPMHIP_SORT_V1": v1}):
            assert view["error"] == 0 and view["n_sorted"] == (1 if name == "one" else 0)


def test_the_view_needs_sorted_particles(tm):
    scene, _ = scene_of("one")
    sim = make_sim(tm, scene)
    info = (C.c_int64 * 16)()
    assert sim._L.mpmhip_debug_sort_info(sim._ctx, info) == -1  # MPMHIP_EINVAL
    assert sim._L.mpmhip_debug_sort_array(sim._ctx, 0, None, 0) == -1
    sim.close()
