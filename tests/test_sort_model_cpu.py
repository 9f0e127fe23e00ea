"""The numpy model of the sort's tables (tests/sort_model.py) and the scenes of tests/test_gpu_sort_tables.py, checked without a GPU:
the model against a second, dumb derivation (np.lexsort and dictionary walks) on every scene; the comparator against planted faults,
one at a time — each is what a subtly wrong kernel of csrc/k_sort.h would leave; and every scene against the edge it exists for."""
import numpy as np
import pytest

from tests import sort_model as sm
from tests import sort_scenes as sc

_CACHE = {}


def case(name):
    """(scene, model, the dumb derivation's view) of a scene, computed once and never changed: the tests work on copies"""
    if name not in _CACHE:
        s = sc.SCENES[name]()
        _CACHE[name] = (s, sc.model_of(s), sm.brute_view(np.arange(len(s["x"])), s["x"], s["v"], s["res"], s["dx"], s["clean_boundary"]))
    return _CACHE[name]


def planted(name):
    s, M, view = case(name)
    return M, {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in view.items()}


def rejected(view, M, deterministic=True):
    with pytest.raises(AssertionError):
        sm.assert_tables(view, M, deterministic)


@pytest.mark.parametrize("name", sorted(sc.SCENES))
def test_the_model_equals_the_dumb_derivation(name):
    s, M, view = case(name)
    sm.assert_tables(view, M, deterministic=True)
    sm.assert_tables(view, M, deterministic=False)
    assert view["n_own"] == M["n_own"] and np.array_equal(view["own_list"], M["own_list"])


@pytest.mark.parametrize("name", sorted(sc.SCENES))
def test_every_scene_reaches_the_edge_it_exists_for(name):
    s, M, _ = case(name)
    s["edge"](M)
    assert M["n_active"] < len(s["x"]) // 48 + 4096  # n_active < max_blocks of a ctx created for the scene (mpmhip_create)


def test_the_key_follows_per_axis_res_and_marks_dead_slots():
    from tests.common import sort_key
    dx = 1.0 / 40
    x = (np.array([[10.2, 10.2, 10.2], [10.2, 23.6, 10.2], [10.2, 23.4, 10.2], [0.4, 10, 10], [10, 10, 51.6], [39.6, 10, 10],
                   [10.2, 17.2, 10.2], [10.2, 16.9, 10.2], [6.9, 10, 10], [np.nan, 10, 10], [10, np.inf, 10], [10, 10, 10]]) * dx).astype(np.float32)
    v = np.zeros_like(x)
    v[11, 2] = -np.inf
    ids = np.arange(len(x))
    k0 = sort_key(x, dx, res=(40, 24, 52), v=v, ids=ids, clean_boundary=False)
    assert (k0 >= 0).tolist() == [True, False, True, False, False, False, True, True, True, False, False, False]
    k1 = sort_key(x, dx, res=(40, 24, 52), v=v, ids=ids, clean_boundary=True)
    assert (k1 >= 0).tolist() == [True, False, False, False, False, False, False, True, False, False, False, False]
    ids[0] = -1
    assert sort_key(x, dx, res=(40, 24, 52), v=v, ids=ids)[0] == -1
    # the bit layout is the one of the two-argument form the older tests use
    assert np.array_equal(k0[[0, 2, 6]], sort_key(x[[0, 2, 6]], dx))
    assert k0[0] == (sm.morton3(*np.array([[2], [2], [2]]))[0] << 6 | (1 << 4) | (1 << 2) | 1)


# ---------------------------------------------------------------------------------------------------------- planted faults
def test_swap_across_a_cell_boundary_is_rejected():
    M, view = planted("runs")
    j = int(M["cell_start"][np.nonzero(M["counts"])[0][3]])  # the first entry of some cell and the last of the cell before
    view["perm"][[j - 1, j]] = view["perm"][[j, j - 1]]
    rejected(view, M, deterministic=False)


def test_swap_inside_a_cell_is_rejected_in_the_deterministic_mode_only():
    M, view = planted("runs")
    c = int(np.nonzero(M["counts"] == 17)[0][0])
    j = int(M["cell_start"][c])
    view["perm"][[j + 3, j + 4]] = view["perm"][[j + 4, j + 3]]
    sm.assert_tables(view, M, deterministic=False)
    rejected(view, M, deterministic=True)


@pytest.mark.parametrize("ct", [16, 32, 64])
def test_cell_start_off_by_one_from_the_second_scan_chunk_is_rejected(ct):
    M, view = planted("many_blocks")
    assert M["n_active"] > ct
    view["cell_start"][64 * ct:] += 1
    rejected(view, M)
    M, view = planted("many_blocks")
    view["act_start"][ct:] += 1
    rejected(view, M)


def test_wprefix_short_by_the_first_chunk_of_the_block_table_is_rejected():
    M, view = planted("many_blocks")
    first = int(M["wprefix"][256])  # active blocks of the words 0..255
    assert first > 0
    view["wprefix"][256] -= first
    rejected(view, M)


def test_a_dropped_and_a_duplicated_owner_entry_are_rejected():
    M, view = planted("many_blocks")
    view["own_list"] = np.delete(view["own_list"], 100)
    rejected(view, M)
    M, view = planted("many_blocks")
    view["own_list"] = np.insert(view["own_list"], 100, view["own_list"][100])
    rejected(view, M)
    M, view = planted("many_blocks")  # ... also with the count adjusted to the faulty list
    view["own_list"] = np.insert(view["own_list"], 100, view["own_list"][100])
    view["n_own"] += 1
    rejected(view, M)


def test_slot_zero_for_a_neighbour_outside_the_domain_is_rejected():
    M, view = planted("many_blocks")
    bx, _, _ = sm.demorton3(M["act_blk"])
    a = int(np.nonzero(bx == 0)[0][5])
    row = view["nbr"].reshape(-1, 32)
    assert row[a, 4] == sm.INVALID  # the neighbour at (-1, 0, 0)
    row[a, 4] = 0
    rejected(view, M)


def test_chunk_blk_naming_the_block_before_is_rejected():
    M, view = planted("runs")
    k = [k for k in range(1, len(M["chunk_blk"])) if 256 * k in M["act_start"]]
    assert k, "no block of the scene starts at a multiple of 256"
    view["chunk_blk"][k[0]] -= 1
    rejected(view, M)


def test_a_dead_slot_in_perm_is_rejected():
    M, view = planted("ragged")
    dead = int(np.nonzero(~M["live"])[0][7])
    view["perm"][123] = dead
    rejected(view, M, deterministic=False)
    M, view = planted("ragged")  # ... appended behind the live range
    view["perm"] = np.append(view["perm"], dead)
    rejected(view, M, deterministic=False)


def test_a_slot_wrongly_deleted_is_rejected():
    M, view = planted("ragged")
    view["slot_id"][int(np.nonzero(M["live"])[0][9])] = -1
    rejected(view, M)
