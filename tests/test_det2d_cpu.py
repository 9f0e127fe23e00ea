"""Host side of the 2D solver's deterministic mode (include/mpmhip.h: mpmhip2d_config.deterministic, mpmhip2d_set_deterministic,
mpmhip2d_upload_ids).  No ctx can be created without a GPU, so this checks what the host layers promise: the config key, the struct
field, the two bound symbols — and restates the order of the cell sort in numpy (csrc/k_mpm2d_det.h: k2d_order)."""
import ctypes as C

import numpy as np

import taichi_mpm_amd as tm
from taichi_mpm_amd import _lib


def test_the_config_key_is_accepted_and_remembered():
    sim = tm.create_simulation2("mpm").initialize(dict(res=(64, 64), deterministic=True))
    assert sim.deterministic is True
    assert tm.create_simulation2("mpm").initialize(dict(res=(64, 64))).deterministic is False
    sim.set_deterministic(False)  # (no ctx yet: remembered for its creation)
    assert sim.deterministic is False


def test_config2d_carries_the_field_where_the_first_reserved_word_was():
    names = [f[0] for f in _lib.Config2D._fields_]
    assert "deterministic" in names and names.index("deterministic") == names.index("device") + 1
    assert _lib.Config2D.deterministic.offset == _lib.Config2D.device.offset + 4
    assert _lib.Config2D.reserved.size == 8  # reserved[3] became deterministic + reserved[2]: size and offsets unchanged


def test_both_new_symbols_are_bound_with_argtypes():
    assert {"mpmhip2d_set_deterministic", "mpmhip2d_upload_ids"} <= set(_lib.exported_symbols())
    import __graft_entry__ as g
    g.build()
    L = tm.load()
    assert L.mpmhip2d_set_deterministic.argtypes == [C.c_void_p, C.c_int32]
    assert L.mpmhip2d_upload_ids.argtypes == [C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]


def cell_order(key, pid):
    """the sorted index the mode builds: live slots (key >= 0) by (cell, creation id, slot)"""
    slot = np.arange(len(key))
    live = key >= 0
    o = np.lexsort((slot[live], pid[live], key[live]))
    return slot[live][o]


def test_cell_order_is_a_permutation_with_duplicate_ids_and_ignores_the_slot_order_without():
    rng = np.random.default_rng(3)
    n = 500
    key = rng.integers(0, 20, n)
    key[rng.random(n) < 0.1] = -1
    pid = rng.permutation(n)
    a = cell_order(key, pid)
    perm = rng.permutation(n)
    b = cell_order(key[perm], pid[perm])
    assert np.array_equal(pid[a], pid[perm][b])  # the same particles at the same sorted positions, whatever the slots
    dup = pid.copy()
    dup[:50] = 7  # duplicate ids: still every live slot exactly once
    c = cell_order(key, dup)
    assert np.array_equal(np.sort(c), np.flatnonzero(key >= 0))
