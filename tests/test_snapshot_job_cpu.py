"""The snapshot of a tiled job without a GPU: the numpy model (tests/snapshot_job_model.py) against brute force on small random blobs,
tiled.assemble_snapshot and tiled.snapshot_head_differs against the model, the ctypes prototypes of the new entry points, the
host-only addition to csrc/snapshot_blob.h (check3d_brick) as a stand-alone program under AddressSanitizer and UBSan, and the resource
budget of the new kernels read from the built code object."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import snapshot_job_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
LLVM = "/opt/rocm/lib/llvm/bin"
CSRC = os.path.join(ROOT, "taichi_mpm_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "snapshot_job_host.cpp")
SAN = os.path.join(ROOT, "tests", "cpp", "_build", "snapshot_job_host_san")
RES, DX = 16, 1.0 / 16


def _header(n_groups, n_slots, next_pid, n_dead, substeps=3, store_b=1, b_stale=0, t=3e-4, dt=1e-4):
    from taichi_mpm_amd import _lib
    h = _lib.SnapHeader()
    h.magic, h.abi, h.n_groups, h.n_slots, h.substeps, h.next_pid = b"MPMHIP01", 3, n_groups, n_slots, substeps, next_pid
    h.b_stale, h.store_b, h.t, h.request_t, h.dx, h.dt, h.n_dead = b_stale, store_b, t, t, DX, dt, n_dead
    h.res[:] = (RES, RES, RES)
    return h


def _groups(n):
    from taichi_mpm_amd import _lib
    rows = (_lib.GroupParams * n)()
    for g in range(n):
        rows[g].type, rows[g].p[0] = 1 + g, 1.0 + g
    return bytes(rows)


def _random_blob(seed, n, dead=0.25, special=True):
    """a one-ctx blob of n slots: random record bytes, ids in no order (a share of them dead), positions inside cells 2 .. 13;
    with `special` slot 0 exactly on the cut plane x = 8 cells, slot 1 below half a cell, slot 2 NaN (all three live)"""
    rng = np.random.RandomState(seed)
    rg = rng.randint(0, 256, (n, 64)).astype(np.uint8)
    rp = rng.randint(0, 256, (n, 64)).astype(np.uint8)
    rb = rng.randint(0, 256, (n, 48)).astype(np.uint8)
    x = ((2 + rng.rand(n, 3) * 11) * DX).astype(np.float32)
    ids = rng.permutation(n * 3)[:n].astype(np.int32)
    ids[rng.rand(n) < dead] = -1
    if special and n >= 3:
        x[0] = (np.float32(8.5) * np.float32(DX), 0.5, 0.5)
        x[1] = (0.5, np.float32(0.4) * np.float32(DX), 0.5)
        x[2] = (0.5, 0.5, np.nan)
        ids[:3] = (n * 3, n * 3 + 1, n * 3 + 2)
    rg[:, :12] = x.view(np.uint8).reshape(n, 12)
    rg[:, 52:56] = rng.randint(0, 2, n).astype(np.uint32).view(np.uint8).reshape(n, 4)
    rg[:, 56:60] = ids.view(np.uint8).reshape(n, 4)
    h = _header(2, n, int(max(ids.max() + 1, 0)) if n else 0, int((ids < 0).sum()))
    return bytes(h) + _groups(2) + rg.tobytes() + rp.tobytes() + rb.tobytes(), x, ids


# ------------------------------------------------------------------------------------------------ the model against brute force
@pytest.mark.parametrize("seed,n", [(1, 0), (2, 1), (3, 40), (4, 257)])
def test_canonical_against_brute_force(seed, n):
    blob, x, ids = _random_blob(seed, n)
    got = model.canonical(blob)
    p, q = model.parse(blob), model.parse(got)
    live = sorted((int(i), s) for s, i in enumerate(ids) if i >= 0)  # brute force: a Python sort of (id, slot)
    assert len(q["rg"]) == len(live) and q["groups"] == p["groups"] and q["tail"] == b""
    for row, (i, s) in enumerate(live):
        assert q["rg"][row].tobytes() == p["rg"][s].tobytes() and q["rp"][row].tobytes() == p["rp"][s].tobytes()
        assert q["rb"][row].tobytes() == p["rb"][s].tobytes()
    h = q["head"]
    assert model.head_field(h, model.H_NSLOTS, np.int64) == len(live) and model.head_field(h, model.H_NDEAD, np.uint32) == 0
    assert model.head_field(h, model.H_NEXT_PID, np.int32) == max(model.head_field(p["head"], model.H_NEXT_PID, np.int32),
                                                                  live[-1][0] + 1 if live else 0)
    keep = np.ones(80, bool)
    keep[16:24] = keep[32:36] = keep[72:76] = False  # every other header byte is the blob's
    assert np.array_equal(h[keep], p["head"][keep])
    assert model.canonical(got) == got  # a canonical blob is its own canonical form


def test_canonical_raises_next_pid_above_a_migrated_id():
    blob, x, ids = _random_blob(5, 30, special=False)
    b = bytearray(blob)
    b[model.H_NEXT_PID:model.H_NEXT_PID + 4] = np.array([1], np.int32).tobytes()  # a rank that handed out one id and received the others
    got = model.parse(model.canonical(bytes(b)))
    assert model.head_field(got["head"], model.H_NEXT_PID, np.int32) == ids.max() + 1


@pytest.mark.parametrize("seed,n", [(6, 3), (7, 64), (8, 300)])
def test_owned_against_brute_force(seed, n):
    from taichi_mpm_amd import tiled
    blob, x, ids = _random_blob(seed, n)
    part = tiled.Partition((RES,) * 3, (2, 2, 1), [[0, 8, RES], [0, 7, RES], [0, RES]], 2)
    got = [model.owned(blob, part, r, DX) for r in range(4)]
    want = [[] for _ in range(4)]
    lost = 0
    for s in range(n):  # brute force: one slot at a time, the cuts walked by hand
        if ids[s] < 0:
            continue
        X = [np.float32(x[s, a]) * np.float32(1.0 / DX) for a in range(3)]
        if not all(np.isfinite(v) and v >= np.float32(0.5) for v in X):
            lost += 1
            continue
        b = [int(v - np.float32(0.5)) for v in X]
        px = 0 if b[0] < 8 else 1
        py = 0 if b[1] < 7 else 1
        want[px * 2 + py].append(s)
    assert [list(g) for g in got] == want
    assert lost == 2 and 0 in want[2] + want[3]  # the two unplaceable records are nobody's; the one ON the plane x = 8 belongs above it
    assert int(model.placeable(blob, DX).sum()) == sum(len(w) for w in want) == int((ids >= 0).sum()) - lost


def test_assemble_against_canonical_and_the_library_function():
    from taichi_mpm_amd import tiled
    blob, x, ids = _random_blob(9, 200, special=False)
    part = tiled.Partition((RES,) * 3, (3, 1, 1), [[0, 6, 9, RES], [0, RES], [0, RES]], 2)
    p = model.parse(blob)
    all_ids, all_rows = model.rows_of(blob)
    slot_of = np.nonzero(ids >= 0)[0]
    rank_of_slot = np.full(len(ids), -1)
    for r in range(3):
        rank_of_slot[model.owned(blob, part, r, DX)] = r
    sel = [rank_of_slot[slot_of] == r for r in range(3)]
    numbers = model.job_row_numbers([all_ids[m] for m in sel])
    parts = [(numbers[r], all_rows[sel[r]]) for r in range(3)]
    head = p["head"].tobytes()
    want = model.canonical(blob)
    assert model.assemble(head, p["groups"], parts) == want
    assert tiled.assemble_snapshot(head, p["groups"], parts) == want
    assert tiled.assemble_snapshot(head, p["groups"], [(i, r.tobytes()) for i, r in parts][::-1]) == want  # any order of the parts, rows as bytes
    # no particle at all
    empty = tiled.assemble_snapshot(head, p["groups"], [(np.zeros(0, np.uint32), np.zeros((0, 176), np.uint8))] * 2)
    assert empty == model.assemble(head, p["groups"], [(np.zeros(0), np.zeros((0, 176), np.uint8))]) and len(empty) == 80 + len(p["groups"])


def test_assemble_snapshot_refuses_a_number_taken_twice_or_left_out():
    from taichi_mpm_amd import tiled
    from taichi_mpm_amd.mpm import MPMError
    head, groups = bytes(_header(2, 0, 0, 0)), _groups(2)
    rows = np.zeros((3, 176), np.uint8)
    with pytest.raises(MPMError, match="two records at one row number"):
        tiled.assemble_snapshot(head, groups, [(np.array([0, 1, 1]), rows)])
    with pytest.raises(MPMError, match="two records at one row number"):
        tiled.assemble_snapshot(head, groups, [(np.array([0, 1, 2]), rows), (np.array([1]), rows[:1])])
    with pytest.raises(MPMError, match="left out"):
        tiled.assemble_snapshot(head, groups, [(np.array([0, 1, 3]), rows)])
    with pytest.raises(MPMError, match="row numbers and"):
        tiled.assemble_snapshot(head, groups, [(np.array([0, 1]), rows)])
    with pytest.raises(MPMError, match="head of"):
        tiled.assemble_snapshot(head[:-1], groups, [])
    with pytest.raises(ValueError):
        model.assemble(head, groups, [(np.array([0, 1, 1]), rows)])


def test_snapshot_head_differs_names_the_field():
    from taichi_mpm_amd import tiled
    g = _groups(2)
    a = bytes(_header(2, 10, 5, 0)) + g
    assert tiled.snapshot_head_differs(a, bytes(_header(2, 99, 77, 0)) + g) is None  # (slot counts and next ids are each rank's own)
    for name, kw in (("substeps", dict(substeps=4)), ("t", dict(t=4e-4)), ("dt", dict(dt=2e-4)), ("store_b", dict(store_b=0)),
                     ("b_stale", dict(b_stale=1))):
        assert tiled.snapshot_head_differs(a, bytes(_header(2, 10, 5, 0, **kw)) + g) == name
    other = _header(2, 10, 5, 0)
    other.res[2] = 2 * RES
    assert tiled.snapshot_head_differs(a, bytes(other) + g) == "res"
    assert tiled.snapshot_head_differs(a, bytes(_header(2, 10, 5, 0)) + _groups(3)) == "group table"
    assert tiled.snapshot_head_differs(a, bytes(_header(2, 10, 5, 0)) + g[:-1] + b"\x07") == "group table"


# ------------------------------------------------------------------------------------------------ prototypes
def test_ctypes_prototypes_of_the_new_entry_points():
    from taichi_mpm_amd import _lib
    L = _lib.load()
    vp, P = C.c_void_p, C.POINTER
    want = {
        "mpmhip_snapshot_size_group": [P(vp), C.c_int32, P(C.c_size_t)],
        "mpmhip_snapshot_save_group": [P(vp), C.c_int32, vp, C.c_size_t, P(C.c_size_t)],
        "mpmhip_snapshot_head": [vp, vp, C.c_size_t, P(C.c_size_t)],
        "mpmhip_snapshot_rows_ranked": [vp, C.c_int64, vp, vp, vp, C.c_int64, P(C.c_int64)],
        "mpmhip_snapshot_load_brick": [vp, vp, C.c_size_t, P(C.c_int64)],
        "mpmhip_snapshot_histogram": [vp, vp, C.c_size_t, P(C.c_int64), P(C.c_int64), P(C.c_int64), P(C.c_int32), P(C.c_int32), P(C.c_int64)],
    }
    for name, argtypes in want.items():
        assert name in _lib.exported_symbols()
        assert list(getattr(L, name).argtypes) == argtypes, name
    assert L.mpmhip_abi_version() == 3  # the format is MPMHIP01 unchanged
    # null arguments are refused before anything is touched (no GPU is needed to say so)
    n = C.c_size_t()
    assert L.mpmhip_snapshot_size_group(None, 1, C.byref(n)) == -1 and L.mpmhip_snapshot_save_group(None, 0, None, 0, None) == -1
    assert L.mpmhip_snapshot_load_brick(None, None, 0, None) == -1 and L.mpmhip_snapshot_histogram(None, None, 0, None, None, None, None, None, None) == -1
    assert L.mpmhip_snapshot_head(None, None, 0, None) == -1 and L.mpmhip_snapshot_rows_ranked(None, 0, None, None, None, 0, None) == -1


# ------------------------------------------------------------------------------------------------ check3d_brick on the host
def test_check3d_brick_under_the_sanitizers():
    """tests/cpp/snapshot_job_host.cpp as a stand-alone program built with -fsanitize=address,undefined; the runtime is linked
    statically, so nothing has to be preloaded"""
    hdrs = [os.path.join(CSRC, h) for h in ("snapshot_blob.h", "async_sched.h", "group_params.h")] + [os.path.join(ROOT, "include", "mpmhip.h"), SRC]
    os.makedirs(os.path.dirname(SAN), exist_ok=True)
    if not os.path.exists(SAN) or max(os.path.getmtime(f) for f in hdrs) > os.path.getmtime(SAN):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-static-libubsan", SRC, "-o", SAN])
    r = subprocess.run([SAN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "scenarios ok" in r.stdout, r.stdout


# ------------------------------------------------------------------------------------------------ the kernels' budget
# mangled name -> (max VGPRs + AGPRs, max instructions, max static LDS bytes).  64 registers = eight waves per SIMD, the re-cut
# kernels' bar.  Static LDS: k_snap_own_count 4 x 3 count words + the 4 x 6 bound words of bounds_epilogue = 144 bytes,
# k_snap_own_emit its 4 wave sums, k_snap_rows_ranked none.  Instruction ceilings: the first working build's counts (262, 1071, 571:
# DESIGN.md section 5) plus a quarter.
BUDGET = {
    "_ZN3mpm18k_snap_rows_ranked": (64, 330, 0),
    "_ZN3mpm16k_snap_own_count": (64, 1340, 144),
    "_ZN3mpm15k_snap_own_emit": (64, 715, 16),
}


@pytest.fixture(scope="module")
def stats():
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    import kernel_diff
    from taichi_mpm_amd import _lib
    return kernel_diff.kernel_stats(_lib.build())


@pytest.mark.parametrize("prefix", sorted(BUDGET))
def test_snapshot_job_kernels_stay_inside_their_budget(stats, prefix):
    hits = {k: v for k, v in stats.items() if k.startswith(prefix)}
    assert len(hits) == 1, (prefix, sorted(hits))
    s = next(iter(hits.values()))
    vmax, imax, lds = BUDGET[prefix]
    assert s["vgpr_spill"] == 0 and s.get("sgpr_spill", 0) == 0 and s["scratch_bytes"] == 0, s
    assert s["vgpr"] + s.get("agpr", 0) <= vmax, s
    assert s["instructions"] <= imax, s
    assert s["lds_bytes"] <= lds, s
