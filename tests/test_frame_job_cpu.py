"""The frame of a tiled job, the parts that need no device: the envelope the library writes round the rows (mpmhip_bgeo_envelope)
against oracle/bgeo.py, the numpy model of the device ranking (tests/frame_rank_model.py) against np.argsort, the pure placement
tiled.assemble_frame, and the resource metadata of the kernels of csrc/k_frame.h."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import bgeo as oracle_bgeo  # noqa: E402
import frame_rank_model as model  # noqa: E402

LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    import taichi_mpm_amd as tm
    return tm.load()


def _state(n, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.random((n, 3), dtype=np.float32)
    v = rng.standard_normal((n, 3)).astype(np.float32)
    return x, v, dict(mass=rng.random(n, dtype=np.float32), debug=rng.random((n, 3), dtype=np.float32),
                      B=rng.standard_normal((n, 9)).astype(np.float32))


def _split(img, n, verbose):
    """(head, rows, tail) of an oracle image of n rows"""
    w = 4 * (23 if verbose else 12)
    empty = oracle_bgeo.encode(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.int32), verbose,
                               mass=np.zeros(0, np.float32), debug=np.zeros((0, 3), np.float32), B=np.zeros((0, 9), np.float32))
    hb = len(empty) - len(_TAIL0)  # (the header's length does not depend on n)
    return img[:hb], img[hb:hb + n * w], img[hb + n * w:]


_TAIL0 = oracle_bgeo._hstr("generator") + b"\x00\x01" + b"\x00\x00\x00\x04" + b"\x00\x00\x00\x01" + oracle_bgeo._hstr("papi") + \
    b"\x00\x00\x80\x00" + b"\x00\x00\x00\x00" + b"\x00\x00\x00\x00" + b"\x00\xff"


def _envelope(L, n, verbose):
    hb, tb = C.c_size_t(), C.c_size_t()
    assert L.mpmhip_bgeo_envelope(n, verbose, None, 0, C.byref(hb), None, 0, C.byref(tb)) == 0
    head, tail = np.zeros(hb.value, np.uint8), np.zeros(tb.value, np.uint8)
    assert L.mpmhip_bgeo_envelope(n, verbose, head.ctypes.data_as(C.c_void_p), head.size, C.byref(hb),
                                  tail.ctypes.data_as(C.c_void_p), tail.size, C.byref(tb)) == 0
    assert (hb.value, tb.value) == (head.size, tail.size)
    return head.tobytes(), tail.tobytes()


@pytest.mark.parametrize("verbose", [0, 1])
@pytest.mark.parametrize("n", [0, 1, 65536, 65537])
def test_envelope_and_the_oracles_rows_are_the_oracles_file(L, n, verbose):
    """65536 / 65537 straddle Partio's switch from uint16 to int32 point numbers (BGEO.cpp:175-180).  The rows are the oracle's own:
    only what stands round them is under test."""
    x, v, extra = _state(n)
    want = oracle_bgeo.encode(x, v, np.arange(n, dtype=np.int32), bool(verbose), **extra)
    _, rows, _ = _split(want, n, verbose)
    head, tail = _envelope(L, n, verbose)
    assert head + rows + tail == want
    assert len(tail) == len(_TAIL0) + n * (4 if n > 65536 else 2)


def test_envelope_refuses_short_buffers(L):
    hb, tb = C.c_size_t(), C.c_size_t()
    head, tail = np.full(4096, 7, np.uint8), np.full(4096, 7, np.uint8)
    rc = L.mpmhip_bgeo_envelope(1000, 0, head.ctypes.data_as(C.c_void_p), head.size, C.byref(hb), tail.ctypes.data_as(C.c_void_p), 100, C.byref(tb))
    assert rc == -4 and (head == 7).all() and (tail == 7).all()  # MPMHIP_ECAPACITY, nothing written
    assert tb.value > 2000


# ------------------------------------------------------------------------------------------------------------- the ranking model
def _sparse(n):
    return (np.arange(n, dtype=np.int64) * 4001) % 2000003  # the id set of test_bgeo_sparse_ids_take_the_sort_path


def _deal(ids, ranks, seed):
    """the ids dealt to `ranks` ranks at random, each rank's in shuffled slot order"""
    rng = np.random.default_rng(seed)
    owner = rng.integers(0, ranks, len(ids))
    return [rng.permutation(ids[owner == r]) for r in range(ranks)]


def _check_against_argsort(rank_ids):
    rows = model.job_rows(rank_ids)
    flat = np.concatenate([np.asarray(i, np.int64)[np.asarray(i, np.int64) >= 0] for i in rank_ids]) if rank_ids else np.zeros(0, np.int64)
    got = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    want = np.empty(len(flat), np.int64)
    want[np.argsort(flat, kind="stable")] = np.arange(len(flat))
    assert np.array_equal(got.astype(np.int64), want)


@pytest.mark.parametrize("ranks", [1, 2, 3, 5, 8])
def test_model_ranks_disjoint_id_sets_like_argsort(ranks):
    ids = np.random.default_rng(ranks).permutation(5000)[:3000].astype(np.int64)
    _check_against_argsort(_deal(ids, ranks, 10 + ranks))


def test_model_at_the_word_edges():
    _check_against_argsort([np.array([0, 31, 32, 63])])
    _check_against_argsort([np.array([63, 0]), np.array([32, 31])])
    _check_against_argsort([np.array([31]), np.array([32])])
    _check_against_argsort([np.arange(32, 64)[::-1], np.arange(0, 32)])  # one rank fills one word, the other the neighbouring word


def test_model_sparse_ids_dead_slots_an_empty_rank_and_a_single_id():
    _check_against_argsort(_deal(_sparse(3000), 2, 1))
    _check_against_argsort([np.array([5, -1, 2, -1]), np.array([-1, 9])])
    _check_against_argsort([np.array([4, 1, 7]), np.zeros(0, np.int64), np.array([3])])
    _check_against_argsort([np.array([77])])
    _check_against_argsort([np.zeros(0, np.int64)])
    assert model.live_id_top([-1, -1]) == 0 and model.live_id_top([6, -1]) == 7


def test_model_sees_an_id_held_twice():
    with pytest.raises(AssertionError):
        model.job_rows([np.array([1, 2]), np.array([2, 3])])


# ------------------------------------------------------------------------------------------------------------- assemble_frame
def _oracle_parts(rank_ids, verbose, seed=5):
    """an oracle file of all ids, and per rank (the model's row numbers, that rank's rows cut from the oracle's file)"""
    flat = np.concatenate(rank_ids)
    n = len(flat)
    x, v, extra = _state(n, seed)
    want = oracle_bgeo.encode(x, v, flat.astype(np.int32), bool(verbose), **extra)
    head, rows, tail = _split(want, n, verbose)
    w = 4 * (23 if verbose else 12)
    rows = np.frombuffer(rows, np.uint8).reshape(n, w)
    parts = []
    for ids, idx in zip(rank_ids, model.job_rows(rank_ids)):
        parts.append((idx.astype(np.uint32), rows[idx.astype(np.int64)].copy()))  # "fake" rows: whatever belongs at that row number
    return want, head, tail, parts, w


@pytest.mark.parametrize("verbose", [0, 1])
def test_assemble_frame_rebuilds_the_oracles_file(verbose):
    from taichi_mpm_amd import tiled
    rank_ids = _deal(_sparse(2000), 3, 2) + [np.zeros(0, np.int64)]
    want, head, tail, parts, w = _oracle_parts(rank_ids, verbose)
    assert tiled.assemble_frame(head, tail, parts, w) == want
    assert tiled.assemble_frame(head, tail, [(i, r.tobytes()) for i, r in parts], w) == want  # rows as bytes
    assert tiled.assemble_frame(b"h", b"t", [], w) == b"ht"


def test_assemble_frame_refuses_a_duplicate_and_a_gap():
    from taichi_mpm_amd import tiled
    from taichi_mpm_amd.mpm import MPMError
    rank_ids = _deal(np.arange(100, dtype=np.int64) * 3, 2, 4)
    _, head, tail, parts, w = _oracle_parts(rank_ids, 0)
    dup = [(parts[0][0].copy(), parts[0][1]), parts[1]]
    dup[0][0][0] = parts[1][0][0]  # a row number of the other rank: taken twice (and the first rank's own one left out)
    with pytest.raises(MPMError):
        tiled.assemble_frame(head, tail, dup, w)
    same = [(parts[0][0].copy(), parts[0][1]), parts[1]]
    same[0][0][1] = same[0][0][0]  # twice within one part
    with pytest.raises(MPMError):
        tiled.assemble_frame(head, tail, same, w)
    gap = [(parts[0][0].copy(), parts[0][1]), parts[1]]
    gap[0][0][0] = 100  # 100 rows numbered 0 .. 99: number 100 leaves one of them out
    with pytest.raises(MPMError):
        tiled.assemble_frame(head, tail, gap, w)
    with pytest.raises(MPMError):
        tiled.assemble_frame(head, tail, [(parts[0][0], parts[0][1][:-1])] + parts[1:], w)  # rows and numbers disagree


# ------------------------------------------------------------------------------------------------------------- kernel resources
FRAME_KERNELS = ["_ZN3mpm13k_live_id_top", "_ZN3mpm9k_id_mark", "_ZN3mpm16k_id_prefix_sums", "_ZN3mpm16k_id_prefix_scan",
                 "_ZN3mpm15k_id_prefix_add", "_ZN3mpm18k_bgeo_rows_rankedILb0EEE", "_ZN3mpm18k_bgeo_rows_rankedILb1EEE"]


@pytest.fixture(scope="module")
def stats(L):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    from taichi_mpm_amd import _lib
    import kernel_diff
    return kernel_diff.kernel_stats(_lib.build())


@pytest.mark.parametrize("prefix", FRAME_KERNELS)
def test_frame_kernels_use_no_scratch(stats, prefix):
    """k_live_id_top, k_id_mark, k_id_prefix (its three launches) and k_bgeo_rows_ranked, plain and verbose: no scratch, no spill —
    from the code object's resource metadata (DESIGN.md section 5 records the register counts)"""
    hits = {k: v for k, v in stats.items() if k.startswith(prefix)}
    assert len(hits) == 1, (prefix, sorted(hits))
    s = next(iter(hits.values()))
    assert s["vgpr_spill"] == 0 and s["sgpr_spill"] == 0 and s["scratch_bytes"] == 0, s
    print(prefix, s)
