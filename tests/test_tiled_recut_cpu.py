"""The host-only rules of re-cutting a running job (taichi_mpm_amd/csrc/tiled_plan.h: balanced_cuts, round_quotas, rounds_needed,
capacity_check) compiled for the host by g++, the header alone (tests/cpp/tiled_recut_host.cpp): tplan::balanced_cuts is held against
tiled.balanced_cuts cut for cut on seeded random histograms, the round rule's invariants are checked round by round on random tables,
the capacity rule on tables written out by hand.  The same source, with its main(), runs once as a program of its own under
AddressSanitizer and UBSan.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from taichi_mpm_amd import tiled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tiled_recut_host.cpp")
HDRS = [os.path.join(ROOT, "taichi_mpm_amd", "csrc", "tiled_plan.h"), os.path.join(ROOT, "include", "mpmhip.h")]
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "libtiled_recut_host.so")
SAN = os.path.join(ROOT, "tests", "cpp", "_build", "tiled_recut_host_san")
I64, U32 = C.POINTER(C.c_int64), C.POINTER(C.c_uint32)


def _stale(out):
    return not os.path.exists(out) or max(os.path.getmtime(f) for f in [SRC] + HDRS) > os.path.getmtime(out)


def host_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if _stale(OUT):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", SRC, "-o", OUT])
    lib = C.CDLL(OUT)
    lib.tr_balanced_cuts.argtypes = [C.c_int, C.c_int, I64, C.POINTER(C.c_int)]
    lib.tr_balanced_cuts.restype = None
    lib.tr_round_quotas.argtypes = [C.c_int, I64, U32, I64]
    lib.tr_round_quotas.restype = C.c_int64
    lib.tr_rounds_needed.argtypes = [C.c_int, I64, U32]
    lib.tr_rounds_needed.restype = C.c_int64
    lib.tr_capacity.argtypes = [C.c_int, I64, I64, I64, I64]
    lib.tr_capacity.restype = None
    lib.tr_live_after.argtypes = [C.c_int, I64, I64, C.c_int]
    lib.tr_live_after.restype = C.c_int64
    return lib


def host_cuts(lib, res, parts, hist):
    h = np.ascontiguousarray(hist, np.int64)
    out = (C.c_int * (parts + 1))()
    lib.tr_balanced_cuts(res, parts, h.ctypes.data_as(I64), out)
    return list(out)


def draw_histogram(rng, kind, res):
    h = np.zeros(res, np.int64)
    if kind == "single":
        h[rng.randint(res)] = rng.randint(1, 100000)
    elif kind == "last":
        h[res - 1] = rng.randint(1, 100000)
    elif kind == "clusters":  # clusters separated by empty stretches
        for _ in range(rng.randint(1, 6)):
            a, w = rng.randint(res), rng.randint(1, 24)
            h[a:a + w] += rng.randint(1, 1000, size=len(h[a:a + w]))
    elif kind == "dense":
        h[:] = rng.randint(0, 50, size=res)
    elif kind == "heavy":  # counts of a large job: the integer comparison must not lose bits
        h[:] = rng.randint(0, 1 << 28, size=res)
    return h


KINDS = ["empty", "single", "last", "clusters", "dense", "heavy"]


def test_the_test_library_does_not_pull_in_the_hip_runtime():
    host_lib()
    needed = subprocess.check_output(["readelf", "-d", OUT], text=True)
    assert "amdhip64" not in needed and "libhsa" not in needed, needed


def test_balanced_cuts_equal_the_python_model_cut_for_cut():
    """2 400 histograms: every kind x parts 1 .. 16 x 25 draws of res in [parts, 512] (res = parts and res = 512 among them)"""
    lib, rng, n = host_lib(), np.random.RandomState(20), 0
    for kind in KINDS:
        for parts in range(1, 17):
            for i in range(25):
                res = parts if i == 0 else (512 if i == 1 else int(rng.randint(parts, 513)))
                h = draw_histogram(rng, kind, res)
                want = [int(c) for c in tiled.balanced_cuts(None, res, parts, hist=h)]
                got = host_cuts(lib, res, parts, h)
                assert got == want, (kind, parts, res, h.tolist(), got, want)
                n += 1
    assert n >= 2000


def test_round_rule_on_random_tables():
    """world 2 .. 16, inbox room 1 .. 10^4, counts 0 .. 10^5.  Every round: the quotas of a destination fit its room, a quota is at
    most what is left, sources are served in ascending rank order (a source that is cut short fills the inbox, and nobody behind it
    is served), every "rank" fed the same table gets the same quotas; nothing is left at the end, and the rounds stay within
    max over dst of ceil(arrivals(dst) / room(dst)) and equal what rounds_needed predicted."""
    lib, rng = host_lib(), np.random.RandomState(21)
    for it in range(120):
        world = int(rng.randint(2, 17))
        # the whole ranges, table by table at a scale that keeps the rounds of one table in the hundreds: counts up to 10 / 10^3 /
        # 10^5 against rooms from 1 / 6 / 600 x world up to 10^4 (the stand-alone program walks tables without that coupling)
        top = (10, 1000, 100000)[it % 3]
        room = rng.randint(max(1, top * world // 160), 10001, size=world).astype(np.uint32)
        left = rng.randint(0, top + 1, size=(world, world)).astype(np.int64)
        left[rng.rand(world, world) < 0.3] = 0
        np.fill_diagonal(left, 0)
        arrivals = left.sum(0)
        bound = int(max(-(-int(a) // int(r)) for a, r in zip(arrivals, room)))
        predicted = int(lib.tr_rounds_needed(world, left.ctypes.data_as(I64), room.ctypes.data_as(U32)))
        rounds = 0
        while left.sum():
            q = [np.zeros((world, world), np.int64) for _ in range(3)]  # the rule as three "ranks" evaluate it
            for r in range(3):
                moved = int(lib.tr_round_quotas(world, left.ctypes.data_as(I64), room.ctypes.data_as(U32), q[r].ctypes.data_as(I64)))
                assert moved == q[r].sum() > 0
                assert np.array_equal(q[r], q[0])
            q = q[0]
            assert (q >= 0).all() and (q <= left).all()
            assert (q.sum(0) <= room).all()
            for dst in range(world):
                short = np.nonzero(q[:, dst] < left[:, dst])[0]
                if len(short):
                    assert q[:, dst].sum() == room[dst] and (q[short[0] + 1:, dst] == 0).all()
            assert ((q.sum(0) > 0) | (left.sum(0) == 0)).all()  # every destination that expects records gets at least one
            left = np.ascontiguousarray(left - q)
            rounds += 1
            assert rounds <= bound
        assert rounds == predicted


def test_capacity_rule_on_hand_made_tables():
    lib = host_lib()
    # 3 ranks: 0 sends 40 to 1 and 10 to 2, 1 sends 5 to 0: the live counts 100, 50, 20 become 55, 85, 30
    counts = np.array([[0, 40, 10], [5, 0, 0], [0, 0, 0]], np.int64)
    live = np.array([100, 50, 20], np.int64)
    assert [int(lib.tr_live_after(3, counts.ctypes.data_as(I64), live.ctypes.data_as(I64), r)) for r in range(3)] == [55, 85, 30]

    def check(cap):
        cap, out = np.asarray(cap, np.int64), (C.c_int64 * 3)()
        lib.tr_capacity(3, counts.ctypes.data_as(I64), live.ctypes.data_as(I64), cap.ctypes.data_as(I64), out)
        return list(out)
    assert check([55, 85, 30])[0] == -1            # every rank exactly full: fits
    assert check([100, 84, 64]) == [1, 85, 1]      # rank 1 one short
    assert check([100, 60, 25]) == [1, 85, 25]     # two ranks too small: the first is reported, with its own excess
    assert check([54, 85, 30]) == [0, 55, 1]       # a rank that shrinks but not enough
    # 2 ranks that swap everything: nobody grows
    swap, two = np.array([[0, 7], [9, 0]], np.int64), np.array([7, 9], np.int64)
    out = (C.c_int64 * 3)()
    lib.tr_capacity(2, swap.ctypes.data_as(I64), two.ctypes.data_as(I64), np.array([9, 7], np.int64).ctypes.data_as(I64), out)
    assert out[0] == -1
    lib.tr_capacity(2, swap.ctypes.data_as(I64), two.ctypes.data_as(I64), np.array([8, 7], np.int64).ctypes.data_as(I64), out)
    assert list(out) == [0, 9, 1]


def test_every_scenario_under_the_sanitizers():
    """the same source as a stand-alone program (its main() runs the scenarios on its own seeded inputs) built with
    -fsanitize=address,undefined; the runtime is linked statically, so nothing has to be preloaded"""
    os.makedirs(os.path.dirname(SAN), exist_ok=True)
    if _stale(SAN):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-static-libubsan", SRC, "-o", SAN])
    r = subprocess.run([SAN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "scenarios ok" in r.stdout, r.stdout
