"""The planner of a tiled run (taichi_mpm_amd/csrc/tiled_plan.h: partition, halo plan, interior, arena, migration table, the decisions
after a migration, the schedule) compiled for the host by g++, the header alone: no HIP header is included, no HIP runtime linked or
loaded (tests/cpp/tiled_plan_host.cpp).  Plans, slack and schedule are held against the Python model (taichi_mpm_amd/tiled.py:
Partition, TiledRank.schedule) on seeded random partitions; the invariants of plans with per-rank occupancy are checked node by node;
the rest are scenarios with their numbers written out by hand.  The same source, with its main(), runs once as a program of its own
under AddressSanitizer and UBSan.  No GPU needed."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

from taichi_mpm_amd import _lib
from taichi_mpm_amd.tiled import Partition, TiledRank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tiled_plan_host.cpp")
HDRS = [os.path.join(ROOT, "taichi_mpm_amd", "csrc", "tiled_plan.h"), os.path.join(ROOT, "include", "mpmhip.h")]
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "libtiled_plan_host.so")
SAN = os.path.join(ROOT, "tests", "cpp", "_build", "tiled_plan_host_san")
SCENARIOS = ["tp_two_bricks", "tp_occupancy_cut_interior", "tp_three_in_a_row", "tp_no_interior", "tp_arena", "tp_mig_table",
             "tp_after_two_blobs", "tp_after_shrink", "tp_after_arrivals", "tp_schedule", "tp_validation"]
DIMS = [(2, 1, 1), (1, 3, 1), (2, 2, 2), (4, 2, 1), (3, 1, 3), (16, 1, 1), (4, 4, 4)]
MAX_BOXES = 64


class Spec(C.Structure):
    """mirror of Spec (tests/cpp/tiled_plan_host.cpp)"""
    _fields_ = [("res", C.c_int32 * 3), ("dims", C.c_int32 * 3), ("cuts", (C.c_int32 * (_lib.MAX_PARTS + 1)) * 3), ("margin", C.c_int32)]


def _stale(out):
    return not os.path.exists(out) or max(os.path.getmtime(f) for f in [SRC] + HDRS) > os.path.getmtime(out)


def host_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if _stale(OUT):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", SRC, "-o", OUT])
    lib = C.CDLL(OUT)
    lib.tp_validate.restype = C.c_char_p
    lib.tp_validate.argtypes = [C.POINTER(Spec), C.c_int]
    ints, u64s = C.POINTER(C.c_int), C.POINTER(C.c_uint64)
    lib.tp_plan.argtypes = [C.POINTER(Spec), ints, ints, ints, C.c_int, C.c_uint64, C.c_int, ints, u64s, u64s]
    lib.tp_invariants.argtypes = [C.POINTER(Spec), ints, ints, ints]
    lib.tp_next_interval.restype = C.c_int64
    lib.tp_next_interval.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float]
    return lib


def draw(rng):
    """a valid partition and a clip box: res per axis in [8, 96], dims from DIMS, strictly increasing cuts from 0 with the last >= res
    (cut planes may lie beyond the grid: such bricks are empty), margin 1 - 4; the clip box the whole grid or a non-empty sub-box"""
    res = [int(rng.randint(8, 97)) for _ in range(3)]
    dims = DIMS[rng.randint(len(DIMS))]
    cuts = []
    for a in range(3):
        inner = sorted(int(v) for v in rng.choice(np.arange(1, res[a] + dims[a]), size=dims[a] - 1, replace=False))
        last = max([res[a]] + [v + 1 for v in inner[-1:]]) + int(rng.randint(0, 3))
        cuts.append([0] + inner + [last])
    margin = int(rng.randint(1, 5))
    if rng.randint(2):
        clip = ([0, 0, 0], [r + 1 for r in res])
    else:
        lo = [int(rng.randint(0, r + 1)) for r in res]
        clip = (lo, [int(rng.randint(lo[a] + 1, res[a] + 2)) for a in range(3)])
    return res, dims, cuts, margin, clip


def spec_of(res, dims, cuts, margin):
    s = Spec()
    s.res[:], s.dims[:], s.margin = res, dims, margin
    for a in range(3):
        for k, v in enumerate(cuts[a]):
            s.cuts[a][k] = v
    return s


def ivec(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def test_the_test_library_does_not_pull_in_the_hip_runtime():
    host_lib()
    needed = subprocess.check_output(["readelf", "-d", OUT], text=True)
    assert "amdhip64" not in needed and "libhsa" not in needed, needed


def test_plans_equal_the_python_model_on_random_partitions():
    """240 partitions: for every rank the (peer, lo, hi) list equals Partition.boxes(rank), the offsets and the total are the running
    sum of the volumes, and peer_off of R's box towards S is off of S's box towards R.  The generator makes only valid partitions:
    one the validator refuses fails the test."""
    lib = host_lib()
    rng = np.random.RandomState(20240611)
    boxes = (C.c_int * (7 * MAX_BOXES))()
    offs = (C.c_uint64 * (3 * MAX_BOXES))()
    total = C.c_uint64()
    seen = set()
    for case in range(240):
        res, dims, cuts, margin, clip = draw(rng)
        seen.add(dims)
        part = Partition(res, dims, cuts, margin)
        part.clip = clip
        s = spec_of(res, dims, cuts, margin)
        off_of = {}
        peer_off_of = {}
        for rank in range(part.world):
            assert lib.tp_validate(C.byref(s), rank) == b"", (case, res, dims, cuts, margin)
            n = lib.tp_plan(C.byref(s), ivec(clip[0]), ivec(clip[1]), None, rank, 1 << 40, MAX_BOXES, boxes, offs, C.byref(total))
            assert 0 <= n <= MAX_BOXES, (case, n)
            got = [(boxes[7 * i], list(boxes[7 * i + 1:7 * i + 4]), list(boxes[7 * i + 4:7 * i + 7])) for i in range(n)]
            assert got == part.boxes(rank), (case, rank, res, dims, cuts, margin, clip)
            run = 0
            for i, (peer, lo, hi) in enumerate(got):
                vol = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])
                assert (offs[3 * i], offs[3 * i + 1]) == (vol, run), (case, rank, i)
                off_of[(rank, peer)], peer_off_of[(rank, peer)] = run, offs[3 * i + 2]
                run += vol
            assert total.value == run, (case, rank)
        assert set(off_of) == {(s_, r) for (r, s_) in off_of}
        for (r, s_), v in peer_off_of.items():
            assert v == off_of[(s_, r)], (case, r, s_)
    assert seen == set(DIMS)


def test_slack_and_schedule_equal_the_python_model():
    lib = host_lib()
    for margin in (1, 2, 3, 4):
        part = Partition((32, 32, 32), (2, 1, 1), [[0, 16, 32], [0, 32], [0, 32]], margin)
        assert lib.tp_clip_slack(margin) == part.clip_slack()
        for fixed in [None] + list(range(1, margin + 1)):
            rank = types.SimpleNamespace(part=part, k=7, migrate_interval=int(fixed or margin), adaptive_cap=0 if fixed else 64, next_migration=0)
            for speed in (0.0, 1e-12, 0.01, 0.3, 5.0, float("inf"), float("nan")):
                speed = float(np.float32(speed))  # (the table carries the speed as a float)
                TiledRank.schedule(rank, speed)
                assert lib.tp_next_interval(rank.migrate_interval, rank.adaptive_cap, margin, speed) == rank.next_migration - rank.k, (margin, fixed, speed)


def test_invariants_of_plans_with_per_rank_occupancy():
    """the same generator plus random occupancy boxes, some empty (a rank without particles): box(R, S) and box(S, R) are the same
    node set at each other's offsets; a rank's boxes are sorted by peer and tile [0, total); a node lies in box(R, S) exactly when it
    lies in both cut node boxes; the interior lies inside the cut node box and shares no node with any box; box_blocks is the count
    of 4^3 blocks marked node by node — all by enumeration (tests/cpp/tiled_plan_host.cpp: tp_invariants)"""
    lib = host_lib()
    rng = np.random.RandomState(777)
    seen = set()
    for case in range(42):
        res, dims, cuts, margin, clip = draw(rng)
        seen.add(dims)
        world = dims[0] * dims[1] * dims[2]
        occ = []
        for r in range(world):
            if rng.randint(4) == 0:
                occ += [0] * 6
            else:
                lo = [int(rng.randint(0, v + 1)) for v in res]
                occ += lo + [int(rng.randint(lo[a] + 1, res[a] + 2)) for a in range(3)]
        s = spec_of(res, dims, cuts, margin)
        assert lib.tp_invariants(C.byref(s), ivec(clip[0]), ivec(clip[1]), ivec(occ)) == 0, (case, res, dims, cuts, margin, clip, occ)
        assert lib.tp_invariants(C.byref(s), ivec(clip[0]), ivec(clip[1]), None) == 0, (case, res, dims, cuts, margin, clip)
    assert seen == set(DIMS)


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_planner(scenario):
    """tp_two_bricks, tp_occupancy_cut_interior (the interior against the cut node box, and its collapse against the uncut one that
    mpmhip_set_halo still hands over), tp_three_in_a_row, tp_no_interior: plans and interiors.  tp_arena: every offset of (halo_cap 1000,
    inbox_cap 65536), alignment, no overlap, the 2^31 refusal.  tp_mig_table: a three-rank table, one rank without particles; an inbox
    one record too small.  tp_after_*: what tests/test_gpu_tiled.py sees on the device, replayed — the first plan of two blobs, the
    re-plan near the cut, the error with its six numbers, the grid-edge exemptions, the shrink rule on both sides of its bound,
    arrivals that widen a rank's box.  tp_schedule, tp_validation: every message, one wrong field at a time.
    A scenario returns the line of its first failed check in tests/cpp/tiled_plan_host.cpp."""
    assert getattr(host_lib(), scenario)() == 0


def test_every_scenario_under_the_sanitizers():
    """the same source as a stand-alone program (its main() runs every scenario and the invariants on partitions of its own) built
    with -fsanitize=address,undefined; the runtime is linked statically, so nothing has to be preloaded"""
    os.makedirs(os.path.dirname(SAN), exist_ok=True)
    if _stale(SAN):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-static-libubsan", SRC, "-o", SAN])
    r = subprocess.run([SAN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "scenarios ok" in r.stdout, r.stdout
