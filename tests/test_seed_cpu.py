"""The periodic blue-noise tile behind mpmhip_seed_particles (taichi_mpm_amd/csrc/poisson_tile.h) compiled for the host by g++
(tests/cpp/poisson_tile_host.cpp: the header alone), and the numpy model of the seeding call (tests/seed_model.py) on top of it.
No GPU needed; tests/test_gpu_seed.py compares the device with the model."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "poisson_tile_host.cpp")
HDR = os.path.join(ROOT, "taichi_mpm_amd", "csrc", "poisson_tile.h")
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "libpoisson_tile_host.so")


def host_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(OUT):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", SRC, "-o", OUT])
    L = C.CDLL(OUT)
    L.pt_generate.argtypes = [C.POINTER(C.c_float), C.c_longlong]
    L.pt_generate.restype = C.c_longlong
    return L


def generate():
    L = host_lib()
    n = L.pt_generate(None, 0)
    out = np.empty((n, 3), np.float32)
    assert L.pt_generate(out.ctypes.data_as(C.POINTER(C.c_float)), n) == n
    return out


@pytest.fixture(scope="module")
def tile():
    return generate()


def test_two_generations_give_identical_bytes(tile):
    again = generate()
    assert again.shape == tile.shape and again.tobytes() == tile.tobytes()


def test_tile_bytes_are_pinned(tile):
    """the count and the SHA-256 of the fp32 array as handed out (C order).  The other tests compare two builds of the same header, so
    a change of the generator would pass them; with the test below this pins the library's tile too"""
    assert tile.shape == (37177, 3) and tile.dtype == np.float32 and tile.nbytes == 446124
    assert hashlib.sha256(tile.tobytes()).hexdigest() == "154d40d1172514708b2c3e5d94313f763577e149d1301a1e664f72f895f81bd2"


def test_the_library_hands_out_the_same_tile(tile):
    """mpmhip_poisson_tile (hipcc's host compiler) and the g++ build of the header: integer arithmetic, the same bytes"""
    import __graft_entry__ as g
    g.build()
    from tests.seed_model import load_tile
    assert load_tile().tobytes() == tile.tobytes()


def test_tile_lies_in_the_period_and_starts_at_the_centre(tile):
    assert tile.min() >= -20.0 and tile.max() < 20.0
    assert np.all(tile[0] == 0.0)


def test_every_point_keeps_its_distance_across_the_seams(tile):
    """nearest periodic neighbour at distance >= 1: the reference's seam handling (70 cells of side 1 / sqrt(3) cover 40.41, the
    wrapped cell index skips a cell) fails this with 228 of 37 167 points, the nearest at 0.816"""
    from scipy.spatial import cKDTree
    p = tile.astype(np.float64) + 20.0
    d, _ = cKDTree(p, boxsize=40.0).query(p, k=2)
    assert d[:, 1].min() >= 1.0, d[:, 1].min()


def test_count_bounds(tile):
    """between 64 000 / (4 pi / 3) = 15 279 (a point set whose covering radius is below 1; Bridson's output is nearly one: a sanity
    bound) and the sphere-packing bound 90 500.  The count itself is recorded in DESIGN.md."""
    assert 15279 <= len(tile) <= 90500, len(tile)


def test_model_count_on_a_sphere(tile):
    """r = 12 dx sphere at res 64, ppc 8: the model's count is within 3 % of V / min_distance^3 * rho_tile (the margin covers the
    surface shell; the tile is uniform at the scale of the sphere)"""
    from tests.seed_model import SeedModel, ShapeRegion
    res, dx = 64, 1.0 / 64
    r = 12 * dx
    m = SeedModel(res, dx, ShapeRegion([(1, 0, [0.5, 0.5, 0.5, r, 0, 0])], dx), ppc=8.0, tile=tile)
    got = len(m.run()["x"])
    rho = len(tile) / 64000.0
    want = 4.0 / 3.0 * np.pi * r ** 3 / float(m.min_distance) ** 3 * rho
    print("model count %d, expected %.1f, ratio %.5f" % (got, want, got / want))
    assert abs(got / want - 1.0) < 0.03
    assert tuple(m.nrep) == (2, 2, 2) and m.n_cand == 8 * len(tile)
