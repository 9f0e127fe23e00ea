"""The periodic blue-noise tile behind mpmhip2d_seed_particles (taichi_mpm_amd/csrc/poisson_tile.h) compiled for the host by g++
(tests/cpp/poisson_tile2d_host.cpp: the header alone), the numpy model of the seeding call (tests/seed2d_model.py) on top of it,
and SampledLevelSet2D.from_polygon.  No GPU needed; tests/test_gpu_seed2d.py compares the device with the model and takes its
setup (RES, DX, PPC, the shape cases) from here."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "poisson_tile2d_host.cpp")
HDR = os.path.join(ROOT, "taichi_mpm_amd", "csrc", "poisson_tile.h")
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "libpoisson_tile2d_host.so")

# the setup of the 2D seeding tests: the tile is 40 * sqrt(1 / 6) dx = 16.33 dx wide
RES, DX, DT, PPC = 64, 1.0 / 64, 1e-4, 4.0
R12, R4 = 12 * DX, 4 * DX
MARGIN = 1e-4  # grid units: candidates with |phi| below it are set aside where the region is given by shapes
# name -> (the region's shapes as (type, inside_out, p[6]) rows, the replicas per axis)
SHAPES = {
    "disc_r12": ([(1, 0, [0.5, 0.5, 0.0, R12, 0, 0])], (2, 2)),
    "box": ([(2, 0, [0.3, 0.33, 0.0, 0.62, 0.52, 0.0])], (2, 1)),
    "disc_r4": ([(1, 0, [0.5, 0.5, 0.0, R4, 0, 0])], (1, 1)),
    # everything outside a disc of r = 20 dx: the region reaches all four walls and the 7-cell margin cuts it
    "inside_out_disc": ([(1, 1, [0.5, 0.5, 0.0, 20 * DX, 0, 0])], (4, 4)),
    # a box that reaches x = 0.05 (3.2 cells from the -x wall)
    "wall_box": ([(2, 0, [0.05, 0.4, 0.0, 0.3, 0.6, 0.0])], (2, 1)),
}


def host_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(OUT):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", SRC, "-o", OUT])
    L = C.CDLL(OUT)
    L.pt2_generate.argtypes = [C.POINTER(C.c_float), C.c_longlong]
    L.pt2_generate.restype = C.c_longlong
    return L


def generate():
    L = host_lib()
    n = L.pt2_generate(None, 0)
    out = np.empty((n, 2), np.float32)
    assert L.pt2_generate(out.ctypes.data_as(C.POINTER(C.c_float)), n) == n
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
    assert tile.shape == (997, 2) and tile.dtype == np.float32 and tile.nbytes == 7976
    assert hashlib.sha256(tile.tobytes()).hexdigest() == "47ace1b1a365480c6351a2bce059bb4f2a2a8a86a29b5c712325ad84107c2714"


def test_the_library_hands_out_the_same_tile(tile):
    """mpmhip2d_poisson_tile (hipcc's host compiler) and the g++ build of the header: integer arithmetic, the same bytes"""
    import __graft_entry__ as g
    g.build()
    from tests.seed2d_model import load_tile
    got = load_tile()
    assert got.shape == tile.shape and got.tobytes() == tile.tobytes()


def test_tile_lies_in_the_period_and_starts_at_the_centre(tile):
    assert tile.min() >= -20.0 and tile.max() < 20.0
    assert np.all(tile[0] == 0.0)


def test_every_point_keeps_its_distance_across_the_seams(tile):
    from scipy.spatial import cKDTree
    p = tile.astype(np.float64) + 20.0
    d, _ = cKDTree(p, boxsize=40.0).query(p, k=2)
    print("nearest periodic pair: %.6f" % d[:, 1].min())
    assert d[:, 1].min() >= 1.0, d[:, 1].min()


def test_count_bounds(tile):
    """between 1600 / pi = 510 (a point set whose covering radius is below 1; Bridson's output is nearly one: a sanity bound) and the
    circle-packing bound 1600 * 2 / sqrt(3) = 1847.  The count itself is recorded in DESIGN.md."""
    print("2D tile: %d points, %.4f per unit area" % (len(tile), len(tile) / 1600.0))
    assert 510 <= len(tile) <= 1847, len(tile)


def test_model_count_on_a_disc(tile):
    """r = 12 dx disc at res 64, ppc 4: the model's count against pi r^2 / min_distance^2 * rho_tile.  The margin covers the boundary
    ring: a point's disc of diameter min_distance straddles the circle when its centre is within min_distance / 2 of it, a ring of
    width min_distance whose share of the area is 2 pi r min_distance / (pi r^2) = 2 min_distance / r (6.8 % here; relatively wider
    than the 3D test's 3 % because perimeter / area is larger)"""
    from tests.seed2d_model import SeedModel2D, ShapeRegion2D
    shapes, nrep = SHAPES["disc_r12"]
    m = SeedModel2D(RES, DX, ShapeRegion2D(shapes, DX), ppc=PPC, tile=tile)
    got = len(m.run()["x"])
    rho = len(tile) / 1600.0
    want = np.pi * R12 ** 2 / float(m.min_distance) ** 2 * rho
    margin = 2.0 * float(m.min_distance) / R12
    print("model count %d, expected %.1f, ratio %.5f, margin %.5f" % (got, want, got / want, margin))
    assert abs(got / want - 1.0) < margin
    assert tuple(m.nrep) == nrep and m.n_cand == 4 * len(tile)
    assert abs(float(m.region_size) / DX - 16.33) < 0.005


@pytest.mark.parametrize("name", list(SHAPES))
def test_model_sets_aside_at_most_one_percent(tile, name):
    """what the GPU test of the shape regions relies on: the candidates within the margin of a shape's surface are few"""
    from tests.seed2d_model import SeedModel2D, ShapeRegion2D
    shapes, nrep = SHAPES[name]
    m = SeedModel2D(RES, DX, ShapeRegion2D(shapes, DX), ppc=PPC, tile=tile)
    want = m.run(margin=MARGIN)
    print("%s: %d candidates, %d survivors, %d unsure" % (name, want["n_cand"], len(want["x"]), len(want["unsure"])))
    assert tuple(m.nrep) == nrep
    assert len(want["x"]) > 0 and len(want["unsure"]) <= 0.01 * want["n_cand"]


def test_model_sampled_disc_agrees_with_the_shape(tile):
    """the bilinear field of a disc on a dx / 2 lattice and the analytic disc accept the same candidates up to a thin ring (the
    interpolant of a convex distance lies above it by at most spacing^2 / (8 r) = 0.0026 dx here)"""
    import taichi_mpm_amd as tm
    from tests.seed2d_model import SampledRegion2D, SeedModel2D, ShapeRegion2D
    origin = tuple(np.float32(0.5 - 14.3 * DX + 0.0137 * DX) for _ in range(2))
    sls = tm.SampledLevelSet2D.from_function(lambda x: np.linalg.norm(x - 0.5, axis=1) - R12, (60, 60), origin, DX / 2)
    a = SeedModel2D(RES, DX, SampledRegion2D(sls.phi, sls.origin, sls.spacing, DX), ppc=PPC, tile=tile).run()
    b = SeedModel2D(RES, DX, ShapeRegion2D(SHAPES["disc_r12"][0], DX), ppc=PPC, tile=tile).run(margin=0.01)
    diff = np.setxor1d(a["c"], b["c"])
    assert len(a["c"]) > 1000 and np.all(np.isin(diff, b["unsure"])), (len(diff), len(b["unsure"]))


def test_from_polygon_unit_square_is_the_box_distance():
    import taichi_mpm_amd as tm
    sq = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]
    sls = tm.SampledLevelSet2D.from_polygon(sq, (41, 37), (-0.51, -0.43), 0.05)
    p = tm.SampledLevelSet2D.lattice_points((41, 37), (-0.51, -0.43), 0.05)
    q = np.abs(p - 0.5) - 0.5  # the closed form of a box's signed distance
    want = np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(axis=1), 0.0)
    assert sls.phi.shape == (41, 37)
    assert np.abs(sls.phi.reshape(-1) - want).max() < 1e-6
    rev = tm.SampledLevelSet2D.from_polygon(sq[::-1], (41, 37), (-0.51, -0.43), 0.05)  # the orientation does not matter
    assert rev.phi.tobytes() == sls.phi.tobytes()


def test_from_polygon_sign_of_a_concave_polygon():
    """an L: the unit square without its upper right quarter"""
    import taichi_mpm_amd as tm
    L = [(0.0, 0.0), (1.0, 0.0), (1.0, 0.5), (0.5, 0.5), (0.5, 1.0), (0.0, 1.0)]
    d = tm.SampledLevelSet2D.polygon_distance
    pts = np.array([(0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75), (0.6, 0.6), (0.45, 0.9), (1.2, 0.25), (-0.1, 0.5),
                    (0.25, 0.5), (0.75, 0.5 + 1e-9)])
    want = np.array([-0.25, -0.25, -0.25, 0.25, 0.1, -0.05, 0.2, 0.1, -0.25, 1e-9])
    got = d(L, pts)
    assert np.abs(got - want).max() < 1e-12, got
    assert abs(d(L, [(1.1, 0.6)])[0] - np.hypot(0.1, 0.1)) < 1e-12  # the nearest point is the corner (1, 0.5)


def test_sampled_levelset2d_refuses_what_it_cannot_hold():
    import taichi_mpm_amd as tm
    with pytest.raises(tm.MPMError, match="2 axes"):
        tm.SampledLevelSet2D(np.zeros((4, 4, 4)))
    with pytest.raises(tm.MPMError, match="at least 2 samples"):
        tm.SampledLevelSet2D(np.zeros((1, 4)))
    with pytest.raises(tm.MPMError, match="non-finite"):
        tm.SampledLevelSet2D(np.full((4, 4), np.nan))
    with pytest.raises(tm.MPMError, match="spacing"):
        tm.SampledLevelSet2D(np.zeros((4, 4)), spacing=0.0)
    with pytest.raises(tm.MPMError, match="at least 3"):
        tm.SampledLevelSet2D.from_polygon([(0, 0), (1, 1)], (4, 4), (0, 0), 0.1)
    sim = tm.create_simulation2("mpm").initialize(dict(res=(RES, RES), delta_x=DX))
    with pytest.raises(tm.MPMError, match="region for add_particles"):
        sim.set_levelset(tm.SampledLevelSet2D(np.zeros((4, 4)), spacing=DX))


def test_ctypes_mirrors_of_the_2d_seeding_structs(tmp_path):
    """mpmhip2d_sdf_desc and mpmhip2d_seed_desc: sizeof and the offset of every field, as gcc lays out include/mpmhip.h, against the
    ctypes mirrors of taichi_mpm_amd/_lib.py"""
    from taichi_mpm_amd import _lib
    pairs = [("mpmhip2d_sdf_desc", _lib.SdfDesc2D), ("mpmhip2d_seed_desc", _lib.SeedDesc2D)]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "mpmhip.h"', "int main(void) {"]
    for cname, mirror in pairs:
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in mirror._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ["  return 0;", "}"]
    src = tmp_path / "abi2d.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "abi2d"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    for cname, mirror in pairs:
        assert got[(cname, "size")] == C.sizeof(mirror), cname
        for fname, _ in mirror._fields_:
            assert got[(cname, fname)] == getattr(mirror, fname).offset, (cname, fname)
