"""mpmhip_seed_particles_brick / mpmhip_seed_histogram without a GPU: the model of the calls (tests/seed_brick_model.py) against a brute
force loop over the candidates, and the resource condition of the new kernels read from the gfx950 code object (hipcc cross-compiles;
profiles/kernel_diff.py: kernel_stats, metadata fields only).  Setup of tests/test_gpu_seed.py: res 64^3, dx = 1/64, ppc 8; the
r = 4 dx sampled sphere at the centre is one replica of the tile and a few thousand particles, the cuts of every partition below pass
through it."""
import os
import sys

import numpy as np
import pytest

from taichi_mpm_amd import tiled
from tests import seed_brick_model as sbm
from tests.seed_model import load_tile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
LLVM = "/opt/rocm/lib/llvm/bin"
RES, DX, PPC = 64, 1.0 / 64, 8.0
R4 = 4 * DX
PARTS = [(2, None), (4, None), (8, None), (3, (1, 3, 1))]


@pytest.fixture(scope="module")
def small():
    """the model of the small sphere and its one-ctx result, shared and left unchanged"""
    import taichi_mpm_amd as tm
    sls = sbm.sampled_sphere(tm, (0.5, 0.5, 0.5), R4, DX)
    m = sbm.sampled_model(sls, RES, DX, load_tile(), ppc=PPC)
    want = m.run()
    assert tuple(m.nrep) == (1, 1, 1) and 1000 < len(want["x"]) < 4000
    return m, want


def _part(x, world, dims):
    part = tiled.Partition.balanced((RES,) * 3, world, x, DX, margin=2, dims=dims)
    b = tiled.base_cells(x, DX)
    for a in range(3):  # every cut plane passes through the particles
        assert all(b[:, a].min() < c <= b[:, a].max() for c in part.cuts[a][1:-1])
    return part


@pytest.mark.parametrize("world,dims", PARTS)
def test_the_split_model_is_the_brute_force_loop(small, world, dims):
    m, want = small
    part = _part(want["x"], world, dims)
    got = sbm.split(want["x"], part, DX, first_id=17)
    ref, _ = sbm.brute_force(m, part, first_id=17)
    for r in range(world):
        assert len(got[r]["id"]) > 0
        assert np.array_equal(got[r]["id"], ref[r]["id"]) and got[r]["x"].tobytes() == ref[r]["x"].tobytes()


@pytest.mark.parametrize("world,dims", PARTS)
def test_ids_partition_the_job_and_ascend_within_a_rank(small, world, dims):
    _, want = small
    n = len(want["x"])
    ranks = sbm.split(want["x"], _part(want["x"], world, dims), DX)
    ids = np.concatenate([r["id"] for r in ranks])
    assert len(ids) == n and np.array_equal(np.sort(ids), np.arange(n))  # disjoint, and their union is arange(n)
    for r in ranks:
        assert (np.diff(r["id"]) > 0).all()
        assert r["x"].tobytes() == want["x"][r["id"]].tobytes()


def test_histogram_model(small):
    m, want = small
    hists, lo, hi, total = sbm.histograms(want["x"], (RES,) * 3, DX)
    b = tiled.base_cells(want["x"], DX)
    for a in range(3):
        assert np.array_equal(hists[a], np.bincount(b[:, a], minlength=RES))
    assert total == len(b) and np.array_equal(lo, b.min(0)) and np.array_equal(hi, b.max(0) + 1)
    _, brute = sbm.brute_force(m, _part(want["x"], 2, None))
    for a in range(3):
        assert np.array_equal(hists[a], brute[a])


@pytest.mark.parametrize("world,dims", PARTS)
def test_partition_from_the_histograms_is_the_balanced_one(small, world, dims):
    _, want = small
    hists, lo, hi, _ = sbm.histograms(want["x"], (RES,) * 3, DX)
    a = tiled.Partition.from_histograms((RES,) * 3, world, hists, lo, hi, margin=2, dims=dims)
    b = tiled.Partition.balanced((RES,) * 3, world, want["x"], DX, margin=2, dims=dims)
    assert a.cuts == b.cuts and a.dims == b.dims and a.clip == b.clip


# ---------------------------------------------------------------------------------------------------- the code object
@pytest.fixture(scope="module")
def stats():
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm-readelf of the ROCm toolchain not found")
    from taichi_mpm_amd import _lib
    import kernel_diff
    return kernel_diff.kernel_stats(_lib.build())


def test_brick_kernels_exist_and_use_no_scratch(stats):
    """k_seed_count_brick and k_seed_hist once per 3D region type, k_seed_write_brick for the 3D sink (the region does not reach it),
    the two-sum scan; none with scratch or a spilled VGPR"""
    regions = ("NS_10SeedRegionE", "NS_10RegionExprILi3EEE")
    want = [("18k_seed_count_brick", r) for r in regions] + [("11k_seed_hist", r) for r in regions] + \
           [("18k_seed_write_brick", "NS_9SeedSink3E"), ("12k_seed_scan2", "")]
    for kern, arg in want:
        hits = {name: s for name, s in stats.items() if kern in name and arg in name}
        assert len(hits) == 1, (kern, arg, sorted(hits))
        (name, s), = hits.items()
        print("%s: %d VGPRs, %d SGPRs, %d bytes of scratch, %d spilled VGPRs" % (name, s["vgpr"], s["sgpr"], s["scratch_bytes"], s["vgpr_spill"]))
        assert s["scratch_bytes"] == 0 and s["vgpr_spill"] == 0, (name, s)
