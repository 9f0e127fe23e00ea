"""Resource condition of the region-expression kernels, read from the gfx950 code object of the built library (no GPU needed: hipcc
cross-compiles).  RegionExpr<D> keeps its four stack slots in named registers and reads the program, leaves and fields from the
kernel arguments: an indexed private array, or a description copied to per-lane memory, would show as scratch.  Every
k_seed_bounds / k_seed_count instantiation over RegionExpr and the two ctx-free kernels must report no scratch and no VGPR spill.
Only metadata fields are read (profiles/kernel_diff.py: kernel_stats)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def stats():
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm-readelf of the ROCm toolchain not found")
    from taichi_mpm_amd import _lib
    import kernel_diff
    return kernel_diff.kernel_stats(_lib.build())


def test_region_kernels_use_no_scratch_and_spill_nothing(stats):
    want = {"k_seed_bounds": 2, "k_seed_count": 2, "k_region_sample": 2, "k_region_bake": 2}  # D = 2 and D = 3 of each
    seen = dict.fromkeys(want, 0)
    for name, s in sorted(stats.items()):
        base = next((b for b in want if ("%d%s" % (len(b), b)) in name), None)
        if base is None or (base.startswith("k_seed") and "RegionExpr" not in name):
            continue
        seen[base] += 1
        print("%s: %d VGPRs, %d SGPRs, %d bytes of scratch, %d spilled VGPRs" % (name, s["vgpr"], s["sgpr"], s["scratch_bytes"], s["vgpr_spill"]))
        assert s["scratch_bytes"] == 0 and s["vgpr_spill"] == 0, (name, s)
    assert seen == want, seen


def test_the_plain_seeding_kernels_are_still_there(stats):
    """the instantiations a plain region launches (SeedRegion, SeedRegion2) exist beside the new ones, without scratch as before"""
    for region in ("10SeedRegion", "11SeedRegion2"):
        for kern in ("13k_seed_bounds", "12k_seed_count"):
            hits = [s for name, s in stats.items() if kern in name and ("NS_%sE" % region) in name]
            assert len(hits) == 1 and hits[0]["scratch_bytes"] == 0, (kern, region, hits)
