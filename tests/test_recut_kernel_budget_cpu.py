"""Resource budget of the kernels of a re-cut (csrc/k_tiling.h: k_live_histogram, k_recut_count, k_recut_pack), read from the gfx950
code object of the built library as tests/test_kernel_budget_cpu.py reads the transfer kernels' (no GPU needed: hipcc cross-compiles).
They are single passes over the particle records, bounded by the record read: no scratch, a register count that leaves the wave
slots full, and for the histogram no static LDS beyond its reduction words (the rows are dynamic: 3 res words)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
LLVM = "/opt/rocm/lib/llvm/bin"

# mangled name -> (max VGPRs, max instructions, max static LDS bytes).  64 VGPRs = eight waves per SIMD.
BUDGET = {
    "_ZN3mpm16k_live_histogramILb1EEE": (64, 700, 256),
    "_ZN3mpm16k_live_histogramILb0EEE": (64, 700, 256),
    "_ZN3mpm13k_recut_count": (64, 600, 256),
    "_ZN3mpm12k_recut_pack": (64, 600, 0),
}


@pytest.fixture(scope="module")
def stats():
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    from taichi_mpm_amd import _lib
    import kernel_diff
    return kernel_diff.kernel_stats(_lib.build())


@pytest.mark.parametrize("prefix", sorted(BUDGET))
def test_recut_kernels_stay_inside_their_budget(stats, prefix):
    hits = {k: v for k, v in stats.items() if k.startswith(prefix)}
    assert len(hits) == 1, (prefix, sorted(hits))
    s = next(iter(hits.values()))
    vmax, imax, lds = BUDGET[prefix]
    assert s["vgpr_spill"] == 0 and s["scratch_bytes"] == 0, s
    assert s["vgpr"] + s.get("agpr", 0) <= vmax, s
    assert s["instructions"] <= imax, s
    assert s["lds_bytes"] <= lds, s
