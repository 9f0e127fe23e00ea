"""Resource budget of the tuned transfer kernels, read from the gfx950 code object of the built library (no GPU needed:
hipcc cross-compiles).  The measured speed of k_g2p / k_p2g rests on their occupancy class (k_g2p: three workgroups per CU, i.e.
<= 168 VGPRs and <= 53 KB of LDS each; k_p2g: <= 256 VGPRs), on the absence of scratch (a spill turns register traffic
into memory traffic) and on an instruction count in the range the profiles were taken with — a compiler update or an
innocent edit that leaves these bands shows up here, before GPU time is spent on it (profiles/kernel_diff.py --stats
prints the table)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def stats():
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    from taichi_mpm_amd import _lib
    import kernel_diff
    return kernel_diff.kernel_stats(_lib.build())


def _one(stats, prefix):
    hits = {k: v for k, v in stats.items() if k.startswith(prefix)}
    assert len(hits) == 1, (prefix, sorted(hits))
    return next(iter(hits.values()))


# name prefix (mangled, up to the template arguments) -> (max VGPRs, instruction band, max static LDS bytes).
# k_g2p: <= 168 VGPRs = THREE workgroups per CU (512 registers per SIMD lane, allocated in eights); at 180 the same code ran
# 14 % slower on the same box (profiles/r03_b_ab_vgpr.txt) — the all-material kernel (MATS = 510, visco included) is the one
# instantiation allowed above it.
G2P = "_ZN3mpm5k_g2pILi256ELi%dELb1ELb0ELb0ELj%dEEE"  # <NT, MINW, ROLL, STORE_B, RIGID, MATS>
# (round 5: + ~450 instructions per eigen-solve for the refinement of ill-conditioned F — a wave-uniform branch the benchmark
# states never take, working in LDS so that the VGPR classes below did not move: csrc/mpm_math.h: sym_eig3_refine)
BUDGET = {
    G2P % (2, 64): (168, (2800, 3750), 53 * 1024),    # sand only (the benchmark configuration C3)
    G2P % (2, 16): (168, (2600, 3650), 53 * 1024),    # jelly only (C2)
    G2P % (2, 508): (168, (3400, 4650), 53 * 1024),   # every material but visco (mixed scenes, C5)
    G2P % (2, 510): (256, (6000, 8000), 80 * 1024),   # all eight (visco: two eigen-solves)
    # k_g2p_packed (large problems without rigid bodies / tiling): the same occupancy class with four block tiles in LDS
    "_ZN3mpm12k_g2p_packedILi256ELi2ELb0ELj64EEE": (168, (2950, 3950), 53 * 1024),   # sand
    "_ZN3mpm12k_g2p_packedILi256ELi2ELb0ELj128EEE": (168, (2950, 3950), 53 * 1024),  # von Mises: the fullest of the seven instantiated
    "_ZN3mpm5k_p2gILb0EEE": (256, (900, 1450), 16 * 1024),  # P2G (one wave per block)
    # the plain kernels of a ctx WITH rigid bodies (they skip the flagged blocks): same occupancy class as without —
    # k_g2p<RIGID> runs beside k_g2p_rigid, whose 255-register workgroups only find room when this one leaves it
    "_ZN3mpm5k_g2pILi256ELi2ELb1ELb0ELb1ELj64EEE": (168, (2800, 3750), 53 * 1024),
    "_ZN3mpm5k_p2gILb1EEE": (256, (900, 1500), 16 * 1024),
}


@pytest.mark.parametrize("prefix", sorted(BUDGET))
def test_tuned_kernels_stay_inside_their_budget(stats, prefix):
    s = _one(stats, prefix)
    vmax, (ilo, ihi), lds = BUDGET[prefix]
    assert s["vgpr_spill"] == 0 and s["scratch_bytes"] == 0, s
    assert 128 < s["vgpr"] + s.get("agpr", 0) <= vmax, s
    assert ilo <= s["instructions"] <= ihi, s
    assert s["lds_bytes"] <= lds, s


def test_no_kernel_of_the_library_uses_scratch_unnoticed(stats):
    """every kernel that spills is listed here on purpose (none of them is on the per-substep path of a scene without bodies)"""
    # the CPIC transfers (colour test per node on top of the full kernels); rocprim = the one library sort (order of the rigid boundary
    # particles for rigid_body_levelset_collision, rigid_api.h — off the substep path of every scene that does not set that key)
    allowed = ("k_p2g_rigid", "k_g2p_rigid", "rocprim")
    bad = [k for k, v in stats.items() if v.get("scratch_bytes", 0) > 0 and not any(a in k for a in allowed)]
    # k_g2p<STORE_B = true> (keep_apic_b scenes, never the benchmark's): since Params::pidc the compiler RESERVES 36 bytes of private
    # segment for these four instantiations and never touches them — no spill counted, no scratch instruction in the code.  Held to
    # exactly that: a reserved but unused segment costs no memory traffic.
    from taichi_mpm_amd import _lib
    import kernel_diff
    code = kernel_diff.kernels(_lib.build())
    reserved_only = [k for k in bad if k.startswith("_ZN3mpm5k_g2pILi256ELi2ELb1ELb1E") and stats[k]["vgpr_spill"] == 0
                     and not any(i.startswith(("scratch_", "buffer_")) for i in code[k])]
    assert len(reserved_only) <= 4
    bad = [k for k in bad if k not in reserved_only]
    assert not bad, bad
