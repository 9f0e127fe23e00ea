"""CPIC rigid bodies on a tiled job, the parts that need no device: the arithmetic of the impulse rows (csrc/tiled_plan.h) as a
stand-alone host program under the sanitizers (tests/cpp/cpic_job_host.cpp), and the resource metadata of the kernels of
csrc/k_rigid_rows.h read from the gfx950 code object."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

SRC = os.path.join(ROOT, "tests", "cpp", "cpic_job_host.cpp")
HDR = os.path.join(ROOT, "taichi_mpm_amd", "csrc", "tiled_plan.h")
SAN = os.path.join(ROOT, "tests", "cpp", "_build", "cpic_job_host_san")
LLVM = "/opt/rocm/lib/llvm/bin"


def test_row_arithmetic_under_the_sanitizers():
    """by_hand: offsets, capacities and epoch words of an 8-rank job written out.  no_overlap: for world = 1, 2, 8, 64 and four node
    capacities up to the 2^31 bound, the rows of both parities and both exchanges against the nodes and each other, byte ranges
    enumerated.  arena_unchanged: tp_arena's numbers again, and what a job with bodies adds."""
    os.makedirs(os.path.dirname(SAN), exist_ok=True)
    if not os.path.exists(SAN) or os.path.getmtime(SAN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-static-libubsan", SRC, "-o", SAN])
    r = subprocess.run([SAN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "cpic_job: 3 scenarios ok" in r.stdout, r.stdout


ROW_KERNELS = ["_ZN3mpm16k_rigid_rows_sum", "_ZN3mpm15k_rigid_row_out", "_ZN3mpm18k_rigid_rows_world"]


@pytest.fixture(scope="module")
def stats():
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    import __graft_entry__ as g
    g.build()
    import kernel_diff
    from taichi_mpm_amd import _lib
    return kernel_diff.kernel_stats(_lib.build())


@pytest.mark.parametrize("prefix", ROW_KERNELS)
def test_row_kernels_use_no_scratch_and_at_most_64_vgprs(stats, prefix):
    hits = {k: v for k, v in stats.items() if k.startswith(prefix)}
    assert len(hits) == 1, (prefix, sorted(hits))
    s = next(iter(hits.values()))
    print(prefix, s)
    assert s["vgpr_spill"] == 0 and s["sgpr_spill"] == 0 and s["scratch_bytes"] == 0, s
    assert s["vgpr"] <= 64, s
