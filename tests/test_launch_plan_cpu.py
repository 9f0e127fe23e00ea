"""Which kernel instantiation each phase of a substep launches, and with how many workgroups (taichi_mpm_amd/csrc/launch_plan.h:
Knobs, Facts, plan_sort / plan_p2g / plan_grid / plan_g2p) compiled for the host by g++, the header alone: no HIP header is included,
no HIP runtime linked or loaded (tests/cpp/launch_plan_host.cpp).  The scenarios restate every rule and compare it with the header's
answer at both sides of each boundary: slot counts around 2 M and 6 M, block fills around 448 per block, owner counts, material
masks, every boolean fact, every environment switch unset, inside and outside its clamp.  The same source, with its main(), runs
once as a program of its own under AddressSanitizer and UBSan.  No GPU needed: the GPU suite checks what the kernels compute,
this checks that the intended ones are launched."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "launch_plan_host.cpp")
HDR = os.path.join(ROOT, "taichi_mpm_amd", "csrc", "launch_plan.h")
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "liblaunch_plan_host.so")
SAN = os.path.join(ROOT, "tests", "cpp", "_build", "launch_plan_host_san")


def _stale(out):
    return not os.path.exists(out) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(out)


def host_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if _stale(OUT):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", SRC, "-o", OUT])
    return C.CDLL(OUT)


def test_the_test_library_does_not_pull_in_the_hip_runtime():
    host_lib()
    needed = subprocess.check_output(["readelf", "-d", OUT], text=True)
    assert "amdhip64" not in needed and "libhsa" not in needed, needed


@pytest.mark.parametrize("scenario", ["lp_env", "lp_sort", "lp_p2g", "lp_grid", "lp_g2p", "lp_known_configurations", "lp_scan_grid"])
def test_plan(scenario):
    """lp_env: Knobs::from_env, today's defaults and clamps, nothing cached between two reads.  lp_sort: keyed front, blocks per
    chunk, owner list, rank and cell-order launches.  lp_p2g: launch sizes and the colour-aware kernel's material set.  lp_grid:
    the walk, its launch size, the sampled instantiation, the refusal of calculate_energy on a tiled ctx without the owner list.
    lp_g2p: packed or per block, material set, launch sizes.  lp_known_configurations: the plans of the measured configurations,
    written out by hand.  A scenario returns the line of its first failed check in tests/cpp/launch_plan_host.cpp."""
    assert getattr(host_lib(), scenario)() == 0


def test_every_scenario_under_the_sanitizers():
    """the same source as a stand-alone program (its main() runs every scenario) built with -fsanitize=address,undefined; the
    runtime is linked statically, so nothing has to be preloaded and nothing that is preloaded comes before it"""
    os.makedirs(os.path.dirname(SAN), exist_ok=True)
    if _stale(SAN):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-static-libubsan", SRC, "-o", SAN])
    r = subprocess.run([SAN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "scenarios ok" in r.stdout, r.stdout
