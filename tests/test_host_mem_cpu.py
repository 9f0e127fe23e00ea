"""The owners of the host layer's device and pinned arrays (taichi_mpm_amd/csrc/host_mem.h: DevBuf, PinnedBuf and the live-buffer
counter behind mpmhip_debug_live_buffers) compiled for the host by g++ against malloc-backed stand-ins for the six runtime
functions the header calls (tests/cpp/host_mem_host.cpp): no HIP runtime is linked or loaded.  Every allocation is released exactly
once, the failure paths of alloc / regrow keep what they promise, moves and swaps neither leak nor free twice.  No GPU needed;
tests/test_gpu_lifetime.py asks the same of whole objects on the device."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "host_mem_host.cpp")
HDR = os.path.join(ROOT, "taichi_mpm_amd", "csrc", "host_mem.h")
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "libhost_mem_host.so")


def host_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(OUT):
        subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O1", "-Wall", "-shared", "-fPIC",
                               SRC, "-o", OUT])
    L = C.CDLL(OUT)
    L.hm_live.restype = C.c_long
    return L


def test_the_test_library_does_not_pull_in_the_hip_runtime():
    host_lib()
    needed = subprocess.check_output(["readelf", "-d", OUT], text=True)
    assert "amdhip64" not in needed and "libhsa" not in needed, needed


@pytest.mark.parametrize("pinned", [0, 1], ids=["DevBuf", "PinnedBuf"])
@pytest.mark.parametrize("scenario", ["hm_release_once", "hm_failed_alloc", "hm_regrow", "hm_move_and_swap"])
def test_buffer(scenario, pinned):
    """destruction / reset / alloc over a held buffer release exactly once; a failed alloc leaves the buffer empty and the counter
    unchanged; a failed regrow keeps the old pointer and bytes, a successful one keeps `keep` elements, zero-fills the rest when
    asked and releases the old array; move and std::swap neither leak nor double-free.  A scenario returns the line of its first
    failed check in tests/cpp/host_mem_host.cpp."""
    L = host_lib()
    assert getattr(L, scenario)(pinned) == 0
    assert L.hm_live() == 0


def test_device_and_pinned_buffers_release_through_their_own_call_and_share_the_counter():
    L = host_lib()
    assert L.hm_kinds_do_not_mix() == 0
    assert L.hm_live() == 0
