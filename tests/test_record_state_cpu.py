"""The owner of mpmhip_ctx's validity flags (taichi_mpm_amd/csrc/record_state.h: RecordState) compiled for the host by g++, the
header alone: no HIP header is included, no HIP runtime linked or loaded (tests/cpp/record_state_host.cpp).  A breadth-first walk
over every state reachable from a fresh ctx under every transition checks the invariants the host code relies on; the other
scenarios replay the host code's own sequences.  No GPU needed; tests/test_gpu_deterministic.py asks for the bit-identical run
that the ids_changed transition exists for."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "record_state_host.cpp")
HDR = os.path.join(ROOT, "taichi_mpm_amd", "csrc", "record_state.h")
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "librecord_state_host.so")


def host_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(OUT):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", SRC, "-o", OUT])
    return C.CDLL(OUT)


def test_the_test_library_does_not_pull_in_the_hip_runtime():
    host_lib()
    needed = subprocess.check_output(["readelf", "-d", OUT], text=True)
    assert "amdhip64" not in needed and "libhsa" not in needed, needed


def test_every_reachable_state_keeps_the_invariants():
    """sorted => !keys_valid, pidc_valid => keys_valid, compact => ordered, b_stale => affine_valid on every state; after a
    transition that moves or replaces positions outside G2P no index, key, id cache or record order is valid, and the block flags
    are cleared whenever G2P had set them.  The walk returns the line of its first failed check in
    tests/cpp/record_state_host.cpp."""
    L = host_lib()
    assert L.rs_walk() == 0
    # seven booleans: at most 128; the four implications leave 4 (sorted, keys, pidc) x 3 (affine, b) x 3 (ordered, compact) = 36
    # states, and the walk reaches every one of them: the implications are all that the transitions guarantee
    assert L.rs_states() == 36, L.rs_states()
    assert L.rs_transitions() == 20  # every transition of the header with every argument value (update the table with the header)


@pytest.mark.parametrize("scenario", ["rs_ids_changed", "rs_substep", "rs_replace"])
def test_sequence(scenario):
    """ids_changed drops the id cache in both modes and the sorted index only in the deterministic one; a substep from fresh
    uploads passes through the states do_sort / do_g2p expect; drops, snapshot loads and regrown index arrays ask for the block
    flags to be cleared when they must be.  A scenario returns the line of its first failed check."""
    assert getattr(host_lib(), scenario)() == 0
