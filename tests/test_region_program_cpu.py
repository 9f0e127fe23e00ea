"""The check of a region expression (taichi_mpm_amd/csrc/region_program.h: limits, indices, the stack discipline of the postfix
program, placements, bands, lattices) compiled for the host by g++, the header alone: no HIP header is included, no HIP runtime
linked or loaded (tests/cpp/region_program_host.cpp).  The scenarios accept the programs of the GPU tests, refuse every malformed
description one fault at a time with its message, and sweep every byte of valid descriptions.  The same source, with its main(),
runs once as a program of its own under AddressSanitizer and UBSan: no value in a description leads to a read outside it.  And
the ctypes mirrors of the description (taichi_mpm_amd/_lib.py) match the structs field by field.  No GPU needed."""
import ctypes as C
import os
import subprocess

import pytest

from taichi_mpm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "region_program_host.cpp")
CSRC = os.path.join(ROOT, "taichi_mpm_amd", "csrc")
HDRS = [os.path.join(CSRC, h) for h in ("region_program.h", "sdf_lattice.h")] + [os.path.join(ROOT, "include", "mpmhip.h")]
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "libregion_program_host.so")
SAN = os.path.join(ROOT, "tests", "cpp", "_build", "region_program_host_san")
SCENARIOS = ["rp_accept", "rp_refuse_program", "rp_refuse_leaves", "rp_refuse_fields", "rp_sweep"]


def _stale(out):
    return not os.path.exists(out) or max(os.path.getmtime(f) for f in [SRC] + HDRS) > os.path.getmtime(out)


def host_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if _stale(OUT):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", SRC, "-o", OUT])
    return C.CDLL(OUT)


def test_the_test_library_does_not_pull_in_the_hip_runtime():
    host_lib()
    needed = subprocess.check_output(["readelf", "-d", OUT], text=True)
    assert "amdhip64" not in needed and "libhsa" not in needed, needed


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_check(scenario):
    """rp_accept: the programs of the GPU tests pass for D = 2 and 3, the sample counts come back, a program at every limit passes.
    rp_refuse_program: empty, too long, too many leaves or fields, leaf and field indices out of range, underflow at a binary
    operator and at a complement, depth 5, two values left, unknown opcode, kind and shape type.  rp_refuse_leaves: rotations that
    are not finite or not orthonormal (D = 2: the angle), scales <= 0 or not finite, non-finite translation and pivot, bands with
    lo >= hi or a NaN edge — and that fields of a leaf that is not placed or banded are not read.  rp_refuse_fields: what
    sdf_lattice::check refuses, a missing array.  rp_sweep: every byte of five valid descriptions at 0x00, 0x7F, 0xFF.
    A scenario returns the line of its first failed check in tests/cpp/region_program_host.cpp."""
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


def test_ctypes_mirrors_match_the_header_structs_field_by_field(tmp_path):
    pairs = [("mpmhip_region_leaf", _lib.RegionLeaf), ("mpmhip_region_op", _lib.RegionOp), ("mpmhip_region_field", _lib.RegionField),
             ("mpmhip_region_desc", _lib.RegionDesc)]
    lines = ["#include <cstdio>", "#include <cstddef>", '#include "mpmhip.h"', "int main() {"]
    for cname, mirror in pairs:
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in mirror._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('  printf("limits %d %d\\n", MPMHIP_REGION_MAX_LEAVES * 1000 + MPMHIP_REGION_MAX_FIELDS * 100 + MPMHIP_REGION_MAX_OPS, MPMHIP_REGION_MAX_DEPTH);')
    lines.append('  printf("codes %d %d\\n", MPMHIP_REGION_PUSH * 1000 + MPMHIP_REGION_UNION * 100 + MPMHIP_REGION_INTERSECT * 10 + MPMHIP_REGION_NEG, 0);')
    lines += ["  return 0;", "}"]
    src = tmp_path / "region_abi.cpp"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "region_abi"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {}
    for ln in subprocess.check_output([str(exe)], text=True).splitlines():
        c, f, v = ln.split()
        got[(c, f)] = int(v)
    for cname, mirror in pairs:
        assert got[(cname, "size")] == C.sizeof(mirror), (cname, got[(cname, "size")], C.sizeof(mirror))
        for fname, _ in mirror._fields_:
            assert got[(cname, fname)] == getattr(mirror, fname).offset, (cname, fname)
    assert got[("limits", str(_lib.REGION_MAX_LEAVES * 1000 + _lib.REGION_MAX_FIELDS * 100 + _lib.REGION_MAX_OPS))] == _lib.REGION_MAX_DEPTH
    assert ("codes", str(_lib.REGION_PUSH * 1000 + _lib.REGION_UNION * 100 + _lib.REGION_INTERSECT * 10 + _lib.REGION_NEG)) in got
