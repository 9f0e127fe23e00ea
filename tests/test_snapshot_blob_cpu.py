"""The three snapshot formats as data (taichi_mpm_amd/csrc/snapshot_blob.h: header structs, record geometry, one layout and one check
function per format) compiled for the host by g++, the header alone: no HIP header is included, no HIP runtime linked or loaded
(tests/cpp/snapshot_blob_host.cpp).  The scenarios build the smallest blobs that have every section in heap buffers of exactly their
size and hold the layouts against offsets written out by hand, the checks against every truncation, single-field corruptions with
their messages, and a sweep of every header byte.  The same source, with its main(), runs once as a program of its own under
AddressSanitizer and UBSan: no header value leads to a read outside the blob.  And the ctypes mirrors of the headers
(taichi_mpm_amd/_lib.py), through which the Python loaders read a blob, match the structs field by field.  No GPU needed."""
import ctypes as C
import os
import subprocess

import pytest

from taichi_mpm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "snapshot_blob_host.cpp")
CSRC = os.path.join(ROOT, "taichi_mpm_amd", "csrc")
HDRS = [os.path.join(CSRC, h) for h in ("snapshot_blob.h", "async_sched.h", "group_params.h")] + [os.path.join(ROOT, "include", "mpmhip.h")]
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "libsnapshot_blob_host.so")
SAN = os.path.join(ROOT, "tests", "cpp", "_build", "snapshot_blob_host_san")
SCENARIOS = ["sb_offsets", "sb_accept", "sb_truncation", "sb_corrupt_3d", "sb_corrupt_async", "sb_corrupt_2d", "sb_sweep"]


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
def test_blob(scenario):
    """sb_offsets: every section of the three blobs, and the total, at offsets written out by hand.  sb_accept: the three blobs pass;
    so do a 3D blob without rigid section, one without the collision tail, one with trailing bytes.  sb_truncation: every length
    below the total is refused, but for the two 3D lengths that end before an optional tail.  sb_corrupt_*: one field wrong at a
    time — magic, abi, grid, dx, dt, negative and overflowing counts, group ids, creation ids, block tags, limits, joint bodies,
    materials, body counts, stepper or not — each refused with its message.  sb_sweep: every header byte at 0x00, 0x7F, 0xFF.
    A scenario returns the line of its first failed check in tests/cpp/snapshot_blob_host.cpp."""
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
    """sizeof and the offset of every field of SnapHeader, SnapAsync, Snap2D and GroupParams as g++ lays out snapshot_blob.h, against
    the ctypes mirrors of taichi_mpm_amd/_lib.py"""
    pairs = [("snap::SnapHeader", _lib.SnapHeader), ("snap::SnapAsync", _lib.SnapAsync), ("snap::Snap2D", _lib.Snap2DHeader),
             ("mpm::GroupParams", _lib.GroupParams)]
    lines = ["#include <cstdio>", "#include <cstddef>", '#include "snapshot_blob.h"', "int main() {"]
    for cname, mirror in pairs:
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in mirror._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ["  return 0;", "}"]
    src = tmp_path / "snap_abi.cpp"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "snap_abi"
    subprocess.check_call(["g++", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])
    got = {}
    for ln in subprocess.check_output([str(exe)], text=True).splitlines():
        c, f, v = ln.split()
        got[(c, f)] = int(v)
    for cname, mirror in pairs:
        assert got[(cname, "size")] == C.sizeof(mirror), (cname, got[(cname, "size")], C.sizeof(mirror))
        for fname, _ in mirror._fields_:
            assert got[(cname, fname)] == getattr(mirror, fname).offset, (cname, fname)
    assert _lib.NPARAM * 4 == _lib.GroupParams.type.offset


def test_a_file_shorter_than_its_header_is_an_mpm_error(tmp_path):
    """the Python loaders read the header through the mirrors: a short file is an MPMError, not a numpy error"""
    from taichi_mpm_amd.mpm import MPMError, read_snapshot, snapshot_groups
    for mirror, words in ((_lib.SnapHeader, 1), (_lib.SnapAsync, 1), (_lib.Snap2DHeader, 2)):
        for size in (0, 5, 8 * words + C.sizeof(mirror) - 1):
            path = tmp_path / ("short_%d" % size)
            path.write_bytes(bytes(size))
            with pytest.raises(MPMError, match="no snapshot"):
                read_snapshot(str(path), mirror, words)
    # ... and a fixture's header and group table come out through them
    fixture = os.path.join(ROOT, "tests", "golden", "snapshot_rigid3d_in.bin")
    (frame,), blob, h = read_snapshot(fixture, _lib.SnapHeader)
    assert h.magic == b"MPMHIP01" and h.abi == 3 and h.n_groups == 2 and h.n_slots == 64 and tuple(h.res) == (16, 16, 16)
    from taichi_mpm_amd import MATERIAL_IDS
    assert [g[0] for g in snapshot_groups(blob, h)] == [MATERIAL_IDS["elastic"], MATERIAL_IDS["sand"]]


class Facts(C.Structure):
    """mirror of snap::Facts (what a context contributes to a check)"""
    _fields_ = [("res", C.c_int32 * 3), ("dx", C.c_float), ("dt", C.c_float), ("capacity", C.c_int64), ("groups_cap", C.c_int64),
                ("n_bodies", C.c_int64), ("nb", C.c_int32 * 3), ("nblk", C.c_int64), ("unit_delta_t", C.c_float), ("resident", C.c_bool),
                ("n_boundary", C.c_uint64)]


@pytest.mark.parametrize("name,kind,lead,facts", [
    ("rigid3d", 0, 8, dict(res=(16, 16, 16), dx=1 / 16, dt=1e-4, capacity=256, groups_cap=64, n_bodies=2)),
    ("async3d", 1, 8, dict(res=(16, 16, 16), dx=1 / 16, unit_delta_t=2e-6, groups_cap=64, nb=(5, 5, 3), nblk=75)),
    ("rigid2d", 2, 16, dict(res=(32, 32, 0), dx=1 / 32, n_bodies=2, n_boundary=1 << 20)),
    ("async2d", 2, 16, dict(res=(32, 32, 0), dx=1 / 32, unit_delta_t=2e-6, resident=True, nb=(5, 3, 0), nblk=15))])
def test_the_recorded_blobs_pass_their_check(name, kind, lead, facts):
    """tests/golden/snapshot_*.bin, saved on a GPU by the library as it was before this header existed, pass the host check with
    the facts of their scenes (tests/snapshot_scenes.py) — and not with another grid"""
    lib = host_lib()
    lib.sb_check.restype = C.c_char_p
    lib.sb_check.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.POINTER(Facts)]
    f = Facts()
    for k, v in facts.items():
        if isinstance(v, tuple):
            getattr(f, k)[:] = v
        else:
            setattr(f, k, v)
    for which in ("in", "out"):
        with open(os.path.join(ROOT, "tests", "golden", "snapshot_%s_%s.bin" % (name, which)), "rb") as fh:
            blob = fh.read()[lead:]
        assert lib.sb_check(kind, blob, len(blob), C.byref(f)) == b""
        f.res[0] += 1
        assert b"grid" in lib.sb_check(kind, blob, len(blob), C.byref(f))
        f.res[0] -= 1
