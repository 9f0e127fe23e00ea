"""Snapshot blobs byte for byte against the library of the commit before the formats got one definition (csrc/snapshot_blob.h):
tests/golden/snapshot_<scene>_in.bin was saved by that library after 20 substeps of a tiny scene, snapshot_<scene>_out.bin is what it
saved after loading `in` into a fresh simulation (tests/golden/make_snapshot_golden.py, tests/snapshot_scenes.py).  Loading `in` and
saving must give `out` exactly — the parser, the state transitions of a load and the writer in one comparison — and the loaded state
must run.  And the 3D loader, like the other two, leaves its context alone when it refuses a blob."""
import ctypes as C

import numpy as np
import pytest

from taichi_mpm_amd import _lib
from tests import snapshot_scenes as ss

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


@pytest.mark.parametrize("name", ss.SCENES)
def test_loading_a_fixture_and_saving_gives_the_recorded_bytes(tm, tmp_path, name):
    with open(ss.fixture_path(name, "out"), "rb") as f:
        want = f.read()
    sim = ss.build(tm, name, with_particles=False)
    sim.load_snapshot(ss.fixture_path(name, "in"))
    n = ss.n_particles(sim, name)
    assert n > 0
    path = str(tmp_path / "again.bin")
    sim.save_snapshot(path)
    with open(path, "rb") as f:
        got = f.read()
    assert len(got) == len(want)
    assert got == want, "first differing byte: %d" % int(np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[0])
    ss.advance(sim, name, 5)  # the loaded state is usable
    p = sim.get_pool_particles() if name.startswith("async") else sim.get_particles()
    assert len(p["x"]) >= n and np.isfinite(p["x"]).all() and np.isfinite(p["v"]).all()
    sim.close()


def test_a_3d_snapshot_with_a_table_index_out_of_range_is_refused_before_anything_is_loaded(tm, tmp_path):
    """a group of an unknown material, a joint to a body that is not there: MPMError, the particles of the simulation stay, and
    the good blob then loads (the asynchronous loader's twin: tests/test_gpu_async.py)"""
    good = ss.fixture_path("rigid3d", "in")
    raw = np.fromfile(good, np.uint8)
    h = _lib.SnapHeader.from_buffer_copy(raw[8:8 + C.sizeof(_lib.SnapHeader)].tobytes())
    groups = 8 + C.sizeof(_lib.SnapHeader)
    records = groups + C.sizeof(_lib.GroupParams) * h.n_groups
    joints = records + int(h.n_slots) * (64 + 64 + 48) + 24 + 188 * 2  # behind the records: the rigid header and the two bodies
    cases = {"material": (groups + C.sizeof(_lib.GroupParams) + _lib.GroupParams.type.offset, 99), "joint": (joints + 4, 1000)}  # JointDev.obj0
    for what, (at, word) in cases.items():
        bad = raw.copy()
        bad[at:at + 4] = np.array([word], np.int32).view(np.uint8)
        p2 = str(tmp_path / ("bad_%s.snap" % what))
        bad.tofile(p2)
        b = ss.build(tm, "rigid3d")
        b.add_particles(dict(type="jelly", positions=np.full((5, 3), 0.5, np.float32) + 0.01 * np.arange(5, dtype=np.float32)[:, None]))
        before = b.get_num_particles()
        assert before == int(h.n_slots) + 5
        with pytest.raises(tm.mpm.MPMError, match="snapshot"):
            b.load_snapshot(p2)
        assert b.get_num_particles() == before  # nothing of the blob got in
        b.load_snapshot(good)                   # ... and the ctx is still usable
        assert b.get_num_particles() == int(h.n_slots) - int(h.n_dead)
        b.run_substeps(2)
        b.close()


def test_a_file_shorter_than_a_header_is_an_mpm_error(tm, tmp_path):
    short = str(tmp_path / "short.snap")
    np.zeros(40, np.uint8).tofile(short)
    for name in ss.SCENES:
        sim = ss.build(tm, name, with_particles=False)
        with pytest.raises(tm.mpm.MPMError, match="no snapshot"):
            sim.load_snapshot(short)
        sim.close()
