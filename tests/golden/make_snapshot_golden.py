"""Generator of tests/golden/snapshot_<scene>_{in,out}.bin (tests/snapshot_scenes.py, tests/test_gpu_snapshot_compat.py).  Run ONCE
on a GPU with the library of the commit the snapshot code is compared with; not part of the suite:

    python tests/golden/make_snapshot_golden.py [output directory]

Per scene: 20 substeps, save -> `in`; a fresh simulation of the same scene loads `in` and saves -> `out`.  `out` is made twice and
nothing is written when the two differ (that scene then needs the deterministic mode).  A later library that loads `in` and saves
must give `out` byte for byte: same parsing, same state transitions of the load, same writer."""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import taichi_mpm_amd as tm  # noqa: E402
from tests import snapshot_scenes as ss  # noqa: E402

SUBSTEPS = 20


def reload_and_save(name, path_in, path_out):
    sim = ss.build(tm, name, with_particles=False)
    sim.load_snapshot(path_in)
    sim.save_snapshot(path_out)
    sim.close()
    with open(path_out, "rb") as f:
        return f.read()


def main(out_dir):
    tm.load()
    os.makedirs(out_dir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for name in ss.SCENES:
            a = ss.build(tm, name)
            ss.advance(a, name, SUBSTEPS)
            path_in = os.path.join(tmp, name + ".in")
            a.save_snapshot(path_in)
            n = ss.n_particles(a, name)
            a.close()
            first = reload_and_save(name, path_in, os.path.join(tmp, name + ".out1"))
            second = reload_and_save(name, path_in, os.path.join(tmp, name + ".out2"))
            if first != second:
                raise SystemExit("%s: two reloads of the same blob save different bytes; no fixture written" % name)
            with open(path_in, "rb") as f:
                blob_in = f.read()
            for which, data in (("in", blob_in), ("out", first)):
                assert len(data) < (1 << 20), (name, which, len(data))
                with open(os.path.join(out_dir, os.path.basename(ss.fixture_path(name, which))), "wb") as f:
                    f.write(data)
            print("%s: %d particles / containers, in %d bytes, out %d bytes, in == out: %s" % (name, n, len(blob_in), len(first), blob_in == first))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden"))
