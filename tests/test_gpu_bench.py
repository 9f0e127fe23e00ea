"""bench.py on the device: a plain run prints the headline and nothing else, --full adds the measurements on top, and
--dump-outputs writes the particle state the timed substeps left — bit for bit the state a caller of the library gets after the
same substeps in the deterministic mode, the mode a dumping run steps in (run with -m gpu on an MI355X).  A reduced C2 scene
(16^3 cells x 8 = 32 768 jelly particles: the whole state is the sample) keeps each run short."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
            "data", "config"}


def _bench(*extra):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MPMHIP_FORCE_TILED", "MPMHIP_BENCH_BACKEND"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c2", "--cells", "16"] + list(extra),
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_the_state_its_timed_substeps_left(tmp_path):
    d = _bench("--steps", "6", "--warmup", "2", "--dump-outputs", str(tmp_path))
    assert set(d) == HEADLINE  # (no phase table, roofline or extra object: those are --full)
    assert d["steps"] == 6 and d["warmup"] == 2 and d["unit"] == "particle-steps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and "REDUCED" in d["config"]["workload"] and d["config"]["deterministic"] is True
    n = d["config"]["particles"]
    assert n == 16 ** 3 * 8 and np.isclose(d["value"], n / (d["ms_per_step"] * 1e-3), rtol=1e-9)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"x", "v", "B", "F", "aux", "gid", "id", "states"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    np.testing.assert_array_equal(got["id"], np.arange(n))
    # the same scene stepped through the library in another process: warm-up + timed substeps, the same bits
    import taichi_mpm_amd as tm

    import bench
    sim = bench.build_sim(tm, dict(bench.CONFIGS["c2"], cells=16, deterministic=True), 0)
    sim.run_substeps(2)
    sim.run_substeps(6)
    sim.synchronize()
    want = sim.get_particles()
    sim.close()
    for k in got:
        np.testing.assert_array_equal(got[k], want[k].astype(got[k].dtype), err_msg=k)


def test_full_run_adds_the_measurements_to_the_headline():
    d = _bench("--steps", "8", "--warmup", "2", "--full", "--no-cpu-baseline")
    assert HEADLINE < set(d) and d["steps"] == 8 and d["config"]["deterministic"] is False
    assert d["roofline"]["kernel"] in ("k_g2p", "k_g2p_packed", "k_p2g") and d["roofline"]["launches_timed"] > 0
    assert set(d["phases_ms_per_step"]) >= {"sort", "p2g", "grid", "g2p"}
    assert d["deterministic"]["ms_per_step"] > 0 and d["evolved"]["ms_per_step"] > 0
    assert "cpu_baseline" not in d and "virtual" not in d and "c5" not in d  # (--no-cpu-baseline; virtual / c5: the C3 line only)
