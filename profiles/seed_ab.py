"""Seeding on the device against uploading sampled positions (profiles/seed_ab.txt).

  python profiles/seed_ab.py                 the table: two fills, each through add_particles(region=...) and through
                                             add_particles(positions=<the numpy model's output>) — the only path before
                                             mpmhip_seed_particles — alternating, one warm-up and REPEATS timed calls each, medians.
                                             A call is timed by the host clock from the call to the end of a device synchronise, on a
                                             ctx created (and sized) beforehand; the model's own time is not part of any number.
  python profiles/seed_ab.py --region-only --fill N   just the region= calls of one fill: what a `rocprofv3 --kernel-trace --stats`
                                             run wraps
  python profiles/seed_ab.py --stats FILE    per-kernel table of that run's kernel_stats.csv

Fills: a sand block of about 8 M particles at 256^3 (a cuboid of 108^3 cells, shapes), and the r = 12 dx sphere of the tests at 64^3
(a sampled field of 60^3 samples, uploaded by every call)."""
import argparse
import csv
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS = 5


def fills(tm):
    from tests.seed_model import SampledRegion, ShapeRegion
    dx = 1.0 / 256
    lo, hi = 74.3 * dx, 182.3 * dx
    block = tm.mpm.LevelSet().add_cuboid((lo,) * 3, (hi,) * 3)
    dx64 = 1.0 / 64
    c = np.array([0.5, 0.5, 0.5])
    origin = tuple(np.float32(0.5 - 14.3 * dx64 + 0.0137 * dx64) for _ in range(3))
    sphere = tm.mpm.SampledLevelSet.from_function(lambda x: np.linalg.norm(x - c, axis=1) - 12 * dx64, (60, 60, 60), origin, dx64 / 2)
    return [("block 108^3 cells at 256^3", 256, dx, block, lambda: ShapeRegion(block.shapes, dx), 12 << 20),
            ("sphere r = 12 dx at 64^3", 64, dx64, sphere, lambda: SampledRegion(sphere.phi, sphere.origin, sphere.spacing, dx64), 1 << 17)]


def timed_fill(tm, res, dx, cap, **how):
    sim = tm.create_simulation3("mpm").initialize(dict(res=(res,) * 3, delta_x=dx, base_delta_t=1e-4, max_particles=cap))
    sim._ensure_ctx()
    sim.synchronize()
    bytes0 = sim._L.mpmhip_host_particle_bytes(sim._ctx)
    t0 = time.perf_counter()
    sim.add_particles(dict(type="sand", ppc=8, **how))
    sim.synchronize()
    dt = time.perf_counter() - t0
    n = sim.get_num_particles()
    moved = sim._L.mpmhip_host_particle_bytes(sim._ctx) - bytes0
    x = sim.get_particles(sort_by_id=False)["x"] if res == 64 else None
    sim.close()
    return dt, n, moved, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--region-only", action="store_true")
    ap.add_argument("--fill", type=int, default=-1, help="only this fill (0 the block, 1 the sphere)")
    ap.add_argument("--stats")
    a = ap.parse_args()
    if a.stats:
        rows = [r for r in csv.DictReader(open(a.stats)) if r["Name"].startswith("mpm::k_seed") or "k_seed" in r["Name"]]
        total = sum(float(r["TotalDurationNs"]) for r in rows)
        print("kernels of %d region= calls (rocprofv3 --kernel-trace --stats, a run of its own):" % (REPEATS + 1))
        for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
            print("  %-16s %4d x  mean %10.2f us  min %10.2f  max %10.2f   %5.1f %%" % (
                r["Name"].split("(")[0].replace("mpm::", ""), int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3,
                float(r["MaxNs"]) / 1e3, 100 * float(r["TotalDurationNs"]) / total))
        return
    import taichi_mpm_amd as tm
    from tests.seed_model import SeedModel
    tm.load()
    for i, (name, res, dx, region, model_region, cap) in enumerate(fills(tm)):
        if a.fill >= 0 and i != a.fill:
            continue
        if a.region_only:
            for _ in range(REPEATS + 1):
                timed_fill(tm, res, dx, cap, region=region)
            continue
        t0 = time.perf_counter()
        m = SeedModel(res, dx, model_region(), ppc=8.0)
        want = m.run()["x"]
        t_model = time.perf_counter() - t0
        tr, tp = [], []
        for k in range(REPEATS + 1):
            r = timed_fill(tm, res, dx, cap, region=region)
            p = timed_fill(tm, res, dx, cap, positions=want)
            assert r[1] == p[1] == len(want), (r[1], p[1], len(want))
            assert r[2] == 0 and p[2] == len(want) * 176, (r[2], p[2])
            if r[3] is not None:
                assert r[3].tobytes() == want.tobytes() == p[3].tobytes()
            if k:
                tr.append(r[0])
                tp.append(p[0])
        print("%s: %d candidates, %d particles (the numpy model: %.1f s, not counted)" % (name, m.n_cand, len(want), t_model))
        for label, t, moved in (("region=   ", tr, 0), ("positions=", tp, len(want) * 176)):
            print("  %s median %9.3f ms   min %9.3f   max %9.3f   (%d calls)   particle bytes through the host: %d" % (
                label, 1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t), len(t), moved))
        print("  ratio of the medians: %.1f" % (statistics.median(tp) / statistics.median(tr)))


if __name__ == "__main__":
    main()
