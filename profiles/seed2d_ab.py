"""Seeding the 2D solver on the device against uploading sampled positions (profiles/seed2d_ab.txt).

  python profiles/seed2d_ab.py     one fill — a disc of r = 292 dx at 1024^2, ppc 4: about 1 M particles — through
                                   add_particles(region=...) and through add_particles(positions=<the same points>), the only path
                                   before mpmhip2d_seed_particles, alternating: one warm-up and REPEATS timed calls each, medians.
                                   A call is timed by the host clock from the call to the end of a device synchronise, on a ctx
                                   created (and sized) beforehand.  The points of the positions= calls are the region= call's own
                                   output, downloaded once: sampling them on the host is not part of any number.
  python profiles/seed2d_ab.py --sampled   the same disc baked on the grid's nodes (1025^2 samples, uploaded by every call): the
                                   region is read by the boundary's sampler.  (Under MPMHIP_LIB_VARIANT=parent: the parent's library.)
A set-up cost: there is no target."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS = 5
RES, R_CELLS, CAP = 1024, 292, 1 << 21


def timed_fill(tm, want_x=False, **how):
    sim = tm.create_simulation2("mpm").initialize(dict(res=(RES, RES), delta_x=1.0 / RES, base_delta_t=1e-4, max_particles=CAP))
    sim._ensure_ctx()
    sim.synchronize()
    t0 = time.perf_counter()
    sim.add_particles(dict(type="sand", ppc=4, **how))
    sim.synchronize()
    dt = time.perf_counter() - t0
    n = sim.get_num_particles()
    x = sim.get_particles(sort_by_id=False)["x"] if want_x else None
    sim.close()
    return dt, n, x


def main():
    import taichi_mpm_amd as tm
    tm.load()
    disc = tm.LevelSet().add_sphere((0.5, 0.5, 0.0), R_CELLS / RES)
    if "--sampled" in sys.argv[1:]:
        disc = tm.SampledLevelSet2D.from_levelset(disc, (RES + 1, RES + 1), (0.0, 0.0), 1.0 / RES)
    _, n, x = timed_fill(tm, want_x=True, region=disc)  # (also the warm-up of the region= path)
    timed_fill(tm, positions=x)
    tr, tp = [], []
    for _ in range(REPEATS):
        r = timed_fill(tm, region=disc)
        p = timed_fill(tm, positions=x)
        assert r[1] == p[1] == n, (r[1], p[1], n)
        tr.append(r[0])
        tp.append(p[0])
    n_tile = int(tm.load().mpmhip2d_poisson_tile(None, 0))
    print("%sdisc r = %d dx at %d^2, ppc 4: %d particles (%.3f per cell of the disc; tile of %d points)" % (
        "sampled " if "--sampled" in sys.argv[1:] else "", R_CELLS, RES, n, n / (np.pi * R_CELLS ** 2), n_tile))
    for label, t, moved in (("region=   ", tr, 0), ("positions=", tp, n * 60)):
        print("  %s median %9.3f ms   min %9.3f   max %9.3f   (%d calls)   particle bytes through the host: %d" % (
            label, 1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t), len(t), moved))
    print("  ratio of the medians: %.1f" % (statistics.median(tp) / statistics.median(tr)))


if __name__ == "__main__":
    main()
