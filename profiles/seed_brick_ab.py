"""What a rank of a tiled job pays to fill its brick on the device ("Tiled jobs"; profiles/seed_ab.txt).

  python profiles/seed_brick_ab.py      two fills — a sand block of 54^3 cells (about 1 M particles) and one of 108^3 cells (about 8 M)
                                        at 256^3, ppc 8 — each three ways, alternating, one warm-up and REPEATS timed calls, medians:
                                          one ctx     add_particles(region=...)                mpmhip_seed_particles
                                          rank 0 of 8 add_particles(region=..., brick=True)    mpmhip_seed_particles_brick
                                          histogram   tiled.seed_histograms                    mpmhip_seed_histogram
                                        A call is timed by the host clock from the call to the end of a device synchronise, on a ctx
                                        created (and sized) beforehand, as profiles/seed_ab.py times its fills.

Every rank evaluates all candidates, so the brick call is expected to cost what the one-ctx call costs less the records it does not
write; the figures are information, not a gate."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS = 5
RES = 256


def timed(tm, tiled, cfg, how, part, cap):
    sim = tm.create_simulation3("mpm").initialize(dict(res=(RES,) * 3, delta_x=1.0 / RES, base_delta_t=1e-4, max_particles=cap))
    sim._ensure_ctx()
    if how == "brick":
        tiled.set_partition(sim, part, 0)
    sim.synchronize()
    t0 = time.perf_counter()
    if how == "hist":
        out = tiled.seed_histograms(sim, cfg)[3]
    else:
        sim.add_particles(dict(cfg, brick=True) if how == "brick" else cfg)
        out = sim.seed_counts[0] if how == "brick" else None
    sim.synchronize()
    dt = time.perf_counter() - t0
    if out is None:
        out = sim.get_num_particles()
    sim.close()
    return dt, out


def main():
    import taichi_mpm_amd as tm
    from taichi_mpm_amd import tiled
    tm.load()
    dx = 1.0 / RES
    for cells, cap in ((54, 2 << 20), (108, 12 << 20)):
        lo = (RES / 2 - cells / 2 + 0.3) * dx
        cfg = dict(type="sand", ppc=8, region=tm.mpm.LevelSet().add_cuboid((lo,) * 3, (lo + cells * dx,) * 3))
        probe = tm.create_simulation3("mpm").initialize(dict(res=(RES,) * 3, delta_x=dx, base_delta_t=1e-4, max_particles=1024))
        hists, clo, chi, total = tiled.seed_histograms(probe, cfg)
        probe.close()
        part = tiled.Partition.from_histograms((RES,) * 3, 8, hists, clo, chi, margin=4)
        t = {"one": [], "brick": [], "hist": []}
        n = {}
        for k in range(REPEATS + 1):
            for how in t:
                dt, n[how] = timed(tm, tiled, cfg, how, part, cap)
                if k:
                    t[how].append(dt)
        assert n["one"] == n["hist"] == total and 0 < n["brick"] < total, n
        print("block of %d^3 cells at %d^3: %d particles, %d on rank 0 of 8 (cuts %s)" % (cells, RES, total, n["brick"], [c[1] for c in part.cuts]))
        for how, label in (("one", "one ctx    "), ("brick", "rank 0 of 8"), ("hist", "histogram  ")):
            print("  %s median %8.3f ms   min %8.3f   max %8.3f   (%d calls)" % (
                label, 1e3 * statistics.median(t[how]), 1e3 * min(t[how]), 1e3 * max(t[how]), len(t[how])))


if __name__ == "__main__":
    main()
