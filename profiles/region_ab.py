"""Seeding a region expression against seeding a plain region (profiles/seed_ab.txt, "Region expressions").

  python profiles/region_ab.py     the table: fills at 64^3, ppc 8, through add_particles(region=...), alternating, one warm-up and
                                   REPEATS timed calls each, medians.  A call is timed as profiles/seed_ab.py times it: by the host
                                   clock from the call to the end of a device synchronise, on a ctx created and sized beforehand.

Fills: the sampled r = 12 dx sphere as a plain region and as the expression of that one leaf (the same particles: what the evaluator
costs over SeedRegion); program (a) sampled sphere minus sampled sphere (two arrays uploaded); program (b) one array, two leaves, one
placed; the clipped shell of three shape leaves; a union of eight placed boxes (every leaf slot, a left-deep chain)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
REPEATS = 5


def main():
    import taichi_mpm_amd as tm
    from seed_ab import timed_fill
    from tests.region_scenes import BOX_HI, BOX_LO, DX, R12, sampled_ball, sampled_scenes, shape_scenes
    tm.load()
    Region, LS = tm.mpm.Region, tm.mpm.LevelSet
    sls = sampled_ball(tm, (0.5, 0.5, 0.5), R12)
    sampled, shapes = sampled_scenes(tm, 3), shape_scenes(tm, 3)
    box = Region(LS().add_cuboid(tuple(0.5 * v for v in BOX_LO), tuple(0.5 * v for v in BOX_HI)))
    eight = None
    for k in range(8):
        b = box.placed(rotate=((0, 0, 1), 11.0 * k), translate=(0.3 + 0.4 * (k % 2), 0.3 + 0.4 * ((k // 2) % 2), 0.3 + 0.4 * (k // 4)))
        eight = b if eight is None else eight | b
    fills = [("sampled sphere, plain region", sls), ("sampled sphere, Region of one leaf", Region(sls)), ("program (a), 2 sampled leaves", sampled["a"]),
             ("program (b), 2 leaves of one array", sampled["b"]), ("clipped shell, 3 shape leaves", shapes["clipped_shell"][0]),
             ("eight placed boxes, 8 shape leaves", eight)]
    times, counts = {name: [] for name, _ in fills}, {}
    for k in range(REPEATS + 1):
        for name, region in fills:
            dt, n, moved, x = timed_fill(tm, 64, DX, 1 << 17, region=region)
            assert moved == 0
            counts[name] = n
            if k:
                times[name].append(dt)
    for name, _ in fills:
        t = times[name]
        print("  %-38s %6d particles   median %7.3f ms   min %7.3f   max %7.3f   (%d calls)" % (
            name, counts[name], 1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t), len(t)))


if __name__ == "__main__":
    main()
