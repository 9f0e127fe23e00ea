"""Bodies on a tiled job: the scene of examples/sand_paddle.py (a scripted paddle wheel in a block of sand on a floor; here at
res 128, the sand seeded on the device) per substep, as ONE ctx and as 8 virtual ranks of the same partition on one GPU.  Host clock
around runs of --steps substeps that end in a synchronise, --runs runs each, after --warmup substeps.

What the two row exchanges cost (k_rigid_row_out, k_rigid_rows_world; deterministic: + k_rigid_rows_sum): run the script under
`rocprofv3 --kernel-trace --stats` and read those rows of the kernel statistics against the total — the script prints the names.
The 8 ranks of a virtual job share one stream, so their kernels run one behind the other: "per rank" is the job's time over 8.
Nothing here has been on more than one GPU.  The record: profiles/cpic_job_ab.txt.

    python profiles/cpic_job_ab.py [--res 128] [--steps 100] [--runs 3] [--warmup 20] [--deterministic]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import taichi_mpm_amd as tm  # noqa: E402
from taichi_mpm_amd import tiled  # noqa: E402


def paddle(r=0.16, h=0.10):
    a = np.array([[[-r, -h, 0], [r, -h, 0], [r, h, 0]], [[-r, -h, 0], [r, h, 0], [-r, h, 0]]], np.float32)
    return np.concatenate([a, a[:, :, [2, 1, 0]]])


def timed(runs, fn):
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--deterministic", action="store_true")
    args = ap.parse_args()
    tm.load()
    r, world, margin = args.res, 8, 2
    dx = 1.0 / r
    sim_cfg = dict(res=(r, r, r), delta_x=dx, base_delta_t=1e-4, gravity=(0, -10, 0), penalty=1e4, deterministic=args.deterministic)
    LS = tm.mpm.LevelSet
    lo, hi = 40.0 / 128, 88.0 / 128  # the cube of sand_paddle.py
    sand = dict(type="sand", ppc=8, region=LS().add_cuboid((lo,) * 3, (hi,) * 3), friction_angle=30)
    wheel = dict(type="rigid", mesh=paddle(), codimensional=True, friction=-2, density=500,
                 scripted_position=lambda t: (0.5, 0.34, 0.5), scripted_rotation=lambda t: (0.0, 360.0 * t, 0.0))
    floor = LS(friction=-1).add_plane((0, 1, 0), d=-0.2)

    one = tm.create_simulation3("mpm").initialize(dict(sim_cfg))
    one.set_levelset(floor)
    hists, cell_lo, cell_hi, total = tiled.seed_histograms(one, sand)
    one.add_particles(dict(wheel))
    one.add_particles(dict(sand))
    n = one.get_num_particles()
    one.run_substeps(args.warmup)
    one.synchronize()

    def run_one():
        one.run_substeps(args.steps)
        one.synchronize()
    ms = timed(args.runs, run_one)
    print("one ctx, %d particles: ms per substep %s (min %.4f)" % (n, " ".join("%.4f" % (v / args.steps) for v in ms), min(ms) / args.steps), flush=True)
    one.close()

    part = tiled.Partition.from_histograms((r, r, r), world, hists, cell_lo, cell_hi, margin)
    sims = tiled.build_seeded_rank_sims(tm, [sand], part, levelset=floor, bodies=[wheel], **sim_cfg)
    job = tiled.NativeVirtualJob([tiled.HipEngine(s, 0) for s in sims], part)
    job.run(args.warmup)
    job.synchronize()

    def run_job():
        job.run(args.steps)
        job.synchronize()
    ms = timed(args.runs, run_job)
    per = min(ms) / args.steps
    print("8 virtual ranks, particles per rank %s: ms per substep of the job %s (min %.4f, per rank %.4f)" % (
        [e.num_particles() for e in job.engines], " ".join("%.4f" % (v / args.steps) for v in ms), per, per / world), flush=True)
    tot = job.totals()
    print("job: %d particles, %d migrated, error word %d, replicas one: %s" % (tot["particles"], tot["migrated"], tot["error"],
                                                                              len(set(job.rigid_digests())) == 1))
    print("row exchanges: 2 per substep and rank = %d launches of k_rigid_row_out and of k_rigid_rows_world in the timed runs"
          % (2 * world * args.steps * args.runs))
    del job
    for s in sims:
        s.close()
