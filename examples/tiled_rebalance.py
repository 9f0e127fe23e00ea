"""The job of examples/tiled_fill.py — 8 ranks of one partition as 8 ctxs on one GPU, a sand ball seeded brick by brick and a jet of
water poured across the cut planes, the ball here thrown sideways — with the bricks re-cut from the live particles after every frame (job.rebalance: the live
histograms counted on the device, mpmhip_live_histogram; new cuts, tiled.Partition.from_histograms; the set-up again; every particle
to its new owner, mpmhip_tiled_redistribute).  The per-rank counts are printed before and after each re-cut.  The ranks of a
multi-GPU job make the same calls, one per process (tiled.NativeTiledJob.rebalance is the collective).  Needs an MI355X.

    python examples/tiled_rebalance.py [frames] [--frames DIR]

--frames DIR: job.visualize() after every frame — DIR/0001.bgeo, 0002.bgeo, ...: ONE file per frame for all 8 ranks, the rows in
ascending creation id (the ids are ranked on the device, mpmhip_bgeo_encode_group).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import taichi_mpm_amd as tm  # noqa: E402
from taichi_mpm_amd import tiled  # noqa: E402

if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('count', nargs='?', type=int, default=10, help='frames to run')
    ap.add_argument('--frames', metavar='DIR', help='write DIR/0001.bgeo, 0002.bgeo, ... after every frame')
    args = ap.parse_args()
    frames = args.count
    r, world, margin = 64, 8, 2
    dx = 1.0 / r
    sim_cfg = dict(res=(r, r, r), delta_x=dx, base_delta_t=1e-4, gravity=(0, -10, 0))
    LS = tm.mpm.LevelSet
    # (the ball is thrown sideways, half a cell per frame: it leaves the bricks it was cut for, and the cut planes follow it)
    ball = dict(type='sand', ppc=8, region=LS().add_sphere((0.5, 0.42, 0.5), 12 * dx), friction_angle=30, initial_velocity=(8.0, 0.0, 0.0))
    # (a wider nozzle than tiled_fill's: within a few frames the bricks under it hold visibly more than the others)
    jet = dict(type='water', ppc=8, region=LS().add_sphere((0.5, 0.75, 0.5), 7 * dx), pd_source=True, delta_t=1e-3,
               initial_velocity=(-1.5, -2.0, 0.5))

    probe = tm.create_simulation3('mpm').initialize(dict(sim_cfg))
    hists, cell_lo, cell_hi, total = tiled.seed_histograms(probe, ball)
    probe.close()
    part = tiled.Partition.from_histograms((r, r, r), world, hists, cell_lo, cell_hi, margin)
    print("%d particles to come; cuts %s" % (total, part.cuts))

    floor = LS(friction=0.4).add_plane((0, 1, 0), d=-0.2)
    sims = tiled.build_seeded_rank_sims(tm, [ball], part, levelset=floor, **sim_cfg)
    job = tiled.NativeVirtualJob([tiled.HipEngine(s, 0) for s in sims], part)
    job.frame_directory = args.frames
    for frame in range(frames):
        job.add_particles(jet)  # every rank: the same call; the jet lands in the bricks under the nozzle
        job.run(10)  # delta_t of the emitter = 10 substeps
        before = [e.num_particles() for e in job.engines]
        res = job.rebalance()  # (threshold 1.15: a frame that left the ranks level costs one histogram per rank)
        after = [e.num_particles() for e in job.engines]
        print("frame %d: per rank %s (max / mean %.3f)" % (frame, before, res["imbalance_before"]))
        if res["recut"]:
            print("         re-cut %s: per rank %s (max / mean %.3f), %d records moved in %d round(s)%s" % (
                res["cuts"], after, res["imbalance_after"], res["moved"], res["rounds"],
                ", ranks %s grew" % res["grew"] if res["grew"] else ""))
        if args.frames:
            print("         wrote %s" % job.visualize())
    tot = job.totals()
    print("job: %d particles after %d substeps, error word %d" % (tot["particles"], job.substeps, tot["error"]))
    del job
    for s in sims:
        s.close()
