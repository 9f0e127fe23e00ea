"""A tiled job whose scene never exists on the host: 8 ranks of one partition, here as 8 ctxs on one GPU (tiled.NativeVirtualJob — the
ranks of a multi-GPU job make the same calls, one per process).  The partition is cut from histograms counted on the device
(tiled.seed_histograms: mpmhip_seed_histogram), every rank fills its own brick of a sand sphere (add_particles(region=..., brick=True):
mpmhip_seed_particles_brick — all ranks evaluate all candidates, so creation ids are global without a message), and an emitter feeds a
jet of water across a cut plane before every frame (job.add_particles: the library plans its halo boxes again at the next advance).
The per-rank counts are printed; --frames writes the job's .bgeo frames.  Needs an MI355X.

    python examples/tiled_fill.py [frames] [--frames DIR]

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
    ap.add_argument('count', nargs='?', type=int, default=4, help='frames to run')
    ap.add_argument('--frames', metavar='DIR', help='write DIR/0001.bgeo, 0002.bgeo, ... after every frame')
    args = ap.parse_args()
    frames = args.count
    r, world, margin = 64, 8, 2
    dx = 1.0 / r
    sim_cfg = dict(res=(r, r, r), delta_x=dx, base_delta_t=1e-4, gravity=(0, -10, 0))
    LS = tm.mpm.LevelSet
    ball = dict(type='sand', ppc=8, region=LS().add_sphere((0.5, 0.42, 0.5), 12 * dx), friction_angle=30)
    # the nozzle sits on the cut planes through the ball's centre; its jet crosses them sideways and downwards
    jet = dict(type='water', ppc=8, region=LS().add_sphere((0.5, 0.75, 0.5), 4 * dx), pd_source=True, delta_t=1e-3,
               initial_velocity=(-1.5, -2.0, 0.5))

    # the partition: balanced over the ball, from the device's histograms (any ctx of the grid will do; it holds no particle)
    probe = tm.create_simulation3('mpm').initialize(dict(sim_cfg))
    hists, cell_lo, cell_hi, total = tiled.seed_histograms(probe, ball)
    probe.close()
    part = tiled.Partition.from_histograms((r, r, r), world, hists, cell_lo, cell_hi, margin)
    print("%d particles to come; cuts %s" % (total, part.cuts))

    floor = LS(friction=0.4).add_plane((0, 1, 0), d=-0.2)
    sims = tiled.build_seeded_rank_sims(tm, [ball], part, levelset=floor, **sim_cfg)
    print("ball: per rank %s of %d" % ([s.seed_counts[0] for s in sims], sims[0].seed_counts[1]))
    job = tiled.NativeVirtualJob([tiled.HipEngine(s, 0) for s in sims], part)
    job.frame_directory = args.frames
    for frame in range(frames):
        added = job.add_particles(jet)  # every rank: the same call
        job.run(10)  # delta_t of the emitter = 10 substeps
        print("frame %d: jet per rank %s of %d; particles per rank %s" % (
            frame, [a for a, _ in added], added[0][1], [e.num_particles() for e in job.engines]))
        if args.frames:
            print("         wrote %s" % job.visualize())
    tot = job.totals()
    print("job: %d particles, %d migrated, error word %d" % (tot["particles"], tot["migrated"], tot["error"]))
    del job
    for s in sims:
        s.close()
