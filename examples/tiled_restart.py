"""Checkpoint and restart of a tiled job on another rank count.  The scene of examples/tiled_rebalance.py — a sand ball seeded brick by
brick and thrown sideways, a jet of water poured across the cut planes — runs for a few frames on 8 ranks (8 ctxs on one GPU) and
saves ONE snapshot file of the whole job (job.save_snapshot: the blob a single simulation holding all particles in id order would
save — no dead slot, the same bytes whatever the bricks).  A fresh job of 3 ranks then cuts its bricks from the file
(tiled.snapshot_histograms: counted on the device from staged chunks of the blob, before any rank holds a particle), loads it
(job.load_snapshot: every rank keeps the records of its own brick) and runs on.  The ranks of a multi-GPU job make the same calls,
one per process.  Needs an MI355X.

    python examples/tiled_restart.py [frames] [--frames DIR] [--snapshot FILE]

--frames DIR: job.visualize() after every frame, before and after the restart — DIR/0001.bgeo, 0002.bgeo, ... (the frame counter
travels in the snapshot file).
"""
import argparse
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import taichi_mpm_amd as tm  # noqa: E402
from taichi_mpm_amd import tiled  # noqa: E402

if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('count', nargs='?', type=int, default=4, help='frames to run before the snapshot, and again after the restart')
    ap.add_argument('--frames', metavar='DIR', help='write DIR/0001.bgeo, 0002.bgeo, ... after every frame')
    ap.add_argument('--snapshot', metavar='FILE', help='where the snapshot goes (default: a temporary file)')
    args = ap.parse_args()
    r, margin = 64, 2
    dx = 1.0 / r
    sim_cfg = dict(res=(r, r, r), delta_x=dx, base_delta_t=1e-4, gravity=(0, -10, 0))
    LS = tm.mpm.LevelSet
    ball = dict(type='sand', ppc=8, region=LS().add_sphere((0.5, 0.42, 0.5), 12 * dx), friction_angle=30, initial_velocity=(8.0, 0.0, 0.0))
    jet = dict(type='water', ppc=8, region=LS().add_sphere((0.5, 0.75, 0.5), 7 * dx), pd_source=True, delta_t=1e-3,
               initial_velocity=(-1.5, -2.0, 0.5))
    floor = LS(friction=0.4).add_plane((0, 1, 0), d=-0.2)
    path = args.snapshot or os.path.join(tempfile.mkdtemp(), "job.snap")

    # ---- the job of 8 ranks, as in tiled_rebalance.py
    probe = tm.create_simulation3('mpm').initialize(dict(sim_cfg))
    hists, cell_lo, cell_hi, total = tiled.seed_histograms(probe, ball)
    part = tiled.Partition.from_histograms((r, r, r), 8, hists, cell_lo, cell_hi, margin)
    sims = tiled.build_seeded_rank_sims(tm, [ball], part, levelset=floor, **sim_cfg)
    job = tiled.NativeVirtualJob([tiled.HipEngine(s, 0) for s in sims], part)
    job.frame_directory = args.frames
    for frame in range(args.count):
        job.add_particles(jet)
        job.run(10)
        job.rebalance()
        print("frame %d on 8 ranks: per rank %s" % (frame, [e.num_particles() for e in job.engines]))
        if args.frames:
            print("         wrote %s" % job.visualize())
    job.save_snapshot(path)
    tot = job.totals()
    print("saved %s: %d bytes, %d particles after %d substeps" % (path, os.path.getsize(path), tot["particles"], job.substeps))
    del job
    for s in sims:
        s.close()

    # ---- the restart on 3 ranks: bricks from the file, rank simulations without particles, the job, the load
    hists, cell_lo, cell_hi, total = tiled.snapshot_histograms(probe, path)
    probe.close()
    part = tiled.Partition.from_histograms((r, r, r), 3, hists, cell_lo, cell_hi, margin)
    print("%d particles in the file; 3 ranks, cuts %s" % (total, part.cuts))
    sims = []
    for rank in range(3):
        sim = tm.create_simulation3('mpm').initialize(dict(sim_cfg, max_particles=total // 2 + 4096))
        sim.set_levelset(floor)
        sim._ensure_ctx()
        sims.append(sim)
    job = tiled.NativeVirtualJob([tiled.HipEngine(s, 0) for s in sims], part)
    job.frame_directory = args.frames
    out = job.load_snapshot(path)
    print("loaded: per rank %s of %d%s; the next frame is %d" % (out["kept"], out["total"], ", ranks %s grew" % out["grew"] if out["grew"] else "",
                                                                 job.frame_count + 1))
    for frame in range(args.count):
        job.run(10)
        print("frame %d on 3 ranks: per rank %s" % (args.count + frame, [e.num_particles() for e in job.engines]))
        if args.frames:
            print("         wrote %s" % job.visualize())
    tot = job.totals()
    print("job: %d particles, error word %d" % (tot["particles"], tot["error"]))
    del job
    for s in sims:
        s.close()
