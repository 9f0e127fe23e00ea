"""The scene of examples/sand_paddle.py as a tiled job: a scripted paddle wheel stirs a block of sand on a floor, on 8 ranks of one
partition — here as 8 ctxs on one GPU (tiled.NativeVirtualJob; the ranks of a multi-GPU job make the same calls, one per process).
Every rank holds the WHOLE paddle: the bodies are added on every rank, in the same order, before the job is set up.  A rank's
colour-aware transfer kernels collect the impulses of the rank's own particles; twice a substep the ranks' impulse rows (288 bytes)
reach every rank, which adds them in rank order, so the body's record is the same bits on all ranks (job.rigid_digests()).
The sand is seeded on the device, every rank filling its own brick.  Prints per-rank particle counts and the body's state per frame.
Needs an MI355X.

    python examples/tiled_paddle.py [frames]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import taichi_mpm_amd as tm  # noqa: E402
from taichi_mpm_amd import tiled  # noqa: E402


def paddle(r=0.16, h=0.10):
    """two crossed rectangular blades around the y axis"""
    a = np.array([[[-r, -h, 0], [r, -h, 0], [r, h, 0]], [[-r, -h, 0], [r, h, 0], [-r, h, 0]]], np.float32)
    return np.concatenate([a, a[:, :, [2, 1, 0]]])


if __name__ == '__main__':
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    r, world, margin = 64, 8, 2
    dx = 1.0 / r
    sim_cfg = dict(res=(r, r, r), delta_x=dx, base_delta_t=1e-4, gravity=(0, -10, 0), penalty=1e4)
    LS = tm.mpm.LevelSet
    sand = dict(type='sand', ppc=8, region=LS().add_cuboid((20 * dx,) * 3, (44 * dx,) * 3), friction_angle=30)
    wheel = dict(type='rigid', mesh=paddle(), codimensional=True, friction=-2, density=500,
                 scripted_position=lambda t: (0.5, 0.34, 0.5), scripted_rotation=lambda t: (0.0, 360.0 * t, 0.0))  # one turn per second

    probe = tm.create_simulation3('mpm').initialize(dict(sim_cfg))
    hists, cell_lo, cell_hi, total = tiled.seed_histograms(probe, sand)
    probe.close()
    part = tiled.Partition.from_histograms((r, r, r), world, hists, cell_lo, cell_hi, margin)
    print("%d particles to come; cuts %s" % (total, part.cuts))

    floor = LS(friction=-1).add_plane((0, 1, 0), d=-0.2)
    sims = tiled.build_seeded_rank_sims(tm, [sand], part, levelset=floor, bodies=[wheel], **sim_cfg)
    job = tiled.NativeVirtualJob([tiled.HipEngine(s, 0) for s in sims], part)  # (checks that every rank holds the same bodies)
    for frame in range(frames):
        job.run(100)  # frame_dt = 0.01
        st = job.get_rigid_state(1)
        print("frame %d: particles per rank %s; paddle rotation %s angular velocity %s; replicas one: %s" % (
            frame, [e.num_particles() for e in job.engines], np.round(st["rotation"], 4), np.round(st["angular_velocity"], 3),
            len(set(job.rigid_digests())) == 1))
    tot = job.totals()
    print("job: %d particles, %d migrated, error word %d" % (tot["particles"], tot["migrated"], tot["error"]))
    del job
    for s in sims:
        s.close()
