"""A hollow shell of sand dropped into a bowl with a drain: both the particles and the boundary are region expressions
(taichi_mpm_amd.Region; include/mpmhip.h, "Region expressions"), evaluated on the device.

  sand      (sphere - sphere) & half space: a hollow ball clipped by a plane, seeded by add_particles(region=...) — no particle is
            made on the host
  boundary  the mesh bowl of examples/sand_bowl.py minus a vertical cylinder through its bottom.  The cylinder is a small sampled
            field; outside its lattice the leaf has no level set (phi = +inf), so its complement holds everywhere else and the bowl
            is cut only where the cylinder is.  Region.to_sampled bakes the difference on the simulation's own nodes and the result
            is installed like any sampled level set.

One .bgeo frame per frame_dt, as examples/sand_bowl.py writes them.  Needs an MI355X.

    python examples/sand_shell.py [out_dir] [frames]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import taichi_mpm_amd as tc_amd  # noqa: E402
from sand_bowl import CENTRE, R_OUT, bowl  # noqa: E402

DRAIN_R = 0.035


def drain(dx):
    """a vertical cylinder of radius DRAIN_R through the bottom of the bowl, sampled on a lattice that just holds it"""
    lo = np.array([CENTRE[0] - DRAIN_R - 4 * dx, CENTRE[1] - R_OUT - 6 * dx, CENTRE[2] - DRAIN_R - 4 * dx])
    hi = np.array([CENTRE[0] + DRAIN_R + 4 * dx, CENTRE[1] - R_OUT + 0.12, CENTRE[2] + DRAIN_R + 4 * dx])
    res = tuple(int(n) for n in np.ceil((hi - lo) / (dx / 2)) + 1)

    def cylinder(x):  # capped: the distance to the side, or to the caps where they are nearer
        rho = np.hypot(x[:, 0] - CENTRE[0], x[:, 2] - CENTRE[2]) - DRAIN_R
        cap = np.maximum(lo[1] + 2 * dx - x[:, 1], x[:, 1] - (hi[1] - 2 * dx))
        return np.minimum(np.maximum(rho, cap), 0.0) + np.hypot(np.maximum(rho, 0.0), np.maximum(cap, 0.0))
    return tc_amd.SampledLevelSet.from_function(cylinder, res, tuple(lo), dx / 2)


if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else "/tmp/sand_shell_frames"
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    r = 128
    dx = 1.0 / r
    Region, LevelSet = tc_amd.Region, tc_amd.LevelSet
    mpm = tc_amd.MPM(res=(r, r, r), base_delta_t=1e-4, frame_dt=0.01, num_frames=frames, gravity=(0, -10, 0),
                     frame_directory=out, verbose_bgeo=False, particle_collision=True)
    solid = Region(tc_amd.MeshLevelSet(bowl(), (r + 1,) * 3, (0, 0, 0), dx, band=3 * dx + 2 * dx)) - Region(drain(dx))
    # samples on the simulation's own nodes (the grid pass reads phi with one load per node); band: the default, what it reads
    boundary = solid.to_sampled((r + 1,) * 3, (0, 0, 0), dx)
    mpm.set_levelset(boundary.set_friction(0.4), False)
    c = (CENTRE[0], CENTRE[1] + 0.12, CENTRE[2])
    shell = (Region(LevelSet().add_sphere(c, 0.11)) - Region(LevelSet().add_sphere(c, 0.07))) & Region(LevelSet().add_plane((0, 1, 0), point=(0, c[1] + 0.04, 0)))
    mpm.add_particles(type='sand', region=shell, ppc=8, friction_angle=30)
    n = mpm.c.get_num_particles()
    mpm.simulate()
    print(n, "particles; frames written to", out, ":", sorted(os.listdir(out))[:3], "...")
