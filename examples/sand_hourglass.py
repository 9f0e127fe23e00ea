"""Sand running through an hourglass: a boundary no union of planes, spheres and cuboids expresses, given as a closed-form
signed-distance function and sampled onto a lattice with SampledLevelSet.from_function (include/mpmhip.h:
mpmhip_set_levelset_sdf).  One .bgeo frame per frame_dt, as examples/sand_column.py writes them.  Needs an MI355X.

    python examples/sand_hourglass.py [out_dir] [frames]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import taichi_mpm_amd as tc_amd  # noqa: E402

CENTRE, HALF_HEIGHT, R_BULB, R_NECK = (0.5, 0.5, 0.5), 0.3, 0.22, 0.04


def hourglass(x):
    """phi of the glass: two cones around the vertical axis through CENTRE that meet in a neck of radius R_NECK, closed by a floor
    and a lid.  Negative inside the glass wall (everything outside the two bulbs).  The distance to a cone is exact; the minimum of
    the three is the distance except close to the edges where they meet."""
    d = x - np.asarray(CENTRE)
    rho, y = np.hypot(d[:, 0], d[:, 2]), d[:, 1]
    slope = (R_BULB - R_NECK) / HALF_HEIGHT
    wall = (R_NECK + slope * np.abs(y) - rho) / np.sqrt(1.0 + slope * slope)
    return np.minimum(wall, np.minimum(y + HALF_HEIGHT, HALF_HEIGHT - y))


if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else "/tmp/sand_hourglass_frames"
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    r = 128
    dx = 1.0 / r
    mpm = tc_amd.MPM(res=(r, r, r), base_delta_t=1e-4, frame_dt=0.01, num_frames=frames, gravity=(0, -10, 0),
                     frame_directory=out, verbose_bgeo=False, particle_collision=True)
    # samples on the simulation's own nodes: the grid pass reads phi with one load per node
    glass = tc_amd.SampledLevelSet.from_function(hourglass, (r + 1,) * 3, (0, 0, 0), dx, friction=0.4)
    mpm.set_levelset(glass, False)
    # the upper bulb, filled to two cells from the wall
    g = (np.arange(2 * r) + 0.5) * (dx / 2)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    x = x[(x[:, 1] > CENTRE[1] + 0.05) & (x[:, 1] < CENTRE[1] + 0.22)]
    x = x[hourglass(x) > 2 * dx]
    mpm.add_particles(type='sand', positions=x.astype(np.float32), friction_angle=30)
    mpm.simulate()
    print(len(x), "particles; frames written to", out, ":", sorted(os.listdir(out))[:3], "...")
