"""Rigid-rigid collisions (rigid_body_collision=True, MPM::rigidify of the reference): two free boxes stacked on a scripted
platform that sinks into a bed of sand.  The boxes rest on each other and on the platform through the collision pass (convex hulls,
libccd's MPR reproduced on the device); the sand couples to the bodies through CPIC.  Without the key the boxes would fall through the
platform and through each other.  Needs an MI355X.

    python examples/box_stack.py [out_dir] [frames]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import taichi_mpm_amd as tc_amd  # noqa: E402


def box(hx, hy, hz):
    """a closed box, outward-facing triangles"""
    c = np.array([[x, y, z] for x in (-hx, hx) for y in (-hy, hy) for z in (-hz, hz)], np.float32)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return np.array([[c[a], c[b], c[d]] for a, b, d, e in q] + [[c[a], c[d], c[e]] for a, b, d, e in q], np.float32)


if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else "/tmp/box_stack_frames"
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    r = 64
    mpm = tc_amd.MPM(res=(r, r, r), base_delta_t=1e-4, frame_dt=0.01, num_frames=frames, gravity=(0, -10, 0), frame_directory=out,
                     penalty=1e4, max_particles=1 << 19,
                     rigid_body_collision=True)  # rigid_body_iterations=5, rigid_penalty=1e3, rigid_body_position_iterations=True
    levelset = mpm.create_levelset()
    levelset.add_plane((0, 1, 0), d=-0.2)
    levelset.set_friction(-1)
    mpm.set_levelset(levelset, False)
    # the platform sinks slowly into the bed, carrying the stack
    platform = mpm.add_particles(type='rigid', mesh=box(0.2, 0.02, 0.2), codimensional=False, friction=0.5,
                                 scripted_position=lambda t: (0.5, 0.46 - 0.3 * t, 0.5), scripted_rotation=lambda t: (0.0, 0.0, 0.0))
    lower = mpm.add_particles(type='rigid', mesh=box(0.08, 0.04, 0.08), codimensional=False, density=400, friction=0.5,
                              initial_position=(0.5, 0.521, 0.5))
    upper = mpm.add_particles(type='rigid', mesh=box(0.05, 0.04, 0.05), codimensional=False, density=400, friction=0.5,
                              initial_position=(0.51, 0.602, 0.5), initial_rotation=(0.0, 20.0, 0.0))
    g = (np.arange(18, 46)[:, None] + np.array([0.25, 0.75])[None, :]).reshape(-1) / r   # a bed of sand below the platform:
    gy = (np.arange(13, 26)[:, None] + np.array([0.25, 0.75])[None, :]).reshape(-1) / r  # 28 x 13 x 28 cells, 8 particles per cell
    mpm.add_particles(type='sand', positions=np.stack(np.meshgrid(g, gy, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32),
                      friction_angle=30)
    mpm.simulate()
    for name, rid in (("lower", lower), ("upper", upper)):
        print(name, "box at", mpm.c.get_rigid_state(int(rid))["position"])
    print("collisions of the last substep:", [(c["i"], c["j"], float(c["depth"])) for c in mpm.c.get_rigid_collisions()])
    print("frames written to", out)
