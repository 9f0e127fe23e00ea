"""Sand poured into a bowl given as a triangle mesh: MeshLevelSet hands the triangles to the library, which voxelises them on the
device straight into the simulation's sampled level set (include/mpmhip.h: mpmhip_set_levelset_mesh).  The bowl is generated here
as a closed surface of revolution — an outer and an inner half sphere joined by a flat rim —; a mesh from a file goes the same way
(MeshLevelSet("bowl.obj", ...)).  One .bgeo frame per frame_dt, as examples/sand_column.py writes them.  Needs an MI355X.

    python examples/sand_bowl.py [out_dir] [frames]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import taichi_mpm_amd as tc_amd  # noqa: E402

CENTRE, R_OUT, R_IN = (0.5, 0.45, 0.5), 0.32, 0.27


def revolve(profile, segments):
    """closed triangle mesh of the profile [(rho, y), ...] turned around the vertical axis; the first and the last point lie on the
    axis (rho = 0), so the surface is closed"""
    profile = np.asarray(profile, np.float64)
    assert profile[0, 0] == 0 and profile[-1, 0] == 0 and np.all(profile[1:-1, 0] > 0)
    ang = np.arange(segments) * 2 * np.pi / segments
    ring = lambda p: np.stack([p[0] * np.cos(ang), np.full(segments, p[1]), p[0] * np.sin(ang)], 1)
    rings = [ring(p) for p in profile]
    nxt = (np.arange(segments) + 1) % segments
    tri = []
    for a, b in zip(rings[:-1], rings[1:]):
        tri.append(np.stack([a, b, b[nxt]], 1))  # (on the axis one of the two is a sliver of zero area: the voxeliser skips it)
        tri.append(np.stack([a, b[nxt], a[nxt]], 1))
    return np.concatenate(tri)


def bowl(segments=96, arcs=32):
    t = np.linspace(0.0, np.pi / 2, arcs + 1)
    outer = [(R_OUT * np.sin(a), -R_OUT * np.cos(a)) for a in t]          # bottom of the outside, up to the rim
    inner = [(R_IN * np.sin(a), -R_IN * np.cos(a)) for a in t[::-1]]       # across the rim, down the inside
    outer[0], inner[-1] = (0.0, -R_OUT), (0.0, -R_IN)
    return revolve(outer + inner, segments) + np.asarray(CENTRE)


if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else "/tmp/sand_bowl_frames"
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    r = 128
    dx = 1.0 / r
    mpm = tc_amd.MPM(res=(r, r, r), base_delta_t=1e-4, frame_dt=0.01, num_frames=frames, gravity=(0, -10, 0),
                     frame_directory=out, verbose_bgeo=False, particle_collision=True)
    # samples on the simulation's own nodes (the grid pass reads phi with one load per node); the band the grid pass needs
    mpm.set_levelset(tc_amd.MeshLevelSet(bowl(), (r + 1,) * 3, (0, 0, 0), dx, band=3 * dx + 2 * dx, friction=0.4), False)
    # a column of sand above the middle of the bowl
    g = (np.arange(2 * r) + 0.5) * (dx / 2)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    d = x - np.asarray(CENTRE)
    x = x[(np.hypot(d[:, 0], d[:, 2]) < 0.1) & (d[:, 1] > -0.15) & (d[:, 1] < 0.25)]
    mpm.add_particles(type='sand', positions=x.astype(np.float32), friction_angle=30)
    mpm.simulate()
    print(len(x), "particles; frames written to", out, ":", sorted(os.listdir(out))[:3], "...")
