"""The 2D solver seeded on the device: a star of jelly — a polygon baked into a SampledLevelSet2D — resting on a floor, under a jet of
water.  The emitter is add_particles(region=..., pd_source=True) called before every frame, as the reference's 2D scenes do: the nozzle
— a small box — is a level set, and each call seeds the strip of it that the jet vacates within one frame from the 2D periodic
Poisson-disk tile, which drifts with the jet (include/mpmhip.h: mpmhip2d_seed_particles).  No particle position is computed on the
host.  One .bgeo frame per frame_dt; the particle count is printed per frame.  Needs an MI355X.

    python examples/jet_2d.py [out_dir] [frames]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import taichi_mpm_amd as tc_amd  # noqa: E402


def star(centre, r_out, r_in, points=5):
    """the vertices of a star polygon, (2 * points, 2)"""
    a = np.pi / 2 + np.arange(2 * points) * np.pi / points
    r = np.where(np.arange(2 * points) % 2 == 0, r_out, r_in)
    return np.asarray(centre) + np.stack([r * np.cos(a), r * np.sin(a)], axis=-1)


if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else "/tmp/jet_2d_frames"
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    r, frame_dt = 128, 0.01
    dx = 1.0 / r
    sim = tc_amd.create_simulation2("mpm").initialize(dict(res=(r, r), base_delta_t=1e-4, gravity=(0, -10), frame_directory=out))
    sim.set_levelset(tc_amd.LevelSet(friction=0.4).add_plane((0, 1, 0), d=-0.1))  # the floor line y = 0.1
    # a lattice of spacing dx / 2 around the star (the field's outside is not in the region)
    jelly = tc_amd.SampledLevelSet2D.from_polygon(star((0.5, 0.27), 0.16, 0.07), (96, 96), (0.31, 0.08), dx / 2)
    sim.add_particles(dict(type='jelly', region=jelly, ppc=4, E=2e4))
    print("jelly star:", sim.get_num_particles(), "particles")
    nozzle = tc_amd.LevelSet().add_cuboid((0.47, 0.80, 0.0), (0.53, 0.84, 0.0))
    for frame in range(frames):  # before every frame: what leaves the nozzle through its lower edge within frame_dt
        before = sim.get_num_particles()
        sim.add_particles(dict(type='water', region=nozzle, ppc=4, pd_source=True, initial_velocity=(0, -2), delta_t=frame_dt))
        sim.step(frame_dt)
        path = sim.visualize()
        print("frame %3d: %6d particles (+%d) -> %s" % (frame + 1, sim.get_num_particles(), sim.get_num_particles() - before, path))
