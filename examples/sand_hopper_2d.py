"""A 2D hopper: the boundary is a polygon — an arch whose two wedges leave a funnel with an open outlet — baked into a sampled level
set and installed with set_levelset(from_polygon(...).as_boundary(friction=...)) (include/mpmhip.h: mpmhip2d_set_levelset_sdf).
Sand is fed by a pd_source emitter before every frame and poured into the funnel; particle_collision keeps it out of the walls; what
passes the outlet falls to the floor of the domain, where the domain rule removes it.  The simulation is created without max_particles:
the ctx grows as the emitter feeds it.  One .bgeo frame per frame_dt; the particle count is printed per frame.  Needs an MI355X.

    python examples/sand_hopper_2d.py [out_dir] [frames]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import taichi_mpm_amd as tc_amd  # noqa: E402

# the solid, counter-clockwise: left foot, left wedge up its slope, under the lid to the right wedge, down its slope, right foot, and
# back over the top.  The outlet between the feet is 0.08 wide.
HOPPER = [(0.14, 0.30), (0.46, 0.30), (0.46, 0.36), (0.20, 0.70), (0.20, 0.84), (0.80, 0.84), (0.80, 0.70), (0.54, 0.36), (0.54, 0.30),
          (0.86, 0.30), (0.86, 0.88), (0.14, 0.88)]

if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else "/tmp/sand_hopper_2d_frames"
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    r, frame_dt = 128, 0.01
    dx = 1.0 / r
    sim = tc_amd.create_simulation2("mpm").initialize(dict(res=(r, r), base_delta_t=1e-4, gravity=(0, -10), particle_collision=True,
                                                           frame_directory=out))
    # the polygon's signed distance on the grid's own nodes; spacing=None would do the same (it resolves to delta_x)
    walls = tc_amd.SampledLevelSet2D.from_polygon(HOPPER, (r + 1, r + 1), (0.0, 0.0), dx)
    sim.set_levelset(walls.as_boundary(friction=0.4))
    nozzle = tc_amd.LevelSet().add_cuboid((0.40, 0.76, 0.0), (0.60, 0.80, 0.0))
    for frame in range(frames):  # before every frame: what leaves the nozzle through its lower edge within frame_dt
        before = sim.get_num_particles()
        sim.add_particles(dict(type='sand', region=nozzle, ppc=4, pd_source=True, initial_velocity=(0, -1.5), delta_t=frame_dt))
        fed = sim.get_num_particles() - before
        sim.step(frame_dt)
        path = sim.visualize()
        x = sim.get_particles()["x"]
        phi = sim.sample_levelset(x)[0]
        print("frame %3d: %6d particles (+%d fed), %d below the outlet, lowest phi %.3f cells -> %s"
              % (frame + 1, len(x), fed, int((x[:, 1] < 0.30).sum()), float(phi.min()) if len(x) else 0.0, path))
