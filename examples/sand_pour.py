"""A jet of sand poured into the bowl of examples/sand_bowl.py.  The emitter is add_particles(region=..., pd_source=True) called
before every frame, as the reference's water.py and sand_stir.py do: the nozzle — a small box above the bowl — is a level set, and
each call seeds, on the device, the shell of it that the jet vacates within one frame, from the periodic Poisson-disk tile that
drifts with the jet (include/mpmhip.h: mpmhip_seed_particles).  No particle position is computed on the host.  One .bgeo frame per
frame_dt.  Needs an MI355X.

    python examples/sand_pour.py [out_dir] [frames]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import taichi_mpm_amd as tc_amd  # noqa: E402
from sand_bowl import bowl  # noqa: E402

if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else "/tmp/sand_pour_frames"
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    r = 128
    dx = 1.0 / r
    mpm = tc_amd.MPM(res=(r, r, r), base_delta_t=1e-4, frame_dt=0.01, num_frames=frames, gravity=(0, -10, 0),
                     frame_directory=out, verbose_bgeo=False, particle_collision=True)
    mpm.set_levelset(tc_amd.MeshLevelSet(bowl(), (r + 1,) * 3, (0, 0, 0), dx, band=3 * dx + 2 * dx, friction=0.4), False)
    nozzle = tc_amd.mpm.LevelSet().add_cuboid((0.46, 0.80, 0.46), (0.54, 0.86, 0.54))
    counts = []

    def pour(t, dt):  # before every frame: what leaves the nozzle through its lower face within dt
        before = mpm.c.get_num_particles()
        mpm.add_particles(type='sand', region=nozzle, ppc=8, pd_source=True, initial_velocity=(0, -2, 0), delta_t=dt, friction_angle=30)
        counts.append(mpm.c.get_num_particles() - before)

    mpm.simulate(frame_update=pour)
    print(mpm.c.get_num_particles(), "particles after", frames, "frames (", counts[:3], "... per frame ); frames written to", out, ":",
          sorted(os.listdir(out))[:3], "...")
