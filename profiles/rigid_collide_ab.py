"""What the rigid-rigid collision pass costs per substep (profiles/rigid_collide_ab.txt).

Scene: examples/sand_paddle.py's size — a 128^3 grid, a 48^3-cell block of sand (885 k particles), a scripted paddle wheel — plus two
free boxes stacked above the wheel (in contact from the first substep, so the resolution runs as well as the detection).

  parent   the library of the parent commit (taichi_mpm_amd/lib/libmpmhip_parent.so, loaded through MPMHIP_LIB_VARIANT=parent):
           the pass does not exist
  off      this library, the key absent
  on       this library, rigid_body_collision=True

    python profiles/rigid_collide_ab.py [rounds]

Every measurement is a process of its own (the variant is chosen when the package is imported); the three alternate, `rounds` times
(default 5); a measurement is the host clock around STEPS substeps between two synchronisations, after WARMUP substeps; the table
gives the median and the spread of each."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS = 50, 200


def measure(mode):
    sys.path.insert(0, ROOT)
    import warnings

    import numpy as np

    import taichi_mpm_amd as tm
    from examples.box_stack import box
    from examples.sand_paddle import paddle
    r = 128
    cfg = dict(res=(r,) * 3, delta_x=1.0 / r, base_delta_t=1e-4, gravity=(0, -10, 0), penalty=1e4, max_particles=1 << 20)
    if mode == "on":
        cfg["rigid_body_collision"] = True
    sim = tm.create_simulation3("mpm").initialize(cfg)
    sim.set_levelset(tm.mpm.LevelSet(friction=-1).add_plane((0, 1, 0), d=-0.2))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sim.add_particles(dict(type="rigid", mesh=paddle(), codimensional=True, friction=-2, density=500,
                               scripted_position=lambda t: (0.5, 0.34, 0.5), scripted_rotation=lambda t: (0.0, 360.0 * t, 0.0)))
        sim.add_particles(dict(type="rigid", mesh=box(0.06, 0.03, 0.06), codimensional=False, density=400, friction=0.5,
                               initial_position=(0.5, 0.74, 0.5)))
        sim.add_particles(dict(type="rigid", mesh=box(0.04, 0.03, 0.04), codimensional=False, density=400, friction=0.5,
                               initial_position=(0.51, 0.799, 0.5), initial_rotation=(0.0, 20.0, 0.0)))
    g = (np.arange(40, 88)[:, None] + np.array([0.25, 0.75])[None, :]).reshape(-1) / r
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    sim.add_particles(dict(type="sand", positions=x))
    sim.run_substeps(WARMUP)
    sim.synchronize()
    t0 = time.perf_counter()
    sim.run_substeps(STEPS)
    sim.synchronize()
    ms = (time.perf_counter() - t0) / STEPS * 1e3
    hits = len(sim.get_rigid_collisions()) if mode != "parent" else 0
    n = sim.get_num_particles()
    sim.close()
    print(json.dumps(dict(mode=mode, ms_per_substep=ms, particles=int(n), collisions_last_substep=hits)))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--measure":
        return measure(sys.argv[2])
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    modes = ["parent", "off", "on"]
    if not os.path.exists(os.path.join(ROOT, "taichi_mpm_amd", "lib", "libmpmhip_parent.so")):
        print("# no libmpmhip_parent.so (build the parent commit's csrc/mpmhip.hip into it): the parent column is left out")
        modes = modes[1:]
    got = {m: [] for m in modes}
    for k in range(rounds):
        for m in modes:
            env = dict(os.environ)
            env.pop("MPMHIP_LIB_VARIANT", None)
            if m == "parent":
                env["MPMHIP_LIB_VARIANT"] = "parent"
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", m], env=env, capture_output=True, text=True, timeout=280)
            if out.returncode != 0:  # nothing more is started on the device after a failure
                print(out.stdout[-2000:], out.stderr[-2000:])
                sys.exit("measurement %r failed with status %d: stopping" % (m, out.returncode))
            row = json.loads(out.stdout.strip().splitlines()[-1])
            got[m].append(row)
            print("# round %d %-6s %.4f ms / substep, %d particles, %d collisions" % (k, m, row["ms_per_substep"], row["particles"], row["collisions_last_substep"]), flush=True)
    print("%-8s %12s %12s %12s   (ms per substep over %d substeps, %d rounds, alternating)" % ("mode", "median", "min", "max", STEPS, rounds))
    for m in modes:
        v = [r["ms_per_substep"] for r in got[m]]
        print("%-8s %12.4f %12.4f %12.4f" % (m, statistics.median(v), min(v), max(v)))


if __name__ == "__main__":
    main()
