"""ms per substep with a sampled level set as the boundary, the parent commit's library and this tree's alternating on one GPU.
    python profiles/sdf2d_ab.py [--rounds 5] [--steps 200] [--scenes A,B] [--modes default,det]   the table (or some of its rows)
    python profiles/sdf2d_ab.py --one SCENE --variant VARIANT [--det]           one measurement (what the table spawns, and what
                                                                                 a rocprofv3 --kernel-trace --stats run wraps)
Variants: parent / shapes = the analytic floor on the parent's library / on this tree's; parent_sampled / sampled = the same floor
baked into a lattice, on the parent's library / on this tree's.  The parent's library runs under this tree's Python package: build it
at the parent commit and copy it to taichi_mpm_amd/lib/libmpmhip_parent.so; the measurement selects it with MPMHIP_LIB_VARIANT=parent
(parent_sampled needs a parent that has the sampled entry points).  Every measurement is a process of its own: scene set-up, 50
substeps of warm-up, then --steps substeps between two synchronisations, wall clock / steps.  Each scene in the default and in the
deterministic mode (--det); particle_collision is on in every variant, so a sampled variant pays for both readers of the set: the
grid pass and the push behind G2P (a pass of its own).
  2D (those of profiles/det2d_ab.py): sand256 (256^2 grid, 40 000 sand particles on a friction floor), sand1024 (1024^2, 1 M sand
      particles on a floor); the lattice has the grid's nodes (k_grid_sdf instead of k_grid, k2_sdf_collide).
  3D, the sampled variants only: 128^3 grid, a block of 48^3 cells x 8 = 885 k sand particles on a floor.  sand3d_aligned: the
      lattice has the grid's nodes, so the grid pass takes one load per node (sdf_node_in_band); sand3d_interp: spacing 1.25 dx, so
      it interpolates (sdf_node_bc's other branch).  k_sdf_collide interpolates in both."""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ("sand256", "sand1024", "sand3d_aligned", "sand3d_interp")
VARIANTS = ("parent", "shapes", "parent_sampled", "sampled")
RES3, CELLS3, FLOOR3 = 128, 48, 0.1


def variants_of(scene):
    return VARIANTS[2:] if scene.startswith("sand3d") else VARIANTS


def one3d(tm, scene, det):
    dx = 1.0 / RES3
    sim = tm.create_simulation3("mpm").initialize(dict(res=(RES3,) * 3, delta_x=dx, base_delta_t=1e-4, gravity=(0, -10, 0),
                                                       particle_collision=True, deterministic=bool(det)))
    floor = tm.mpm.LevelSet(friction=0.5, delta_x=dx).add_plane((0, 1, 0), d=-FLOOR3)
    h = dx if scene == "sand3d_aligned" else 1.25 * dx
    sim.set_levelset(tm.mpm.SampledLevelSet.from_levelset(floor, (int(1.0 / h) + 2,) * 3, (0.0, 0.0, 0.0), h))
    lo = RES3 // 2 - CELLS3 // 2
    sim.add_particles(dict(type="sand", cube_lo=(lo, int(FLOOR3 * RES3) + 1, lo), cube_cells=CELLS3))  # the block stands on the floor
    return sim


def one2d(tm, scene, variant, det):
    from tests.golden.make_golden import mpm2d_state
    res, lo, cells = (256, (78, 40), 100) if scene == "sand256" else (1024, (262, 80), 500)
    dx, dt = 1.0 / res, min(1e-4, 0.0256 / res)
    x, v, F, B = mpm2d_state(res, lo=lo, cells=cells, seed=9)
    vol = dx * dx / 4
    gp, _ = tm.group_params("sand", 400.0 * vol, vol)
    sim = tm.create_simulation2("mpm").initialize(dict(res=(res, res), delta_x=dx, base_delta_t=dt, max_particles=len(x) + 64,
                                                       particle_collision=True, deterministic=bool(det)))
    floor = tm.mpm.LevelSet(friction=0.5, delta_x=dx).add_plane((0, 1, 0), d=-0.12 if res == 256 else -0.06)
    if variant.endswith("sampled"):
        floor = tm.SampledLevelSet2D.from_levelset(floor, (res + 1, res + 1), (0.0, 0.0), dx).as_boundary(0.5)
    sim.set_levelset(floor)
    sim.add_particles(dict(type="sand", positions=x, velocities=v, F=F, B=B, params=gp))
    return sim


def one(scene, variant, det, steps):
    sys.path.insert(0, REPO)
    import taichi_mpm_amd as tm
    tm.load()
    sim = one3d(tm, scene, det) if scene.startswith("sand3d") else one2d(tm, scene, variant, det)
    sim.run_substeps(50)
    sim.synchronize()
    t0 = time.perf_counter()
    sim.run_substeps(steps)
    sim.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    n = sim.get_num_particles()
    sim.close()
    print("RESULT %s %s %s %.5f %d" % (scene, "det" if det else "default", variant, ms, n))


def against(got, key, a, b):
    """the row of the convention: b's median against a's own min-max"""
    ta, tb = got[key + (a,)], got[key + (b,)]
    lo, hi, m = min(ta), max(ta), statistics.median(tb)
    where = "inside" if lo <= m <= hi else ("BELOW" if m < lo else "ABOVE")
    return "%s against %s: %.4f vs %.4f (%s's own spread %.4f-%.4f): %s" % (b, a, m, statistics.median(ta), a, lo, hi, where)


def table(rounds, steps, scenes, modes):
    got = {(s, d, v): [] for s in scenes for d in modes for v in variants_of(s)}
    for r in range(rounds):
        for s, d, v in got:
            env = dict(os.environ)
            env.pop("MPMHIP_LIB_VARIANT", None)
            if v.startswith("parent"):
                env["MPMHIP_LIB_VARIANT"] = "parent"
            cmd = [sys.executable, os.path.abspath(__file__), "--one", s, "--variant", v, "--steps", str(steps)] + (["--det"] if d else [])
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
            if out.returncode != 0 or not line:
                print(out.stdout[-2000:], out.stderr[-2000:])
                raise SystemExit("measurement failed: %s %s %s" % (s, d, v))  # (nothing more is started on the GPU)
            got[(s, d, v)].append(float(line[0].split()[4]))
        print("round %d done" % (r + 1), flush=True)
    print("ms per substep, %d rounds alternating the variants, %d substeps each after 50 of warm-up" % (rounds, steps))
    for s in scenes:
        for d in modes:
            mode = "det" if d else "default"
            for v in variants_of(s):
                t = got[(s, d, v)]
                print("  %-14s %-8s %-14s %s   median %.4f  spread %.4f-%.4f" % (s, mode, v, " ".join("%.4f" % q for q in t), statistics.median(t), min(t), max(t)))
            if "shapes" in variants_of(s):
                a, b = (statistics.median(got[(s, d, v)]) for v in ("shapes", "sampled"))
                print("  %-14s %-8s %s;  sampled - shapes: %+.4f ms (%+.1f %%)" % (s, mode, against(got, (s, d), "parent", "shapes"), b - a, 100.0 * (b - a) / a))
            print("  %-14s %-8s %s" % (s, mode, against(got, (s, d), "parent_sampled", "sampled")))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--scenes", default=",".join(SCENES), help="the table's scenes, comma-separated")
    ap.add_argument("--modes", default="default,det", help="the table's modes, comma-separated")
    ap.add_argument("--one", choices=SCENES)
    ap.add_argument("--variant", choices=VARIANTS, default="shapes")
    ap.add_argument("--det", action="store_true")
    a = ap.parse_args()
    if a.one:
        one(a.one, a.variant, a.det, a.steps)
    else:
        table(a.rounds, a.steps, a.scenes.split(","), [m == "det" for m in a.modes.split(",")])
