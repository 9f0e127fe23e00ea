"""ms per substep of the 2D solver with a sampled level set as its boundary: the parent commit's library with the analytic floor, this
tree with the analytic floor, this tree with the same floor baked at spacing dx — alternating on one GPU.
    python profiles/sdf2d_ab.py [--rounds 5] [--steps 200]                      the table
    python profiles/sdf2d_ab.py --one SCENE --variant parent|shapes|sampled [--det]   one measurement (what the table spawns, and what
                                                                                 a rocprofv3 --kernel-trace --stats run wraps)
`parent` is the parent commit's library under this tree's Python package: build it at the parent commit and copy it to
taichi_mpm_amd/lib/libmpmhip_parent.so; the measurement selects it with MPMHIP_LIB_VARIANT=parent (it only ever gets the analytic
floor, so none of the new entry points is called on it).  Every measurement is a process of its own: scene set-up, 50 substeps of
warm-up, then --steps substeps between two synchronisations, wall clock / steps.  Scenes (those of profiles/det2d_ab.py): sand256
(256^2 grid, 40 000 sand particles on a friction floor), sand1024 (1024^2, 1 M sand particles on a floor); each in the default and in
the deterministic mode (--det).  particle_collision is on in every variant, so the sampled variant pays for both readers of the set:
the grid pass (k_grid_sdf instead of k_grid) and the push behind G2P (k2_sdf_collide, a pass of its own)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ("sand256", "sand1024")
VARIANTS = ("parent", "shapes", "sampled")


def one(scene, variant, det, steps):
    sys.path.insert(0, REPO)
    import taichi_mpm_amd as tm
    tm.load()
    from tests.golden.make_golden import mpm2d_state
    res, lo, cells = (256, (78, 40), 100) if scene == "sand256" else (1024, (262, 80), 500)
    dx, dt = 1.0 / res, min(1e-4, 0.0256 / res)
    x, v, F, B = mpm2d_state(res, lo=lo, cells=cells, seed=9)
    vol = dx * dx / 4
    gp, _ = tm.group_params("sand", 400.0 * vol, vol)
    sim = tm.create_simulation2("mpm").initialize(dict(res=(res, res), delta_x=dx, base_delta_t=dt, max_particles=len(x) + 64,
                                                       particle_collision=True, deterministic=bool(det)))
    floor = tm.mpm.LevelSet(friction=0.5, delta_x=dx).add_plane((0, 1, 0), d=-0.12 if res == 256 else -0.06)
    if variant == "sampled":
        floor = tm.SampledLevelSet2D.from_levelset(floor, (res + 1, res + 1), (0.0, 0.0), dx).as_boundary(0.5)
    sim.set_levelset(floor)
    sim.add_particles(dict(type="sand", positions=x, velocities=v, F=F, B=B, params=gp))
    sim.run_substeps(50)
    sim.synchronize()
    t0 = time.perf_counter()
    sim.run_substeps(steps)
    sim.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    n = sim.get_num_particles()
    sim.close()
    print("RESULT %s %s %s %.5f %d" % (scene, "det" if det else "default", variant, ms, n))


def table(rounds, steps):
    got = {(s, d, v): [] for s in SCENES for d in (0, 1) for v in VARIANTS}
    for r in range(rounds):
        for s in SCENES:
            for d in (0, 1):
                for v in VARIANTS:
                    env = dict(os.environ)
                    env.pop("MPMHIP_LIB_VARIANT", None)
                    if v == "parent":
                        env["MPMHIP_LIB_VARIANT"] = "parent"
                    cmd = [sys.executable, os.path.abspath(__file__), "--one", s, "--variant", v, "--steps", str(steps)] + (["--det"] if d else [])
                    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
                    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
                    if out.returncode != 0 or not line:
                        print(out.stdout[-2000:], out.stderr[-2000:])
                        raise SystemExit("measurement failed: %s %s %s" % (s, d, v))  # (nothing more is started on the GPU)
                    got[(s, d, v)].append(float(line[0].split()[4]))
        print("round %d done" % (r + 1), flush=True)
    print("ms per substep, %d rounds alternating parent / shapes / sampled, %d substeps each after 50 of warm-up" % (rounds, steps))
    for s in SCENES:
        for d in (0, 1):
            mode = "det" if d else "default"
            for v in VARIANTS:
                t = got[(s, d, v)]
                print("  %-9s %-8s %-8s %s   median %.4f  spread %.4f-%.4f" % (s, mode, v, " ".join("%.4f" % q for q in t), statistics.median(t), min(t), max(t)))
            p, a, b = (statistics.median(got[(s, d, v)]) for v in VARIANTS)
            lo, hi = min(got[(s, d, "parent")]), max(got[(s, d, "parent")])
            where = "inside" if lo <= a <= hi else ("BELOW" if a < lo else "ABOVE")
            print("  %-9s %-8s shapes against parent: %.4f vs %.4f (parent's own spread %.4f-%.4f): %s;  sampled - shapes: %+.4f ms (%+.1f %%)"
                  % (s, mode, a, p, lo, hi, where, b - a, 100.0 * (b - a) / a))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--one", choices=SCENES)
    ap.add_argument("--variant", choices=VARIANTS, default="shapes")
    ap.add_argument("--det", action="store_true")
    a = ap.parse_args()
    if a.one:
        one(a.one, a.variant, a.det, a.steps)
    else:
        table(a.rounds, a.steps)
