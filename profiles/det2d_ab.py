"""ms per substep of the 2D solver: the parent commit's default path, this tree's default path and this tree's deterministic mode
(mpmhip2d_config.deterministic), alternating on one GPU.
    python profiles/det2d_ab.py --parent DIR [--rounds 5] [--steps 200]     the table (DIR: a built copy of the parent tree)
    python profiles/det2d_ab.py --one SCENE --variant parent|default|det [--root DIR]    one measurement (what the table spawns, and
                                                                                          what a rocprofv3 --kernel-trace run wraps)
Every measurement is a process of its own (the parent's library lacks the mode's symbols, so it needs its own package): scene set-up,
50 substeps warm-up, then --steps substeps between two synchronisations, wall clock / steps.  Scenes: sand256 (256^2 grid, 40 000
sand particles on a floor: the scene of tests/test_gpu_deterministic_2d.py), sand1024 (1024^2, 1 M sand particles on a floor),
box512 (the box_sand CPIC scene of tests/cpic_scenes.py at 512^2: a free box in 51 200 sand particles)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ("sand256", "sand1024", "box512")


def one(scene, variant, root, steps):
    sys.path.insert(0, root)
    import numpy as np
    import taichi_mpm_amd as tm
    tm.load()
    sys.path.insert(0, REPO)  # the scene helpers always come from this tree
    from tests.golden.make_golden import mpm2d_state
    cfg = dict(deterministic=True) if variant == "det" else {}
    if scene in ("sand256", "sand1024"):
        res, lo, cells = (256, (78, 40), 100) if scene == "sand256" else (1024, (262, 80), 500)
        dx, dt = 1.0 / res, min(1e-4, 0.0256 / res)
        x, v, F, B = mpm2d_state(res, lo=lo, cells=cells, seed=9)
        vol = dx * dx / 4
        gp, _ = tm.group_params("sand", 400.0 * vol, vol)
        sim = tm.create_simulation2("mpm").initialize(dict(res=(res, res), delta_x=dx, base_delta_t=dt, max_particles=len(x) + 64, **cfg))
        sim.set_levelset(tm.mpm.LevelSet(friction=0.5).add_plane((0, 1, 0), d=-0.12 if res == 256 else -0.06))
        sim.add_particles(dict(type="sand", positions=x, velocities=v, F=F, B=B, params=gp))
    else:
        import tests.cpic_scenes as cs
        from oracle import oracle as orc
        res = 512
        dx, dt = 1.0 / res, 5e-5
        rng = np.random.default_rng(0)
        g = np.arange(22 * 8, 42 * 8) + 0.25
        X = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
        X = np.concatenate([X, X + 0.5]) + rng.uniform(-0.2, 0.2, (2 * len(X), 2))
        x, v = (X * dx).astype(np.float32), rng.normal(0, 0.3, X.shape).astype(np.float32)
        vol = dx * dx / 4
        sim = tm.create_simulation2("mpm").initialize(dict(res=(res, res), delta_x=dx, base_delta_t=dt, gravity=(0, -10),
                                                           max_particles=len(x) + 64, penalty=1e3, **cfg))
        sim.add_particles(dict(type="rigid", **cs.BODIES2["box"]))
        sim.add_particles(dict(type="sand", positions=x, velocities=v, params=orc.group_params("sand", 400.0 * vol, vol)[0]))
    sim.run_substeps(50)
    sim.synchronize()
    t0 = time.perf_counter()
    sim.run_substeps(steps)
    sim.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    n = sim.get_num_particles()
    sim.close()
    print("RESULT %s %s %.5f %d" % (scene, variant, ms, n))


def table(parent, rounds, steps):
    variants = [("parent", parent), ("default", REPO), ("det", REPO)]
    got = {(s, v): [] for s in SCENES for v, _ in variants}
    for r in range(rounds):
        for s in SCENES:
            for v, root in variants:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", s, "--variant", v, "--root", root, "--steps", str(steps)],
                                     capture_output=True, text=True, timeout=600)
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
                if out.returncode != 0 or not line:
                    print(out.stdout[-2000:], out.stderr[-2000:])
                    raise SystemExit("measurement failed: %s %s" % (s, v))  # (nothing more is started on the GPU)
                got[(s, v)].append(float(line[0].split()[3]))
                live = line[0].split()[4]
        print("round %d done" % (r + 1), flush=True)
    print("ms per substep, %d rounds alternating parent / default / det, %d substeps each after 50 of warm-up" % (rounds, steps))
    for s in SCENES:
        for v, _ in variants:
            t = got[(s, v)]
            print("  %-9s %-8s %s   median %.4f  spread %.4f-%.4f" % (s, v, " ".join("%.4f" % q for q in t), statistics.median(t), min(t), max(t)))
        p, d, m = (statistics.median(got[(s, v)]) for v in ("parent", "default", "det"))
        lo, hi = min(got[(s, "parent")]), max(got[(s, "parent")])
        print("  %-9s default against parent: %.4f vs %.4f (parent's own spread %.4f-%.4f): %s;  mode against parent: %+.4f ms (%+.1f %%)"
              % (s, d, p, lo, hi, "inside" if lo <= d <= hi else "OUTSIDE", m - p, 100.0 * (m - p) / p))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--one", choices=SCENES)
    ap.add_argument("--variant", choices=("parent", "default", "det"), default="default")
    ap.add_argument("--root", default=REPO)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.variant, os.path.abspath(a.root), a.steps)
    else:
        table(os.path.abspath(a.parent), a.rounds, a.steps)
