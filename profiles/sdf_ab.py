"""What the sampled level set costs: ms per substep of the C3 scene (256^3 grid, 100^3 cells x 8 = 8 M sand particles) resting on its
floor, the parent commit's library and this tree's alternating on one GPU.
    python profiles/sdf_ab.py --parent DIR [--rounds 5] [--steps 200]    the table (DIR: a built copy of the parent tree)
    python profiles/sdf_ab.py --one VARIANT [--root DIR]                 one measurement (what the table spawns, and what a
                                                                         rocprofv3 --kernel-trace --stats run wraps)
Variants:  none       no level set (parent and this tree: the three hot kernels are instruction-identical, so this tree must sit
                      inside the parent's own run-to-run spread)
           plane      the floor y = 0.1 as an analytic plane            plane_pc   ... with particle_collision
           sdf        the same plane baked at 257^3 samples, spacing dx sdf_pc     ... with particle_collision
Every measurement is a process of its own under its own time limit; a failed one ends the run (nothing more is started on the GPU).
Scene set-up, 50 substeps warm-up, then --steps substeps between two synchronisations, wall clock / steps."""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("none", "plane", "sdf", "plane_pc", "sdf_pc")
RES, CELLS, FLOOR = 256, 100, 0.1


def one(variant, root, steps):
    sys.path.insert(0, root)
    import taichi_mpm_amd as tm
    tm.load()
    dx = 1.0 / RES
    sim = tm.create_simulation3("mpm").initialize(dict(res=(RES,) * 3, delta_x=dx, base_delta_t=1e-4, gravity=(0, -10, 0),
                                                       particle_collision=variant.endswith("_pc")))
    if variant != "none":
        ls = tm.mpm.LevelSet(friction=-1.0, delta_x=dx).add_plane((0, 1, 0), d=-FLOOR)
        if variant.startswith("sdf"):
            ls = tm.mpm.SampledLevelSet.from_levelset(ls, (RES + 1,) * 3)
        sim.set_levelset(ls)
    lo = RES // 2 - CELLS // 2
    sim.add_particles(dict(type="sand", cube_lo=(lo, int(FLOOR * RES) + 1, lo), cube_cells=CELLS))  # the block stands on the floor
    sim.run_substeps(50)
    sim.synchronize()
    t0 = time.perf_counter()
    sim.run_substeps(steps)
    sim.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    n = sim.get_num_particles()
    sim.close()
    print("RESULT %s %.5f %d" % (variant, ms, n))


def table(parent, rounds, steps):
    runs = [("none", "parent", parent)] + [(v, "this", REPO) for v in VARIANTS]
    got = {(v, who): [] for v, who, _ in runs}
    for r in range(rounds):
        for v, who, root in runs:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", v, "--root", root, "--steps", str(steps)],
                                 capture_output=True, text=True, timeout=300)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
            if out.returncode != 0 or not line:
                print(out.stdout[-2000:], out.stderr[-2000:])
                raise SystemExit("measurement failed: %s %s" % (v, who))  # (nothing more is started on the GPU)
            got[(v, who)].append(float(line[0].split()[2]))
        print("round %d done" % (r + 1), flush=True)
    print("ms per substep, %d rounds alternating, %d substeps each after 50 of warm-up" % (rounds, steps))
    med = {}
    for v, who, _ in runs:
        t = got[(v, who)]
        med[(v, who)] = statistics.median(t)
        print("  %-9s %-6s %s   median %.4f  spread %.4f-%.4f" % (v, who, " ".join("%.4f" % q for q in t), med[(v, who)], min(t), max(t)))
    lo, hi = min(got[("none", "parent")]), max(got[("none", "parent")])
    d = med[("none", "this")]
    print("  no level set, this tree against parent: %.4f vs %.4f (parent's own spread %.4f-%.4f): %s"
          % (d, med[("none", "parent")], lo, hi, "inside" if lo <= d <= hi else "OUTSIDE"))
    for a, b in (("plane", "sdf"), ("plane_pc", "sdf_pc")):
        p, s = med[(a, "this")], med[(b, "this")]
        print("  %s against %s: %.4f vs %.4f ms: %+.4f ms (%+.1f %%)" % (b, a, s, p, s - p, 100.0 * (s - p) / p))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--one", choices=VARIANTS)
    ap.add_argument("--root", default=REPO)
    a = ap.parse_args()
    if a.one:
        one(a.one, os.path.abspath(a.root), a.steps)
    else:
        table(os.path.abspath(a.parent), a.rounds, a.steps)
