"""ms per step() of the resident asynchronous stepper, the parent commit's library and this tree's alternating on one GPU.
    python profiles/async_ab.py [--rounds 5] [--steps 8] [--scenes async3d,async2d]     the table
    python profiles/async_ab.py --one SCENE --variant parent|result [--steps 8]          one measurement (what the table spawns)
The parent's library runs under this tree's Python package: build it at the parent commit and copy it to
taichi_mpm_amd/lib/libmpmhip_parent.so; the measurement selects it with MPMHIP_LIB_VARIANT=parent.  Every measurement is a process
of its own: scene set-up, 2 steps of warm-up, then --steps calls of step(DT) between two synchronisations, wall clock / steps.
  async3d: the two-stiffness scene of tests/test_gpu_async.py's million-particle test (128^3 grid, soft Hencky-elastic slab next to a
           stiff sand slab, unit_delta_t 2e-6, max_units 256)
  async2d: 1024^2 grid, a soft elastic square next to a stiff sand square, 360^2 cells x 4 particles each = 1.04 M particles
           (the scene of tests/test_gpu_async2d.py at eight times the resolution; unit_delta_t 2e-6, max_units 1024)
The bar: the result's median inside the parent's own min-max of the same call."""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ("async3d", "async2d")
VARIANTS = ("parent", "result")
DT = 2e-4


def scene3d(tm):
    from tests.common import lattice_cube, make_state
    res = 128
    dx = 1.0 / res
    xa = lattice_cube(res, 30, 70, dx, jitter=0.2, seed=11)
    xa = xa[xa[:, 0] < 50 * dx]
    xb = lattice_cube(res, 30, 70, dx, jitter=0.2, seed=12)
    xb = xb[xb[:, 0] >= 50 * dx]
    sa = make_state(xa, "elastic", dx, perturb_F=0.01, vel_scale=0.5, seed=13)
    sb = make_state(xb, "sand", dx, perturb_F=0.01, vel_scale=0.5, seed=14)
    sim = tm.create_simulation3("async_mpm").initialize(dict(res=(res,) * 3, delta_x=dx, unit_delta_t=2e-6, max_units=256))
    sim.set_levelset(tm.mpm.LevelSet(friction=0.4).add_plane((0, 1, 0), d=-0.2))
    for s, mat in ((sa, "elastic"), (sb, "sand")):
        sim.add_particles(dict(type=mat, positions=s.x, velocities=s.v, F=s.F, B=s.B, aux=s.aux, params=s.gparams[0]))
    return sim


def scene2d(tm):
    from tests.golden.make_golden import mpm2d_state
    res = 1024
    dx = 1.0 / res
    vol = dx * dx / 4
    sim = tm.create_simulation2("async_mpm").initialize(dict(res=(res, res), delta_x=dx, unit_delta_t=2e-6, max_units=1024))
    sim.set_levelset(tm.mpm.LevelSet(friction=0.4).add_plane((0, 1, 0), d=-0.2))
    for mat, lo, seed in (("elastic", (152, 320), 3), ("sand", (512, 320), 4)):
        x, v, F, B = mpm2d_state(res, lo=lo, cells=360, seed=seed)
        gp, _ = tm.group_params(mat, 400 * vol, vol)
        sim.add_particles(dict(type=mat, positions=x, velocities=0.3 * v, F=F, B=B, params=gp))
    return sim


def one(scene, variant, steps):
    sys.path.insert(0, REPO)
    import taichi_mpm_amd as tm
    tm.load()
    sim = scene3d(tm) if scene == "async3d" else scene2d(tm)
    for _ in range(2):
        sim.step(DT)
    st0 = sim._state()  # (mpmhip*_async_state settles the counters: the stream is idle)
    t0 = time.perf_counter()
    for _ in range(steps):
        sim.step(DT)
    st = sim._state()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    sim.close()
    print("RESULT %s %s %.4f updates %d containers %d compactions %d" % (scene, variant, ms, st[1] - st0[1], st[4], st[6]))


def table(rounds, steps, scenes):
    got, facts = {(s, v): [] for s in scenes for v in VARIANTS}, {}
    for r in range(rounds):
        for s, v in got:
            env = dict(os.environ)
            env.pop("MPMHIP_LIB_VARIANT", None)
            if v == "parent":
                env["MPMHIP_LIB_VARIANT"] = "parent"
            cmd = [sys.executable, os.path.abspath(__file__), "--one", s, "--variant", v, "--steps", str(steps)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
            if out.returncode != 0 or not line:
                print(out.stdout[-2000:], out.stderr[-2000:])
                raise SystemExit("measurement failed: %s %s" % (s, v))  # (nothing more is started on the GPU)
            got[(s, v)].append(float(line[0].split()[3]))
            facts[(s, v)] = " ".join(line[0].split()[4:])
        print("round %d done" % (r + 1), flush=True)
    print("ms per step(%g), %d rounds alternating parent / result, %d steps each after 2 of warm-up" % (DT, rounds, steps))
    for s in scenes:
        for v in VARIANTS:
            t = got[(s, v)]
            print("  %-8s %-7s %s   median %.4f  spread %.4f-%.4f   (%s)" % (s, v, " ".join("%.4f" % q for q in t), statistics.median(t), min(t), max(t), facts[(s, v)]))
        ta, m = got[(s, "parent")], statistics.median(got[(s, "result")])
        where = "inside" if min(ta) <= m <= max(ta) else ("BELOW" if m < min(ta) else "ABOVE")
        print("  %-8s result against parent: %.4f vs %.4f (parent's own spread %.4f-%.4f): %s" % (s, m, statistics.median(ta), min(ta), max(ta), where))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--scenes", default=",".join(SCENES), help="the table's scenes, comma-separated")
    ap.add_argument("--one", choices=SCENES)
    ap.add_argument("--variant", choices=VARIANTS, default="result")
    a = ap.parse_args()
    if a.one:
        one(a.one, a.variant, a.steps)
    else:
        table(a.rounds, a.steps, a.scenes.split(","))
