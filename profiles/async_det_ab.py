"""What the deterministic mode of the asynchronous stepper costs, and that the default mode did not get slower: ms per step() and per
advance of the resident 3D stepper — the parent commit's library in default mode, this tree in default mode, this tree in the mode —
taking turns on one GPU (the order inside a round rotates).
    python profiles/async_det_ab.py [--rounds 5] [--steps 8]            the table
    python profiles/async_det_ab.py --one parent|default|det [--steps 8]   one measurement (what the table spawns)
The parent's library runs under this tree's Python package: build it at the parent commit and copy it to
taichi_mpm_amd/lib/libmpmhip_parent.so; the measurement selects it with MPMHIP_LIB_VARIANT=parent.  Every measurement is a process
of its own: the scene of tests/test_gpu_async.py's million-particle test (128^3 grid, a soft Hencky-elastic slab next to a stiff sand
slab, 2 x 0.5 M particles, unit_delta_t 2e-6, max_units 256), 2 steps of warm-up, then --steps calls of step(DT) between two
synchronising state reads: wall clock / steps, and from the stepper's own profile (mpmhip_async_profile) the host time inside
advance() per advance.  A second pass of --steps steps with the profile's synchronisation on splits an advance into its substep and
the rest (gather, read-back, clear, compaction, filing): that pass is slower by the synchronisations and is only read for the split.
The bar for the default mode: its median inside the parent's own min-max."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("parent", "default", "det")
DT = 2e-4


def scene(tm, det):
    from tests.common import lattice_cube, make_state
    res = 128
    dx = 1.0 / res
    xa = lattice_cube(res, 30, 70, dx, jitter=0.2, seed=11)
    xa = xa[xa[:, 0] < 50 * dx]
    xb = lattice_cube(res, 30, 70, dx, jitter=0.2, seed=12)
    xb = xb[xb[:, 0] >= 50 * dx]
    sa = make_state(xa, "elastic", dx, perturb_F=0.01, vel_scale=0.5, seed=13)
    sb = make_state(xb, "sand", dx, perturb_F=0.01, vel_scale=0.5, seed=14)
    sim = tm.create_simulation3("async_mpm").initialize(dict(res=(res,) * 3, delta_x=dx, unit_delta_t=2e-6, max_units=256, deterministic=det))
    sim.set_levelset(tm.mpm.LevelSet(friction=0.4).add_plane((0, 1, 0), d=-0.2))
    for s, mat in ((sa, "elastic"), (sb, "sand")):
        sim.add_particles(dict(type=mat, positions=s.x, velocities=s.v, F=s.F, B=s.B, aux=s.aux, params=s.gparams[0]))
    return sim


def profile(sim, sync):
    o = (C.c_double * 6)()
    sim._check(sim._L.mpmhip_async_profile(sim._ctx, int(sync), o))
    return list(o)


def one(variant, steps):
    sys.path.insert(0, REPO)
    import taichi_mpm_amd as tm
    tm.load()
    sim = scene(tm, variant == "det")
    for _ in range(2):
        sim.step(DT)
    st0 = sim._state()  # (mpmhip_async_state settles the counters: the stream is idle)
    p0 = profile(sim, 0)
    t0 = time.perf_counter()
    for _ in range(steps):
        sim.step(DT)
    st = sim._state()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    p1 = profile(sim, 1)  # from here on the stream is synchronised behind every substep
    for _ in range(steps):
        sim.step(DT)
    sim._state()
    p2 = profile(sim, 0)
    adv = p1[5] - p0[5]
    adv2 = p2[5] - p1[5]
    sim.close()
    print("RESULT %s %.4f advance %.4f synced_advance %.4f synced_substep %.4f advances %d updates %d containers %d compactions %d" %
          (variant, ms, (p1[2] - p0[2]) / adv, (p2[2] - p1[2]) / adv2, (p2[3] - p1[3]) / adv2, adv, st[1] - st0[1], st[4], st[6]))


def table(rounds, steps):
    keys = ("step", "advance", "synced_advance", "synced_substep")
    got, facts = {v: {k: [] for k in keys} for v in VARIANTS}, {}
    for r in range(rounds):
        for v in VARIANTS[r % 3:] + VARIANTS[:r % 3]:  # (the order inside a round rotates: a process that follows another is not always the same variant)
            env = dict(os.environ)
            env.pop("MPMHIP_LIB_VARIANT", None)
            env.pop("MPMHIP_DETERMINISTIC", None)
            if v == "parent":
                env["MPMHIP_LIB_VARIANT"] = "parent"
            cmd = [sys.executable, os.path.abspath(__file__), "--one", v, "--steps", str(steps)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
            if out.returncode != 0 or not line:
                print(out.stdout[-2000:], out.stderr[-2000:])
                raise SystemExit("measurement failed: %s" % v)  # (nothing more is started on the GPU)
            w = line[0].split()
            got[v]["step"].append(float(w[2]))
            for k in keys[1:]:
                got[v][k].append(float(w[w.index(k) + 1]))
            facts[v] = " ".join(w[w.index("advances"):])
        print("round %d done" % (r + 1), flush=True)
    print("ms, %d rounds of parent / default / det in rotating order, %d steps of step(%g) each after 2 of warm-up" % (rounds, steps, DT))
    for k in keys:
        for v in VARIANTS:
            t = got[v][k]
            print("  %-15s %-8s %s   median %.4f  spread %.4f-%.4f" % (k, v, " ".join("%.4f" % q for q in t), statistics.median(t), min(t), max(t)))
    for v in VARIANTS:
        print("  %-8s %s" % (v, facts[v]))
    for k in ("step", "advance"):
        ta, m, d = got["parent"][k], statistics.median(got["default"][k]), statistics.median(got["det"][k])
        where = "inside" if min(ta) <= m <= max(ta) else ("BELOW" if m < min(ta) else "ABOVE")
        print("  %s: default against parent: %.4f vs %.4f (parent's own spread %.4f-%.4f): %s" % (k, m, statistics.median(ta), min(ta), max(ta), where))
        print("  %s: the mode against default: %.4f vs %.4f: %+.4f ms, %+.1f %%" % (k, d, m, d - m, 100.0 * (d - m) / m))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--one", choices=VARIANTS)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.steps)
    else:
        table(a.rounds, a.steps)
