"""What voxelising a mesh on the device costs, against what a user did before it existed (a point-to-mesh distance in numpy on the
host plus the upload of the array through mpmhip_set_levelset_sdf) and against the substeps of one frame.
    python profiles/mesh_sdf_ab.py [--out profiles/mesh_sdf_ab.txt]    the table (one process per case, each under its own time limit)
    python profiles/mesh_sdf_ab.py --one CASE                          one case (what the table spawns, and what a
                                                                       rocprofv3 --kernel-trace --stats run wraps)
Cases:  big5k    257^3 lattice on the nodes of a 256^3 grid, icosphere of 5 120 triangles, band = 3 dx + 2 spacing
        big82k   the same lattice, 81 920 triangles
        small    65^3 lattice, 1 280 triangles, band = +inf (every tile reads every triangle)
Per case: the warm mpmhip_set_levelset_mesh call between two device events on the ctx's stream (first call apart: it allocates),
REPEATS times, median and spread; the upload of one key frame of that lattice through mpmhip_set_levelset_sdf (wall clock); the
float64 numpy model (tests/mesh_sdf_model.py) on the host — in full for `small`, on every 4th sample per axis for `big5k` and
scaled by the sample count (marked extrapolated), not for `big82k`; and for the big lattice the ms per substep of the C3 block
(8 M sand particles) with that level set installed, so a per-frame moving mesh (two voxelisations per frame) can be weighed against
the frame's substeps.  A failed case ends the run: nothing more is started on the GPU."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CASES = {"big5k": (256, 4, False), "big82k": (256, 6, False), "small": (64, 3, True)}  # grid res, icosphere subdivisions, band = inf
REPEATS = 7


class Events:
    """two device events on a stream of our own, which the ctx is told to use"""

    def __init__(self, sim):
        self.hip = C.CDLL("libamdhip64.so")
        self.stream, self.e0, self.e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._ok(self.hip.hipStreamCreate(C.byref(self.stream)))
        self._ok(self.hip.hipEventCreate(C.byref(self.e0)))
        self._ok(self.hip.hipEventCreate(C.byref(self.e1)))
        sim._check(sim._L.mpmhip_set_stream(sim._ctx, self.stream))

    @staticmethod
    def _ok(rc):
        if rc != 0:
            raise SystemExit("HIP call failed: %d" % rc)

    def time(self, f):
        self._ok(self.hip.hipEventRecord(self.e0, self.stream))
        f()
        self._ok(self.hip.hipEventRecord(self.e1, self.stream))
        self._ok(self.hip.hipEventSynchronize(self.e1))
        ms = C.c_float()
        self._ok(self.hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1))
        return ms.value


def one(case):
    import taichi_mpm_amd as tm
    from tests import mesh_sdf_model as M
    tm.load()
    res, sub, inf = CASES[case]
    dx = 1.0 / res
    lat = ((res + 1,) * 3, (0.0, 0.0, 0.0), dx)
    band = float("inf") if inf else 3 * dx + 2 * dx
    tri = M.icosphere(sub, 0.25, (0.5, 0.3, 0.5)).astype(np.float32)
    sim = tm.create_simulation3("mpm").initialize(dict(res=(res,) * 3, delta_x=dx, base_delta_t=1e-4, gravity=(0, -10, 0)))
    sim._ensure_ctx()
    ev = Events(sim)
    mesh = tm.MeshLevelSet(tri, *lat, band=band, friction=0.4)
    first = ev.time(lambda: sim.set_levelset(mesh))
    warm = [ev.time(lambda: sim.set_levelset(mesh)) for _ in range(REPEATS)]
    print("RESULT %s voxelise_ms first %.3f warm median %.3f spread %.3f-%.3f (%d triangles, %d^3 samples)"
          % (case, first, statistics.median(warm), min(warm), max(warm), len(tri), res + 1))
    phi = sim.download_levelset_sdf()[0]
    arr = tm.SampledLevelSet(phi, lat[1], lat[2], 0.4)
    up = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        sim.set_levelset(arr)
        sim.synchronize()
        up.append((time.perf_counter() - t0) * 1e3)
    print("RESULT %s upload_ms median %.3f spread %.3f-%.3f (%.1f MB per key frame)" % (case, statistics.median(up), min(up), max(up), phi.nbytes / 1e6))
    if case != "big82k":
        stride = 1 if case == "small" else 4
        ax = [a[::stride].astype(np.float64) for a in M.lattice_axes(*lat)]
        pts = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
        t0 = time.perf_counter()
        d = M.distance(tri, pts)
        M.parity(tri, *lat)
        host = time.perf_counter() - t0
        sub_dev = np.abs(phi[::stride, ::stride, ::stride]).reshape(-1).astype(np.float64)
        near = sub_dev < band
        print("RESULT %s host_model_s %.2f on %d samples -> %.1f s for the lattice%s; max |device - model| within the band %.3g"
              % (case, host, len(pts), host * phi.size / len(pts), "" if stride == 1 else " (extrapolated)", np.abs(d - sub_dev)[near].max()))
    if res == 256:
        sim.set_levelset(mesh)
        lo = res // 2 - 50
        sim.add_particles(dict(type="sand", cube_lo=(lo, int(0.56 * res), lo), cube_cells=100))  # the C3 block, above the sphere
        sim.run_substeps(50)
        sim.synchronize()
        t = []
        for _ in range(3):
            ms = ev.time(lambda: sim.run_substeps(100))
            t.append(ms / 100)
        print("RESULT %s substep_ms median %.4f spread %.4f-%.4f (%d particles; a frame of 100 substeps: %.1f ms)"
              % (case, statistics.median(t), min(t), max(t), sim.get_num_particles(), 100 * statistics.median(t)))
    sim.close()


def table(out):
    lines = []
    for case in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", case], capture_output=True, text=True, timeout=420)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")]
        if r.returncode != 0 or not got:
            print(r.stdout[-2000:], r.stderr[-2000:])
            raise SystemExit("case %s failed" % case)  # (nothing more is started on the GPU)
        lines += got
        print("\n".join(got), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("# python profiles/mesh_sdf_ab.py — MI355X; times in ms unless named otherwise; %d repeats per figure\n" % REPEATS)
        fh.write("\n".join(ln[len("RESULT "):] for ln in lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=sorted(CASES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_sdf_ab.txt"))
    a = ap.parse_args()
    if a.one:
        one(a.one)
    else:
        table(a.out)
