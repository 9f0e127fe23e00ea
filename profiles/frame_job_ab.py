"""The frame of a job against the one-ctx encoder, on bench.py's c3 scene (256^3, 8 M sand) after 2 substeps (slots out of id order):
mpmhip_bgeo_encode on one ctx (ids to the host, ordered there, the order uploaded, rows gathered), mpmhip_bgeo_encode_group with K = 1
on the same ctx and with K = 8 on the 8 virtual ranks of the same particles.  Host clock around calls that end in a synchronise,
5 calls each; the group call's phases from the events it records (mpmhip_debug_frame_phases).  The record: profiles/frame_job_ab.txt.

    python profiles/frame_job_ab.py [--config c3] [--calls 5]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import taichi_mpm_amd as tm  # noqa: E402
from taichi_mpm_amd import tiled  # noqa: E402

PHASES = ("top", "mark", "prefix", "rows", "copy")


def timed(calls, fn):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def line(name, ms):
    print("%-58s min %9.3f  median %9.3f ms   (%s)" % (name, min(ms), float(np.median(ms)), " ".join("%.3f" % v for v in ms)), flush=True)


def group_calls(L, sims, buf, calls):
    K = len(sims)
    arr = (C.c_void_p * K)(*[s._ctx for s in sims])
    w = C.c_size_t()
    phases = []

    def call():
        rc = L.mpmhip_bgeo_encode_group(arr, K, 0, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(w))
        assert rc == 0, L.mpmhip_last_error(sims[0]._ctx)
        ms = (C.c_double * 5)()
        L.mpmhip_debug_frame_phases(ms)
        phases.append(list(ms))
    call()  # warm-up: code objects, the first allocations
    phases.clear()
    return timed(calls, call), np.asarray(phases), w.value


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    cfg = dict(bench.CONFIGS[args.config])
    L = tm.load()
    sim = bench.build_sim(tm, cfg, 0)
    sim.run_substeps(2)
    ids = sim.get_particles(sort_by_id=False)["id"]
    print("%s: %d particles, slots in id order: %s" % (args.config, len(ids), bool(np.all(np.diff(ids) > 0))), flush=True)
    n = C.c_size_t()
    sim._check(L.mpmhip_bgeo_size(sim._ctx, 0, C.byref(n)))
    buf, ref = np.zeros(n.value, np.uint8), np.zeros(n.value, np.uint8)
    w = C.c_size_t()

    def one():
        sim._check(L.mpmhip_bgeo_encode(sim._ctx, 0, ref.ctypes.data_as(C.c_void_p), ref.size, C.byref(w)))
    one()
    base = timed(args.calls, one)
    line("mpmhip_bgeo_encode, one ctx (%d MB)" % (n.value >> 20), base)
    ms, ph, wrote = group_calls(L, [sim], buf, args.calls)
    assert wrote == n.value and np.array_equal(buf, ref), "K = 1 must give the one-ctx file"
    line("mpmhip_bgeo_encode_group, K = 1, same ctx (same bytes)", ms)
    for k, name in enumerate(PHASES):
        line("    " + name, ph[:, k])
    print("    K = 1 / one ctx: %.3f (min), %.3f (median)" % (min(ms) / min(base), np.median(ms) / np.median(base)), flush=True)
    sim.close()

    K = 8
    part = tiled.scene_partition(cfg, K, margin=4)
    sims = [tiled.build_rank_sim(tm, cfg, part, r, 0)[0] for r in range(K)]
    job = tiled.NativeVirtualJob([tiled.HipEngine(s, 0) for s in sims], part, overlap=False)
    job.run(2)
    job.synchronize()
    print("8 virtual ranks: particles per rank %s" % [s.get_num_particles() for s in sims], flush=True)
    ms8, ph8, wrote8 = group_calls(L, sims, buf, args.calls)
    assert wrote8 == n.value
    line("mpmhip_bgeo_encode_group, K = 8 virtual ranks", ms8)
    for k, name in enumerate(PHASES):
        line("    " + name, ph8[:, k])
    print("    K = 8 / one ctx: %.3f (min), %.3f (median)" % (min(ms8) / min(base), np.median(ms8) / np.median(base)), flush=True)
    head, _ = tiled.frame_envelope(len(ids), 0)
    got = np.frombuffer(buf, ">u4", count=12 * len(ids), offset=len(head)).reshape(len(ids), 12)[:, 5]
    assert np.array_equal(got, np.sort(ids).astype(np.uint32)), "the K = 8 file must list the job's ids in ascending order"
    for s in sims:
        s.close()
