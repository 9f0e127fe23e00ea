"""The snapshot of a job against the route a tiled job had before it, on bench.py's c3 scene (256^3, 8 M sand) after 2 substeps, as
K = 1 (one ctx) and as 8 virtual ranks of the same particles.  Host clock around calls that end in a synchronise, 5 calls each.

  save   old route: mpmhip_snapshot_save on every rank's ctx (K blobs, tied to the bricks, dead slots included)
         new:       mpmhip_snapshot_save_group (ONE canonical blob)
  load   old route: the one-ctx blob filtered on the host (tiled.base_cells, Partition.rank_of_cells), every rank cleared and filled
                    with add_particles + upload(F_ID); K = 1: mpmhip_snapshot_load
         new:       mpmhip_snapshot_load_brick on every rank with the same bytes

--old-only times the old routes alone: they use entry points the parent commit has, so the same script runs on the parent's library
(MPMHIP_LIB_VARIANT).  What the kernels cost beside the host copies: run the script under `rocprofv3 --kernel-trace --stats`.
The record: profiles/snapshot_job_ab.txt.

    python profiles/snapshot_job_ab.py [--config c3] [--calls 5] [--old-only]
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
from taichi_mpm_amd import _lib, tiled  # noqa: E402
from taichi_mpm_amd.mpm import F_ID  # noqa: E402


def timed(calls, fn):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def line(name, ms):
    print("%-66s min %10.3f  median %10.3f ms   (%s)" % (name, min(ms), float(np.median(ms)), " ".join("%.1f" % v for v in ms)), flush=True)


def one_blob(sim, buf=None):
    n = int(sim._check(sim._L.mpmhip_snapshot_size(sim._ctx)))
    buf = np.empty(n, np.uint8) if buf is None or buf.size < n else buf
    sim._check(sim._L.mpmhip_snapshot_save(sim._ctx, buf.ctypes.data_as(C.c_void_p), buf.size))
    return buf[:n]


def fields_of(blob):
    """(x, v, F, B, aux, gid, id, material, params) of the live records of a one-group blob"""
    h = _lib.SnapHeader.from_buffer_copy(blob[:80].tobytes())
    n, at = int(h.n_slots), 80 + 80 * int(h.n_groups)
    rg = blob[at:at + 64 * n].reshape(n, 64)
    rp = blob[at + 64 * n:at + 128 * n].reshape(n, 64)
    rb = blob[at + 128 * n:at + 176 * n].reshape(n, 48)
    f = np.ascontiguousarray(rg).view(np.float32).reshape(n, 16)
    p = np.ascontiguousarray(rp).view(np.float32).reshape(n, 16)
    b = np.ascontiguousarray(rb).view(np.float32).reshape(n, 12)
    ids = np.ascontiguousarray(rg[:, 56:60]).view(np.int32).ravel()
    live = ids >= 0
    return dict(x=f[live, 0:3], aux=f[live, 3], F=f[live, 4:13], v=p[live, 3:6], B=b[live, 0:9], id=ids[live])


def host_filter_load(sims, part, blob, cfg, dx):
    """the old route to the state of a job: filter on the host, fill every rank again"""
    d = fields_of(blob)
    owner = part.rank_of_cells(tiled.base_cells(d["x"], dx)) if part is not None else np.zeros(len(d["id"]), np.int64)
    for r, sim in enumerate(sims):
        m = owner == r
        sim._check(sim._L.mpmhip_clear_particles(sim._ctx))
        sim._n_added = 0
        sim.add_particles(dict(type=cfg["material"], positions=d["x"][m], velocities=d["v"][m], F=d["F"][m], B=d["B"][m], aux=d["aux"][m]))
        if m.any():
            sim.upload(F_ID, np.ascontiguousarray(d["id"][m]))
        sim.synchronize()


def group_save(L, sims, buf):
    K = len(sims)
    arr = (C.c_void_p * K)(*[s._ctx for s in sims])
    w = C.c_size_t()
    rc = L.mpmhip_snapshot_save_group(arr, K, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(w))
    assert rc == 0, [L.mpmhip_last_error(s._ctx) for s in sims]
    return w.value


def brick_load(sims, blob):
    kept = []
    for sim in sims:
        info = (C.c_int64 * 4)()
        sim._check(sim._L.mpmhip_snapshot_load_brick(sim._ctx, blob.ctypes.data_as(C.c_void_p), blob.size, info))
        kept.append(int(info[0]))
    for sim in sims:
        sim.synchronize()
    return kept


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--old-only", action="store_true")
    args = ap.parse_args()
    cfg = dict(bench.CONFIGS[args.config])
    dx = 1.0 / cfg["res"]
    L = tm.load()
    print("library: %s" % _lib.lib_path(), flush=True)

    # ---- K = 1
    sim = bench.build_sim(tm, cfg, 0)
    sim.run_substeps(2)
    sim.synchronize()
    blob = one_blob(sim).copy()
    mb = blob.size >> 20
    print("%s: %d particles, blob %d MB" % (args.config, sim.get_num_particles(), mb), flush=True)
    buf = np.empty(blob.size, np.uint8)
    line("save K = 1, old: mpmhip_snapshot_save", timed(args.calls, lambda: one_blob(sim, buf)))
    if not args.old_only:
        group_save(L, [sim], buf)
        line("save K = 1, new: mpmhip_snapshot_save_group", timed(args.calls, lambda: group_save(L, [sim], buf)))
        canon = buf.copy()
        ids = fields_of(canon)["id"]
        assert len(ids) == sim.get_num_particles() and np.all(np.diff(ids) > 0), "the job's blob lists the ids in ascending order"
    line("load K = 1, old: mpmhip_snapshot_load", timed(args.calls, lambda: (sim._check(L.mpmhip_snapshot_load(sim._ctx, blob.ctypes.data_as(C.c_void_p), blob.size)), sim.synchronize())))
    if not args.old_only:
        tiled.set_partition(sim, tiled.Partition((cfg["res"],) * 3, (1, 1, 1), [[0, cfg["res"]]] * 3, 4), 0)
        brick_load([sim], blob)
        line("load K = 1, new: mpmhip_snapshot_load_brick", timed(args.calls, lambda: brick_load([sim], blob)))
    sim.close()

    # ---- 8 virtual ranks
    K = 8
    part = tiled.scene_partition(cfg, K, margin=4)
    sims = [tiled.build_rank_sim(tm, cfg, part, r, 0)[0] for r in range(K)]
    job = tiled.NativeVirtualJob([tiled.HipEngine(s, 0) for s in sims], part, overlap=False)
    job.run(2)
    job.synchronize()
    print("8 virtual ranks: particles per rank %s" % [s.get_num_particles() for s in sims], flush=True)
    bufs = [np.empty(int(s._check(L.mpmhip_snapshot_size(s._ctx))), np.uint8) for s in sims]
    line("save K = 8, old: mpmhip_snapshot_save on every rank (8 blobs)", timed(args.calls, lambda: [one_blob(s, b) for s, b in zip(sims, bufs)]))
    if not args.old_only:
        group_save(L, sims, buf)
        line("save K = 8, new: mpmhip_snapshot_save_group (one blob)", timed(args.calls, lambda: group_save(L, sims, buf)))
        assert np.array_equal(fields_of(buf)["id"], ids), "K = 8 saves the ids K = 1 saved"
    src = blob if args.old_only else canon
    host_filter_load(sims, part, src, cfg, dx)
    line("load K = 8, old: host filter + add_particles + upload(F_ID)", timed(max(2, args.calls // 2), lambda: host_filter_load(sims, part, src, cfg, dx)))
    print("    per rank after the old route: %s" % [s.get_num_particles() for s in sims], flush=True)
    if not args.old_only:
        kept = brick_load(sims, src)
        line("load K = 8, new: mpmhip_snapshot_load_brick on every rank", timed(args.calls, lambda: brick_load(sims, src)))
        print("    per rank after the new route: %s" % kept, flush=True)
    for s in sims:
        s.close()
