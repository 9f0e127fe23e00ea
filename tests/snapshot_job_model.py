"""numpy model of the snapshot of a tiled job (include/mpmhip.h: "the snapshot of a whole tiled job"): the canonical form of an
MPMHIP01 blob, which records of a blob a rank of a partition keeps, and the job's blob assembled from the ranks' records.  No
library: the layout is restated here from csrc/snapshot_blob.h (header 80 bytes, group rows of 80, RecG 64, RecP 64, apic_b row 48;
group id and creation id at bytes 52 and 56 of a RecG)."""
import numpy as np

HEADER, GROUP, RECG, RECP, BROW = 80, 80, 64, 64, 48
ROW = RECG + RECP + BROW
# byte offsets of the header's fields (SnapHeader)
H_NGROUPS, H_NSLOTS, H_SUBSTEPS, H_NEXT_PID, H_B_STALE, H_STORE_B, H_RES, H_T, H_REQUEST_T, H_DX, H_DT, H_NDEAD = 12, 16, 24, 32, 36, 40, 44, 56, 60, 64, 68, 72
PID = 56


def parse(blob):
    """dict(head (80 bytes, writable copy), groups (bytes), rg [n][64], rp [n][64], rb [n][48] uint8, tail (bytes behind rb))"""
    b = np.frombuffer(bytes(blob), np.uint8)
    n_groups = int(b[H_NGROUPS:H_NGROUPS + 4].view(np.uint32)[0])
    n = int(b[H_NSLOTS:H_NSLOTS + 8].view(np.int64)[0])
    at = HEADER
    groups = b[at:at + GROUP * n_groups].tobytes()
    at += GROUP * n_groups
    out = dict(head=b[:HEADER].copy(), groups=groups)
    for name, w in (("rg", RECG), ("rp", RECP), ("rb", BROW)):
        out[name] = b[at:at + n * w].reshape(n, w)
        at += n * w
    out["tail"] = b[at:].tobytes()
    return out


def ids_of(rg):
    return np.ascontiguousarray(rg[:, PID:PID + 4]).view(np.int32).ravel()


def positions_of(rg):
    return np.ascontiguousarray(rg[:, :12]).view(np.float32).reshape(-1, 3)


def head_field(head, off, dtype):
    return np.asarray(head[off:off + np.dtype(dtype).itemsize]).view(dtype)[0]


def _put(head, off, value, dtype):
    head[off:off + np.dtype(dtype).itemsize] = np.array([value], dtype).view(np.uint8)


def build(head, groups, rg, rp, rb):
    return head.tobytes() + bytes(groups) + np.ascontiguousarray(rg).tobytes() + np.ascontiguousarray(rp).tobytes() + np.ascontiguousarray(rb).tobytes()


def canonical(blob):
    """the blob without its dead slots, rows stable-sorted by creation id, n_slots = the live rows, n_dead = 0, next_pid =
    max(the blob's, 1 + the largest live id).  A tail (rigid bodies) is not carried: a job has none."""
    p = parse(blob)
    ids = ids_of(p["rg"])
    live = np.nonzero(ids >= 0)[0]
    order = live[np.argsort(ids[live], kind="stable")]
    head = p["head"]
    _put(head, H_NSLOTS, len(order), np.int64)
    _put(head, H_NDEAD, 0, np.uint32)
    nxt = int(head_field(head, H_NEXT_PID, np.int32))
    _put(head, H_NEXT_PID, max(nxt, int(ids[order].max()) + 1 if len(order) else 0), np.int32)
    return build(head, p["groups"], p["rg"][order], p["rp"][order], p["rb"][order])


def placeable(blob, dx):
    """mask over the blob's slots: live, position finite and at or above half a cell on every axis (fp32, the device's product)"""
    p = parse(blob)
    x = positions_of(p["rg"])
    with np.errstate(invalid="ignore", over="ignore"):
        X = x * np.float32(1.0 / dx)
        ok = np.isfinite(X).all(1) & (X >= np.float32(0.5)).all(1)
    return (ids_of(p["rg"]) >= 0) & ok


def owned(blob, part, rank, dx):
    """indices, in blob order, of the slots rank `rank` of `part` keeps: placeable, base cell (tiled.base_cells) in its brick"""
    from taichi_mpm_amd import tiled
    p = parse(blob)
    ok = placeable(blob, dx)
    x = np.where(ok[:, None], positions_of(p["rg"]), np.float32(1.0))  # (the others are nobody's: any finite stand-in)
    owner = part.rank_of_cells(tiled.base_cells(x, dx))
    return np.nonzero(ok & (owner == rank))[0]


def assemble(head, groups, parts):
    """the job's blob: head (80 bytes of a rank, next_pid already the ranks' maximum), groups (bytes), parts = [(row numbers,
    records [n_r][176])]; the numbers must be a permutation of 0 .. n - 1 (ValueError otherwise)"""
    idx = np.concatenate([np.asarray(i, np.int64).reshape(-1) for i, _ in parts]) if parts else np.zeros(0, np.int64)
    rows = np.concatenate([np.asarray(r, np.uint8).reshape(-1, ROW) for _, r in parts]) if parts else np.zeros((0, ROW), np.uint8)
    n = len(idx)
    if len(rows) != n or not np.array_equal(np.sort(idx), np.arange(n)):
        raise ValueError("row numbers are no permutation of 0 .. %d" % (n - 1))
    out = np.empty((n, ROW), np.uint8)
    out[idx] = rows
    h = np.frombuffer(bytes(head), np.uint8).copy()
    _put(h, H_NSLOTS, n, np.int64)
    _put(h, H_NDEAD, 0, np.uint32)
    ids = ids_of(out[:, :RECG])
    _put(h, H_NEXT_PID, max(int(head_field(h, H_NEXT_PID, np.int32)), int(ids.max()) + 1 if n else 0), np.int32)
    return build(h, groups, out[:, :RECG], out[:, RECG:RECG + RECP], out[:, RECG + RECP:])


def rows_of(blob):
    """(ids, records [n][176]) of the live slots of a one-ctx blob, in slot order: what a rank contributes to the job's blob"""
    p = parse(blob)
    ids = ids_of(p["rg"])
    live = np.nonzero(ids >= 0)[0]
    return ids[live], np.concatenate([p["rg"][live], p["rp"][live], p["rb"][live]], axis=1)


def job_row_numbers(rank_ids):
    """per rank the row number of each of its ids in the job's blob: the number of the job's ids below it"""
    allids = np.sort(np.concatenate([np.asarray(i, np.int64) for i in rank_ids])) if rank_ids else np.zeros(0, np.int64)
    return [np.searchsorted(allids, np.asarray(i, np.int64)) for i in rank_ids]
