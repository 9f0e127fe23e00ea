"""numpy restatements of what orders the containers of the asynchronous steppers in the deterministic mode (csrc/k_async.h):
async_block_of — the scheduler block of a position — and the ordered stream compaction of the four ordered kernels, walked the
way the device walks it (chunks of 1024 elements dealt round-robin to the workgroups, a chained exclusive scan of the chunk sums).
Shared by tests/test_async_order_cpu.py (the models against hand-computed values and a brute-force loop) and
tests/test_gpu_async_deterministic.py (the device against the models)."""
import numpy as np

INVALID = 0xFFFFFFFF
BLOCK_SHIFT = {2: (3, 4), 3: (2, 2, 3)}  # ASYNC_BLOCK_SHIFT: a scheduler block is 8 x 16 nodes in 2D, 4 x 4 x 8 in 3D
CHUNK = 1024


def block_counts(res, dim):
    """blocks per axis of the dense table (AsyncSched::nb)"""
    return tuple((int(res) >> s) + 1 for s in BLOCK_SHIFT[dim])


def async_block_of(x, res, dim):
    """k_async.h: async_block_of<D> for positions x [n, dim] on a res^dim grid with delta_x = 1 / res, in fp32 as the device
    computes it: the block holding the particle's base node, INVALID (as int64) below half a cell or outside the table"""
    x = np.asarray(x, np.float32).reshape(-1, dim)
    idx = np.float32(1.0) / np.float32(1.0 / res)
    X = x * idx  # fp32
    nb = block_counts(res, dim)
    ok = np.all(X >= np.float32(0.5), axis=1)
    base = (np.where(ok[:, None], X, np.float32(0.5)) - np.float32(0.5)).astype(np.int32)  # (int) truncates; X - 0.5 >= 0 here
    b = np.stack([base[:, k] >> BLOCK_SHIFT[dim][k] for k in range(dim)], 1).astype(np.int64)
    ok &= np.all(b < np.asarray(nb, np.int64)[None, :], axis=1)
    flat = b[:, 0] * nb[1] + b[:, 1]
    if dim == 3:
        flat = flat * nb[2] + b[:, 2]
    return np.where(ok, flat, INVALID).astype(np.int64)


def ordered_slots(flags, wgs, base=0):
    """slot of every flagged element (-1 for the others) and the end of the output, computed as the ordered kernels do: chunk c
    of 1024 elements belongs to workgroup c % wgs, which walks its chunks in ascending order; a chunk publishes its count (chunk 0
    with `base` folded in) and starts at the sum of what the chunks before it published"""
    flags = np.asarray(flags, bool)
    n = len(flags)
    nchunks = (n + CHUNK - 1) // CHUNK
    published = np.zeros(nchunks, np.int64)
    slots = np.full(n, -1, np.int64)
    # every workgroup's walk; a chunk only reads the words of earlier chunks, so any interleaving of the walks gives the same
    # result: the model takes the workgroups one after the other in two passes (publish, then place)
    for wg in range(min(wgs, max(nchunks, 1))):
        for c in range(wg, nchunks, wgs):
            published[c] = int(flags[c * CHUNK:(c + 1) * CHUNK].sum()) + (base if c == 0 else 0)
    end = base
    for wg in range(min(wgs, max(nchunks, 1))):
        for c in range(wg, nchunks, wgs):
            f = flags[c * CHUNK:(c + 1) * CHUNK]
            pre = int(published[:c].sum()) + (base if c == 0 else 0)
            excl = np.cumsum(f) - f
            slots[c * CHUNK:(c + 1) * CHUNK] = np.where(f, pre + excl, -1)
            if c == nchunks - 1:
                end = pre + int(f.sum())
    return slots, end


def pooled_store(batches, res, dim, wgs=4096, next_id=0):
    """the pools after the batches of positions were added and pooled one after the other, before any step: (ids, blocks) of
    the containers in store order — every batch is filed behind the store's end in ascending slot, without the positions
    async_block_of drops; creation ids count through all positions, dropped ones included"""
    ids, blks = [], []
    size = 0
    for x in batches:
        b = async_block_of(x, res, dim)
        slots, end = ordered_slots(b != INVALID, wgs, base=size)
        kept = np.flatnonzero(b != INVALID)
        assert np.array_equal(slots[kept], size + np.arange(len(kept)))  # (what a compaction is)
        ids.append(next_id + kept)
        blks.append(b[kept])
        next_id += len(b)
        size = end
    return np.concatenate(ids).astype(np.int64), np.concatenate(blks).astype(np.int64)
