"""A numpy model of everything the device's sort (csrc/k_sort.h) leaves behind, and the comparator that holds a view of the device's
tables (mpmhip_debug_sort_info / mpmhip_debug_sort_array) against it.  Everything is an integer: nothing is approximate.

model(ids, x, v, res, dx, clean_boundary) follows the rules as the kernels state them:
  key          particle_key of csrc/mpm_common.h (tests/common.py: sort_key), -1 for a slot the device deletes
  act_blk      the sorted distinct block keys; bits / wprefix: the bitmap (bit b of word w = block 32 w + b) and the active blocks
               with a key below 32 w
  cell_start   exclusive prefix of the per-cell counts over cidx = 64 slot(block) + cell, sentinel at [64 na]; act_start = every 64th
  nbr          27 neighbour slots per block (INVALID: inactive, a negative coordinate, or a key >= 32 nbw), [27] the block's key, [28]
               the owner mask by lower_sources (k_sort.h): bit o is set when no neighbour b + o - q, q < o, is active
  own_list     8 a + o of every set mask bit, ascending
  chunk_blk    the block whose range of the sorted index holds position 256 k
"""
import numpy as np

from tests.common import sort_key

INVALID = 0xFFFFFFFF
BC = 64
ARRAYS = ("slot_id", "bits", "wprefix", "act_blk", "act_start", "cell_start", "perm", "nbr", "own_list", "chunk_blk")
INFO = ("n_slots", "n_sorted", "n_active", "n_dead", "error", "rank_mode", "n_own", "keyed", "list", "ct", "cell_order", "ids_cached",
        "list_valid", "nbw", "max_blocks", "kbits")


def grid_bits(res):
    """(kbits, nbw) of a grid: Morton bits per axis and words of the block bitmap (mpmhip_create)"""
    maxnb = max((int(r) + 4) // 4 + 1 for r in res)
    kbits = 1
    while (1 << kbits) < maxnb:
        kbits += 1
    return kbits, max(1, (1 << (3 * kbits)) // 32)


def _spread(v):
    r = np.zeros_like(v)
    for b in range(10):
        r |= ((v >> b) & 1) << (3 * b)
    return r


def _compact(m):
    r = np.zeros_like(m)
    for b in range(10):
        r |= ((m >> (3 * b)) & 1) << b
    return r


def morton3(bx, by, bz):
    return (_spread(bx) << 2) | (_spread(by) << 1) | _spread(bz)


def demorton3(m):
    return _compact(m >> 2), _compact(m >> 1), _compact(m)


def lower_sources(o):
    """bits (of the 27-neighbour mask) of the blocks that own candidate o before this block does (k_sort.h)"""
    m = 0
    for q in range(o):
        d = ((o >> 2) - (q >> 2), ((o >> 1) & 1) - ((q >> 1) & 1), (o & 1) - (q & 1))
        m |= 1 << (((d[0] + 1) * 3 + (d[1] + 1)) * 3 + (d[2] + 1))
    return m


def model(ids, x, v, res, dx, clean_boundary):
    ids = np.asarray(ids, np.int64)
    res = tuple(int(r) for r in ((res,) * 3 if np.isscalar(res) else res))
    kbits, nbw = grid_bits(res)
    key = sort_key(np.asarray(x, np.float32), dx, res=res, v=np.asarray(v, np.float32), ids=ids, clean_boundary=clean_boundary)
    live = key >= 0
    M = dict(ids=ids, key=key, live=live, res=res, kbits=kbits, nbw=nbw, n_slots=len(ids), n_sorted=int(live.sum()))
    act_blk = np.unique(key[live] >> 6)
    na = len(act_blk)
    assert na == 0 or act_blk[-1] < 32 * nbw
    word = np.zeros(nbw, np.int64)
    np.bitwise_or.at(word, act_blk >> 5, 1 << (act_blk & 31))
    pop = np.bincount(act_blk >> 5, minlength=nbw)
    M.update(act_blk=act_blk, n_active=na, bits=word, wprefix=np.cumsum(pop) - pop)
    cidx = np.full(len(ids), -1, np.int64)
    cidx[live] = np.searchsorted(act_blk, key[live] >> 6) * BC + (key[live] & 63)
    counts = np.bincount(cidx[live], minlength=BC * na)
    cell_start = np.concatenate([[0], np.cumsum(counts)])
    M.update(cidx=cidx, counts=counts, cell_start=cell_start, act_start=cell_start[::BC])
    # the index in the deterministic mode: cell by cell, ascending creation id inside a cell
    slots = np.nonzero(live)[0]
    M["perm_det"] = slots[np.lexsort((ids[slots], cidx[slots]))]
    # neighbour rows
    bx, by, bz = demorton3(act_blk)
    nbr = np.full((na, 29), INVALID, np.int64)
    amask = np.zeros(na, np.int64)
    for n in range(27):
        sx, sy, sz = bx + n // 9 - 1, by + (n // 3) % 3 - 1, bz + n % 3 - 1
        ok = (sx >= 0) & (sy >= 0) & (sz >= 0)
        bk = morton3(np.where(ok, sx, 0), np.where(ok, sy, 0), np.where(ok, sz, 0))
        ok &= bk < 32 * nbw
        at = np.minimum(np.searchsorted(act_blk, bk), max(na - 1, 0))
        ok &= act_blk[at] == bk if na else ok
        nbr[ok, n] = at[ok]
        amask |= ok.astype(np.int64) << n
    own = np.zeros(na, np.int64)
    for o in range(8):
        own |= ((amask & lower_sources(o)) == 0).astype(np.int64) << o
    if na:
        nbr[:, 27], nbr[:, 28] = act_blk, own
    a, o = np.nonzero((own[:, None] >> np.arange(8)) & 1)
    M.update(nbr=nbr, own_mask=own, own_list=8 * a + o, n_own=len(a))
    # (every active block holds a particle: the ranges [act_start[a], act_start[a + 1]) are not empty)
    M["chunk_blk"] = np.searchsorted(M["act_start"], 256 * np.arange((M["n_sorted"] + 255) // 256), side="right") - 1
    return M


def _same(name, got, want):
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = np.nonzero(got != want)
    assert len(bad[0]) == 0, "%s: %d entries differ, the first at %s: device %d, model %d" % (
        name, len(bad[0]), tuple(int(b[0]) for b in bad), got[tuple(b[0] for b in bad)], want[tuple(b[0] for b in bad)])


def assert_tables(view, M, deterministic):
    """view: {name: value} of INFO and ARRAYS as the device left them; M: model() of the same slots.  Every table over its live range,
    exactly; perm as a permutation of the live slots whose cell segments hold the cells' slots (in ascending id when deterministic)."""
    na = M["n_active"]
    assert view["error"] == 0, view["error"]
    assert na <= view["max_blocks"]
    for f in ("n_slots", "n_sorted", "n_active", "nbw", "kbits"):
        assert view[f] == M[f], (f, view[f], M[f])
    _same("slot_id", view["slot_id"], np.where(M["live"], M["ids"], -1))
    for f in ("bits", "wprefix", "act_blk", "act_start", "cell_start", "chunk_blk"):
        _same(f, view[f], M[f])
    perm = np.asarray(view["perm"], np.int64)
    assert perm.shape == (M["n_sorted"],)
    assert np.all((perm >= 0) & (perm < M["n_slots"])), "perm: an entry outside the slots"
    _same("perm as a set (a permutation of the live slots)", np.sort(perm), np.nonzero(M["live"])[0])
    _same("cell of every entry of perm", M["cidx"][perm], np.repeat(np.arange(BC * na), M["counts"]))
    if deterministic:
        _same("perm (ascending id inside every cell)", perm, M["perm_det"])
    if view["list_valid"]:
        assert view["n_own"] == M["n_own"], (view["n_own"], M["n_own"])
        _same("nbr", np.asarray(view["nbr"]).reshape(na, 32)[:, :29], M["nbr"])
        _same("own_list", view["own_list"], M["own_list"])


# ---------------------------------------------------------------------------------------------------------------------------------
# a second, deliberately dumb derivation of the same tables (tests/test_sort_model_cpu.py holds the model against it): Python loops,
# np.lexsort for the index, dictionaries for the blocks
def brute_view(ids, x, v, res, dx, clean_boundary, max_blocks=1 << 30, list_valid=True):
    ids = np.asarray(ids, np.int64)
    res = tuple(int(r) for r in ((res,) * 3 if np.isscalar(res) else res))
    kbits, nbw = grid_bits(res)
    key = sort_key(np.asarray(x, np.float32), dx, res=res, v=np.asarray(v, np.float32), ids=ids, clean_boundary=clean_boundary)
    live = [i for i in range(len(ids)) if key[i] >= 0]
    order = np.lexsort((ids[live], key[live])) if live else []
    perm = [live[j] for j in order]
    blocks = sorted({int(key[i]) >> 6 for i in live})
    slot = {b: a for a, b in enumerate(blocks)}
    bits, wprefix = [0] * nbw, [0] * nbw
    for b in blocks:
        bits[b >> 5] |= 1 << (b & 31)
    for w in range(1, nbw):
        wprefix[w] = wprefix[w - 1] + bin(bits[w - 1]).count("1")
    cell_start, act_start, chunk_blk = [0] * (BC * len(blocks) + 1), [0] * (len(blocks) + 1), [0] * ((len(perm) + 255) // 256)
    pos = 0
    for c in range(BC * len(blocks)):
        cell_start[c] = pos
        while pos < len(perm) and slot[int(key[perm[pos]]) >> 6] * BC + (int(key[perm[pos]]) & 63) == c:
            if pos % 256 == 0:
                chunk_blk[pos // 256] = c // BC
            pos += 1
    cell_start[-1] = pos
    act_start = cell_start[::BC]
    coords = {}
    for b in blocks:
        bx, by, bz = (int(t[0]) for t in demorton3(np.asarray([b], np.int64)))
        coords[(bx, by, bz)] = slot[b]
    nbr, own_list = [], []
    for b in blocks:
        bx, by, bz = (int(t[0]) for t in demorton3(np.asarray([b], np.int64)))
        row = [coords.get((bx + n // 9 - 1, by + (n // 3) % 3 - 1, bz + n % 3 - 1), INVALID) for n in range(27)]
        mask = 0
        for o in range(8):  # the grid block b + o belongs to the active source block (b + o) - q with the smallest q
            c = (bx + (o >> 2), by + ((o >> 1) & 1), bz + (o & 1))
            owner = min(q for q in range(8) if (c[0] - (q >> 2), c[1] - ((q >> 1) & 1), c[2] - (q & 1)) in coords)
            if owner == o:
                mask |= 1 << o
                own_list.append(8 * slot[b] + o)
        nbr.append(row + [b, mask, 0, 0, 0])
    view = dict(n_slots=len(ids), n_sorted=len(perm), n_active=len(blocks), n_dead=len(ids) - len(perm), error=0, rank_mode=0,
                n_own=len(own_list), keyed=1, list=1, ct=16, cell_order=1, ids_cached=1, list_valid=int(list_valid), nbw=nbw,
                max_blocks=max_blocks, kbits=kbits)
    live_set = set(live)
    view.update(slot_id=np.asarray([ids[i] if i in live_set else -1 for i in range(len(ids))], np.int64),
                bits=np.asarray(bits, np.int64), wprefix=np.asarray(wprefix, np.int64), act_blk=np.asarray(blocks, np.int64),
                act_start=np.asarray(act_start, np.int64), cell_start=np.asarray(cell_start, np.int64), perm=np.asarray(perm, np.int64),
                nbr=np.asarray(nbr, np.int64).reshape(-1), own_list=np.asarray(own_list, np.int64), chunk_blk=np.asarray(chunk_blk, np.int64))
    return view
