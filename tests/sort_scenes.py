"""Seeded scenes for the tests of the sort's tables (tests/test_gpu_sort_tables.py on the device, tests/test_sort_model_cpu.py
without one).  A scene is a dict: res, dx, clean_boundary, x, v (fp32, in upload order = slot order while nothing reorders), env
(the knobs it needs) and `edge`, a function of the model of its slots that asserts the edge of csrc/k_sort.h the scene exists for —
whoever edits a scene so that it no longer gets there fails on the CPU."""
import numpy as np

from tests.common import lattice_cube

RANK_BATCH, WAVE_TILE, CO_CAP, BT_CHUNK_KEYS = 1024, 256, 704, 8192  # k_sort.h: slots per batch / per wave, k_cell_order_blocks' slab,
#                                                                      block keys per chunk of block_table_body (256 words of 32)


def _scene(res, dx, x, v=None, clean_boundary=True, env=None, edge=None):
    x = np.ascontiguousarray(x, np.float32)
    v = np.zeros_like(x) if v is None else np.ascontiguousarray(v, np.float32)
    res = (res,) * 3 if np.isscalar(res) else tuple(res)
    return dict(res=res, dx=dx, x=x, v=v, clean_boundary=clean_boundary, env=dict(env or {}), edge=edge or (lambda M: None))


def in_cells(cells, counts, dx, rng):
    """counts[i] particles inside cell cells[i] (their stencil base), cell by cell; 0.05 of a cell away from its faces"""
    c = np.repeat(np.asarray(cells, np.float64), counts, axis=0)
    return ((c + 0.5 + rng.uniform(0.05, 0.95, c.shape)) * dx).astype(np.float32)


def block_cells(b):
    """the 64 cells of block b = (bx, by, bz), in cell order"""
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    return g + 4 * np.asarray(b)


def _runs_of(a):
    """(start, length) of the maximal runs of equal values in a"""
    cut = np.concatenate([[0], np.nonzero(np.diff(a))[0] + 1, [len(a)]])
    return cut[:-1], np.diff(cut)


def ragged():
    res, dx = 32, 1.0 / 32
    rng = np.random.default_rng(101)
    x = lattice_cube(res, 8, 16, dx, jitter=0.2, seed=100)                       # 4096, eight per cell in adjacent slots
    x = np.concatenate([x, (rng.uniform(8.0, 24.0, (903, 3)) * dx).astype(np.float32)])  # + spray: 4999 slots
    v = rng.normal(0, 0.1, x.shape).astype(np.float32)
    v[5::97] = np.nan                                                            # single dead slots
    x[11::131, 1] = np.inf
    x[40::211] = (rng.uniform(1.0, 6.5, (len(x[40::211]), 3)) * dx).astype(np.float32)  # inside the 7-cell margin
    v[1000:1037] = np.nan                                                        # stretches of dead slots, one across a batch boundary
    x[2040:2060, 2] = -np.inf
    x[3000:3070] = np.float32(28.5 * dx)                                         # the far margin
    x[-1, 0] = np.nan                                                            # the last slot of the n % 4 tail

    def edge(M):
        n, live = M["n_slots"], M["live"]
        assert n % 4 == 3 and not live[-1] and live[-2]
        assert (n + RANK_BATCH - 1) // RANK_BATCH > 3  # MPMHIP_RANK_WGS=3: some workgroup takes a second batch
        s, l = _runs_of(live)
        dead = ~live[s]
        assert (l[dead] == 1).sum() > 20 and (l[dead] >= 20).sum() >= 3
        assert np.any(dead & (s < 2048) & (s + l > 2048))  # a dead stretch across a batch boundary
        assert 0 < M["n_sorted"] < n and M["n_active"] < 4096
    return _scene(res, dx, x, v, env={"MPMHIP_RANK_WGS": "3"}, edge=edge)


def runs(shuffled=False):
    """uploaded cell by cell: every branch of the in-cell ordering (1, 2..16, 17..64, > 64 per cell; a block of 704 / 705 entries),
    runs longer than a wave's tile and across a batch boundary"""
    res, dx = 32, 1.0 / 32
    rng = np.random.default_rng(111)
    cells, counts = [], []

    def add(cs, ns):
        cells.extend(np.asarray(cs).tolist()); counts.extend(int(n) for n in ns)
    c = block_cells((2, 3, 2))      # block C, 165 entries: every size class, the > 64 loop of the LDS path
    add(c[[0, 5, 17, 18, 40, 63]], [1, 2, 16, 17, 64, 65])
    add(block_cells((2, 2, 2)), [11] * 64)          # block A: exactly 704 entries (the last block of the LDS path)
    add(block_cells((3, 3, 2))[[21]], [300])        # block D: one cell of 300, in slots 869..1168: across slots 1023 | 1024
    add(block_cells((3, 3, 2))[[22, 23]], [3, 9])
    add(block_cells((3, 2, 2)), [11] * 63 + [12])   # block B: 705 entries (the first of the per-lane walk)
    e = block_cells((4, 4, 4))                      # block E: 741 entries with a cell of 300: the > 64 loop of the per-lane walk
    add(e, [300] + [7] * 63)
    add(block_cells((2, 2, 3)), [1] * 64)           # block G, behind A in key order: 704 + 64 = 768, so block C starts at position 3 * 256
    x = in_cells(cells, counts, dx, rng)
    if shuffled:
        x = x[np.random.default_rng(112).permutation(len(x))]

    def edge(M):
        per_block = np.diff(M["act_start"])
        assert CO_CAP in per_block and CO_CAP + 1 in per_block
        cnt = M["counts"].reshape(-1, 64)
        for n in (1, 2, 16, 17, 64, 65, 300):
            assert n in cnt
        assert np.any((cnt.max(1) > 64) & (per_block <= CO_CAP)) and np.any((cnt.max(1) > 64) & (per_block > CO_CAP))
        s, l = _runs_of(M["cidx"])
        if not shuffled:
            assert l.max() > WAVE_TILE                                              # a run longer than a wave's tile of 256 slots
            assert np.any((s <= RANK_BATCH - 1) & (s + l > RANK_BATCH))             # a run over slots 1023 and 1024
            assert len(s) == len(np.unique(M["cidx"]))                              # cell by cell
        else:
            assert l.max() < 8
        assert np.any((M["act_start"][1:-1] % 256) == 0)  # 256 k is the first position of a block, for some k > 0
        assert M["live"].all()
    return _scene(res, dx, x, edge=edge)


def hash_scene():
    """20^3 cells with two particles each, fully shuffled: about a thousand distinct cells in every batch of 1024 slots"""
    res, dx = 32, 1.0 / 32
    rng = np.random.default_rng(121)
    g = np.stack(np.meshgrid(*(np.arange(5, 25),) * 3, indexing="ij"), -1).reshape(-1, 3)
    x = in_cells(g, [2] * len(g), dx, rng)
    x = x[rng.permutation(len(x))]

    def edge(M):
        nb = M["n_slots"] // RANK_BATCH
        per_batch = [len(np.unique(M["cidx"][b * RANK_BATCH:(b + 1) * RANK_BATCH])) for b in range(nb)]
        assert nb >= 15 and min(per_batch) > 900, per_batch  # (the LDS table has 2048 entries)
        assert len(_runs_of(M["cidx"])[0]) * 3 > M["n_slots"]  # the statistics that select mode 1 at the default multiplier
        assert M["live"].all() and np.all(M["counts"][M["counts"] > 0] == 2)
    return _scene(res, dx, x, clean_boundary=False, edge=edge)


def many_blocks():
    """72^3 without the boundary margin: block coordinates up to 17 per axis, 1024 bitmap words = four chunks of the block table; blocks
    on the low faces (no neighbour at -1) and at coordinate 16 and up (Morton keys in the 2nd to 4th chunk)"""
    res, dx = 72, 1.0 / 72
    rng = np.random.default_rng(131)
    dense = lattice_cube(res, 30, 38, dx, jitter=0.2, seed=130)
    spray = rng.uniform(0.6, 71.4, (3000, 3))
    spray[:150, 0] = rng.uniform(0.6, 4.4, 150)      # cells 0..3 of x, y and z
    spray[150:300, 1] = rng.uniform(0.6, 4.4, 150)
    spray[300:450, 2] = rng.uniform(0.6, 4.4, 150)
    spray[450:600, 0] = rng.uniform(64.6, 71.4, 150)  # block coordinate 16 and 17
    spray[600:750, 1] = rng.uniform(64.6, 71.4, 150)
    spray[750:800, :2] = rng.uniform(64.6, 71.4, (50, 2))
    x = np.concatenate([dense, (spray * dx).astype(np.float32)])

    def edge(M):
        assert M["nbw"] == 1024 and M["kbits"] == 5
        assert len(np.unique(M["act_blk"] // BT_CHUNK_KEYS)) >= 3 and M["act_blk"].max() // BT_CHUNK_KEYS == 3
        assert M["n_active"] > 193  # four chunks and more of the cell table at 16, 32 and 64 blocks per chunk
        nbr = M["nbr"]
        for n in (4, 10, 12):  # the neighbours at (-1, 0, 0), (0, -1, 0), (0, 0, -1)
            assert np.sum(nbr[:, n] == 0xFFFFFFFF) > 20
        from tests.sort_model import demorton3
        bx, by, bz = demorton3(M["act_blk"])
        assert (bx == 0).sum() > 20 and (by == 0).sum() > 20 and (bz == 0).sum() > 20 and bx.max() == 17 and by.max() == 17
        assert np.any(M["wprefix"][256] > 0) and M["wprefix"][256] < M["n_active"]  # the second chunk starts inside the table
        assert M["live"].all()
    return _scene(res, dx, x, clean_boundary=False, edge=edge)


def side_array_real():
    """260^3: kbits = 7, so the keyed sort's packed word keeps 32 - 27 = 5 bits of rank and a rank of 31 and up goes to the side array"""
    res, dx = 260, 1.0 / 260
    rng = np.random.default_rng(141)
    cells = [(100, 100, 100), (100, 100, 101), (130, 90, 200), (131, 90, 200), (60, 200, 77)]
    x = in_cells(cells, [30, 31, 32, 33, 40], dx, rng)
    x = np.concatenate([x, (rng.uniform(20.0, 240.0, (300, 3)) * dx).astype(np.float32)])
    x = x[rng.permutation(len(x))]

    def edge(M):
        assert M["kbits"] == 7 and 32 - (3 * M["kbits"] + 6) == 5
        for n in (30, 31, 32, 33, 40):
            assert n in M["counts"]
    return _scene(res, dx, x, edge=edge)


def big_grid():
    """516^3: beyond the keyed sort's block space: the four launches by necessity, kbits = 8, a block table of 2048 chunks"""
    res, dx = 516, 1.0 / 516
    rng = np.random.default_rng(151)
    x = np.concatenate([np.asarray(lo) + rng.uniform(0.0, 6.0, (400, 3)) for lo in ((8.0, 8.0, 8.0), (250.0, 300.0, 20.0), (500.0, 480.0, 502.0))])
    x = (x * dx).astype(np.float32)

    def edge(M):
        assert M["kbits"] == 8 and (M["nbw"] + 255) // 256 == 2048
        assert len(np.unique(M["act_blk"] // BT_CHUNK_KEYS)) >= 3 and M["live"].all()
    return _scene(res, dx, x, edge=edge)


def non_cubic(clean_boundary=True):
    """res = (40, 24, 52): a cloud larger than the two short axes; what is deleted follows the axis"""
    res, dx = (40, 24, 52), 1.0 / 40
    rng = np.random.default_rng(161)
    x = (rng.uniform(-2.0, 54.0, (6000, 3)) * dx).astype(np.float32)

    def edge(M):
        X = x / np.float32(dx)
        lo, hi = (7.5, (32.5, 16.5, 44.5)) if clean_boundary else (0.6, (38.4, 22.4, 50.4))
        for k in range(3):
            others = [j for j in range(3) if j != k]
            inside = np.all([(X[:, j] > lo) & (X[:, j] < hi[j]) for j in others], 0)
            assert np.any(inside & (X[:, k] > hi[k] + 1.1) & ~M["live"]) and np.any(inside & (X[:, k] < hi[k]) & (X[:, k] > hi[k] - 2) & M["live"])
        assert np.any(M["live"] & (X[:, 2] > 40)) and not np.any(M["live"] & (X[:, 1] > 24))
    return _scene(res, dx, x, clean_boundary=clean_boundary, edge=edge)


def degenerate(kind):
    res, dx = 32, 1.0 / 32
    x = {"empty": np.zeros((0, 3)), "one": np.full((1, 3), 12.3 * dx), "all_dead": np.full((37, 3), 3.0 * dx)}[kind]

    def edge(M):
        assert M["n_sorted"] == (1 if kind == "one" else 0) and M["n_slots"] == len(x)
    return _scene(res, dx, x, edge=edge)


SCENES = {
    "ragged": ragged, "runs": runs, "runs_shuffled": lambda: runs(True), "hash": hash_scene, "many_blocks": many_blocks,
    "side_array_real": side_array_real, "big_grid": big_grid, "non_cubic": non_cubic, "non_cubic_no_margin": lambda: non_cubic(False),
    "empty": lambda: degenerate("empty"), "one": lambda: degenerate("one"), "all_dead": lambda: degenerate("all_dead"),
}
PRODUCT_SCENES = ("ragged", "runs", "runs_shuffled", "hash", "many_blocks")  # the ones every form of the sort is run on


def model_of(scene, ids=None, x=None, v=None):
    from tests.sort_model import model
    x = scene["x"] if x is None else x
    return model(np.arange(len(x)) if ids is None else ids, x, scene["v"] if v is None else v, scene["res"], scene["dx"],
                 scene["clean_boundary"])
