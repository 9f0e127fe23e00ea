"""The models the deterministic asynchronous steppers are tested against on the device (tests/async_order_model.py), checked on
the host: async_block_of against hand-computed blocks at the edges of the block table, the ordered compaction against a
brute-force loop."""
import numpy as np
import pytest

from tests.async_order_model import CHUNK, INVALID, async_block_of, block_counts, ordered_slots, pooled_store


def test_block_of_a_position_at_the_edges_of_the_3d_table():
    res, dx = 32, 1.0 / 32
    assert block_counts(res, 3) == (9, 9, 5)  # 4 x 4 x 8 nodes per block, one more block than res / size per axis
    # base node = int(x / dx - 0.5); block = (base >> 2, base >> 2, base >> 3); flat = (bx * 9 + by) * 5 + bz
    cases = [
        ((0.75, 0.75, 0.75), 0),                       # base (0, 0, 0)
        ((4.25, 0.75, 0.75), 0),                       # base (3, 0, 0): still block 0
        ((4.75, 0.75, 0.75), (1 * 9 + 0) * 5 + 0),     # base (4, 0, 0): the next block along x
        ((0.75, 4.75, 0.75), (0 * 9 + 1) * 5 + 0),
        ((0.75, 0.75, 8.25), 0),                       # base z = 7: eight nodes per block along z
        ((0.75, 0.75, 8.75), 1),                       # base z = 8
        ((31.9, 31.9, 31.9), (7 * 9 + 7) * 5 + 3),     # base 31 -> (7, 7, 3)
        ((32.6, 32.6, 32.6), (8 * 9 + 8) * 5 + 4),     # base 32 -> the table's last block (8, 8, 4)
        ((36.6, 0.75, 0.75), INVALID),                 # base 36 -> bx = 9 = nb[0]: outside
        ((0.75, 0.75, 40.6), INVALID),                 # base z = 40 -> bz = 5 = nb[2]: outside
        ((0.3, 0.75, 0.75), INVALID),                  # below half a cell: no base node
        ((0.75, 0.49, 0.75), INVALID),
        ((0.75, 0.75, -0.2), INVALID),
        ((float("nan"), 0.75, 0.75), INVALID),         # !(X >= 0.5)
    ]
    x = np.array([c[0] for c in cases], np.float64) * dx
    want = np.array([c[1] for c in cases], np.int64)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(async_block_of(x.astype(np.float32), res, 3), want)


def test_block_of_a_position_at_the_edges_of_the_2d_table():
    res, dx = 64, 1.0 / 64
    assert block_counts(res, 2) == (9, 5)  # 8 x 16 nodes per block
    cases = [
        ((0.75, 0.75), 0),
        ((8.25, 0.75), 0),                 # base x = 7
        ((8.75, 0.75), 1 * 5 + 0),         # base x = 8
        ((0.75, 16.25), 0),                # base y = 15
        ((0.75, 16.75), 1),                # base y = 16
        ((63.9, 63.9), 7 * 5 + 3),         # base 63 -> (7, 3)
        ((64.6, 64.6), 8 * 5 + 4),         # base 64 -> the last block
        ((72.6, 0.75), INVALID),           # base 72 -> bx = 9: outside
        ((0.75, 80.6), INVALID),           # base 80 -> by = 5: outside
        ((0.3, 10.0), INVALID),
        ((10.0, 0.45), INVALID),
    ]
    x = np.array([c[0] for c in cases], np.float64) * dx
    want = np.array([c[1] for c in cases], np.int64)
    assert np.array_equal(async_block_of(x.astype(np.float32), res, 2), want)
    # another grid: 128 -> 17 x 9 blocks
    assert block_counts(128, 2) == (17, 9)
    assert async_block_of(np.array([[100.7, 50.7]], np.float32) / 128, 128, 2)[0] == (100 >> 3) * 9 + (50 >> 4)


@pytest.mark.parametrize("n", [0, 1, 1000, CHUNK, CHUNK + 1, 3 * CHUNK, 3524, 10 * CHUNK + 7])
@pytest.mark.parametrize("wgs", [1, 3, 4096])
def test_the_ordered_compaction_model_equals_a_brute_force_loop(n, wgs):
    rng = np.random.default_rng(n + wgs)
    for density, base in ((0.0, 0), (1.0, 5), (0.5, 0), (0.9, 2049)):
        flags = rng.uniform(size=n) < density
        slots, end = ordered_slots(flags, wgs, base)
        want, o = np.full(n, -1, np.int64), base
        for i in range(n):
            if flags[i]:
                want[i] = o
                o += 1
        assert np.array_equal(slots, want) and end == o


def test_the_pooled_store_model_lists_the_kept_particles_in_upload_order():
    rng = np.random.default_rng(7)
    res = 32
    batches = []
    for n in (1000, 1024, 1500):
        x = rng.uniform(2.0 / res, 1 - 2.0 / res, (n, 3)).astype(np.float32)
        x[rng.choice(n, 5, replace=False), rng.integers(0, 3, 5)] = 0.3 / res
        batches.append(x)
    ids, blks = pooled_store(batches, res, 3, wgs=3)
    allx = np.concatenate(batches)
    b = async_block_of(allx, res, 3)
    want_ids = [i for i in range(len(allx)) if b[i] != INVALID]  # brute force: every kept particle, in upload order
    assert len(want_ids) == len(allx) - 15
    assert ids.tolist() == want_ids and np.array_equal(blks, b[want_ids])
