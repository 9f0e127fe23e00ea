"""Numpy model of the ranking behind the frame of a tiled job (csrc/k_frame.h) — test infrastructure.

Every rank holds some creation ids.  top = 1 + the largest; every rank sets bit `id` of a bitmap of ceil(top / 32) words; prefix[w] =
the set bits of the words before w; the row of an id in the job's file is prefix[id >> 5] + popcount(bits[id >> 5] & lower bits)."""
import numpy as np


def live_id_top(ids):
    ids = np.asarray(ids, np.int64)
    ids = ids[ids >= 0]
    return int(ids.max()) + 1 if ids.size else 0


def bitmap(ids, top):
    """(words uint32 [ceil(top / 32)], live) of one rank — dead slots (id < 0) are skipped"""
    ids = np.asarray(ids, np.int64)
    ids = ids[ids >= 0]
    words = np.zeros((top + 31) // 32, np.uint32)
    np.bitwise_or.at(words, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return words, int(ids.size)


def popcount(words):
    return np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8)).reshape(-1, 32).sum(1).astype(np.uint32) \
        if len(words) else np.zeros(0, np.uint32)


def prefix(words):
    """exclusive prefix of the words' popcounts"""
    c = popcount(words).astype(np.int64)
    return (np.cumsum(c) - c).astype(np.uint32)


def row_numbers(ids, words, pre):
    """row number of every id (all must be set in `words`)"""
    ids = np.asarray(ids, np.int64)
    w = words[ids >> 5]
    bit = np.uint32(1) << (ids & 31).astype(np.uint32)
    assert ((w & bit) != 0).all()
    below = w & (bit - np.uint32(1))
    return pre[ids >> 5] + popcount(below)


def job_rows(rank_ids):
    """[row numbers of rank r's live ids, in the order given] for the ids of every rank"""
    top = max([live_id_top(i) for i in rank_ids] + [0])
    union = np.zeros((top + 31) // 32, np.uint32)
    live = 0
    for ids in rank_ids:
        w, n = bitmap(ids, top)
        union |= w
        live += n
    assert int(popcount(union).sum()) == live, "an id is held twice"
    pre = prefix(union)
    return [row_numbers(np.asarray(i, np.int64)[np.asarray(i, np.int64) >= 0], union, pre) for i in rank_ids]
