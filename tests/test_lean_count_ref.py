"""What the lean count rests on ("the lean count"), pinned on the CPU with the per-round model tests/bcr_rounds_ref.py:
in a round in which every interval is empty and every string is a group of its own, the record k_sym writes for a string tile -- the tile's
symbol histogram, its first and last group head and the symbol counts in front of them -- is a function of the tile's bytes of A alone:

    hist = the count per symbol, fh = 0, lh = nval - 1, fhpre = 0, lhpre = hist - [the last string's symbol]

`sym_record` below is k_sym's rule in its general form (a string is a head when its position differs from its predecessor's, the first string
of a bucket always is; csrc/rb2_kernels.h); `count_record` is what k_count_lean computes, from the symbols only -- the bit-plane popcounts
included.  The model runs in input order, where every string is a group of its own in every round.
"""
import numpy as np
import pytest

import helpers as H
import bcr_rounds_ref as M


def sym_record(l, a, first_of_bucket):
    """k_sym: positions l and symbols a of one tile's strings (l_prev = the string in front of the tile, None at the start of a bucket)"""
    l_prev, l = first_of_bucket, np.asarray(l, np.int64)
    prev = np.concatenate([[-1 if l_prev is None else l_prev], l[:-1]])
    head = l != prev
    if l_prev is None:
        head[0] = True
    hist = np.bincount(a, minlength=6)[:6]
    hs = np.flatnonzero(head)
    if len(hs) == 0:
        return hist, np.zeros(6, np.int64), np.zeros(6, np.int64), -1, -1
    fh, lh = int(hs[0]), int(hs[-1])
    return hist, np.bincount(a[:fh], minlength=6)[:6], np.bincount(a[:lh], minlength=6)[:6], fh, lh


def count_record(a):
    """k_count_lean: the same record from the symbols alone, by the five popcounts the kernel takes"""
    a = np.asarray(a, np.int64) & 7
    p0, p1, p2 = int((a & 1).sum()), int((a >> 1 & 1).sum()), int((a >> 2 & 1).sum())
    p01, p02 = int(((a & 3) == 3).sum()), int(((a & 5) == 5).sum())
    c = np.zeros(6, np.int64)
    c[3], c[5], c[1], c[2], c[4] = p01, p02, p0 - p01 - p02, p1 - p01, p2 - p02
    c[0] = len(a) - c[1:].sum()
    lhpre = c.copy()
    lhpre[a[-1]] -= 1
    return c, np.zeros(6, np.int64), lhpre, 0, len(a) - 1


def same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


@pytest.mark.parametrize("tile", [64, 512])
def test_record_of_an_all_single_tile_is_a_function_of_its_symbols(tile):
    reads = [r for r in H.splitmix_bases(1500, 24, seed=9)] + [np.array([5, 1, 5, 5, 2], np.uint8)] * 3   # (N, and strings that end early: sentinels in later rounds)
    model, tiles = M.RoundsModel(), 0
    for rd in model.rounds(H.encode_batch(reads)):
        f = np.flatnonzero(rd.isnew)                               # the round's strings in array order: bucket by bucket
        piece = np.searchsorted(rd.start, f, side="right") - 1
        l, a = f - rd.start[piece], model.bwt[f]
        for b in np.unique(piece):
            lb, ab = l[piece == b], a[piece == b]
            assert (np.diff(lb) > 0).all()                         # every string a group of its own
            for t0 in range(0, len(lb), tile):
                got = count_record(ab[t0:t0 + tile])
                want = sym_record(lb[t0:t0 + tile], ab[t0:t0 + tile], None if t0 == 0 else lb[t0 - 1])
                assert same(got, want), (rd.r, b, t0)
                tiles += 1
    assert tiles > 100


def test_a_group_of_two_is_not():
    """... and only of such a tile: with two strings in one group the record depends on the positions (what the audit rounds are for)"""
    a = np.array([1, 2, 2, 3, 1], np.uint8)
    assert same(count_record(a), sym_record([3, 5, 8, 9, 12], a, None))
    assert not same(count_record(a), sym_record([3, 5, 8, 9, 9], a, None))
    assert not same(count_record(a), sym_record([3, 3, 8, 9, 12], a, 3))
