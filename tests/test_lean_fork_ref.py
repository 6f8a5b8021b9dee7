"""What the forked round ("the forked round") rests on, from the per-round model tests/bcr_rounds_ref.py alone, without a GPU:
the layout of the new side needs no symbol counts.  A string of bucket r inserts into piece r, so

  * a piece's size after the round = its size before + the size of its bucket, and
  * the leaf, superblock and window offsets k_part<.., FORK> derives from those sizes alone are the ones the round's windows really have.

The buckets of a round are what setup_body laid out the round before, from that round's count matrix (bucket (a, b) = the strings that sat
in a piece of rope b and inserted a; round 0: every string in the bucket of rope `$`).  The test computes them that way, from the symbols the
model's rounds really inserted, and never asks the model which piece a string is in.

The model inserts in input order.  The RLO and RCLO cases feed it every batch sorted in that order: the rows of a first batch are then the
engine's own (checked against the oracle), and a second batch is another valid insertion with other buckets -- the identity does not depend
on the order, only on "bucket r inserts into piece r".

A wrong rule must fail: sizes taken from the count matrix's column of the SAME round (the next round's buckets) do not give the round's pieces.
"""
import numpy as np
import pytest

import bcr_rounds_ref as R
import helpers as H

LEAF, SB, WPL = 1024, 32, 4                      # symbols per leaf, leaves per superblock, leaves per window (csrc/rb2_device.h)
assert WPL * LEAF == R.WIN


def rope_sym(r):
    return 0 if r == 0 else 1 + (r - 1) // 6


def sorted_batch(reads, so):
    """the batch buffer (reversed, 0-terminated strings) of the reads in the order the sorted modes insert them: by the reversed string (RLO), by
    its complement (RCLO); `$` sorts first; stable"""
    if so == 0:
        return H.encode_batch(reads)
    def key(r):
        s = np.asarray(r, np.uint8)[::-1]
        if so == 2:
            s = np.where((s >= 1) & (s <= 4), 5 - s, s)
        return bytes(s.tolist())
    return H.encode_batch([reads[i] for i in sorted(range(len(reads)), key=lambda i: key(reads[i]))])


def layout_from_sizes(n):
    """the arithmetic of k_part<.., FORK>'s first wave (and of setup_body's dense branch): lane = piece, two exclusive scans"""
    n = np.asarray(n, np.int64)
    nleaves = (n + LEAF - 1) // LEAF
    padded = (nleaves + SB - 1) // SB * SB
    nwin = (nleaves + WPL - 1) // WPL
    leaf0 = np.cumsum(padded) - padded
    wf0 = np.concatenate([np.cumsum(nwin) - nwin, [nwin.sum()]])
    return {"nleaves": nleaves, "leaf0": leaf0, "sb0": leaf0 // SB, "wf0": wf0, "nsb_total": int(padded.sum()) // SB}


def layout_of_round(rd):
    """the same figures from what the model's round really looks like: its pieces' rows and its list of windows, piece after piece"""
    nleaves, leaf0, sb0, wf0 = [], [], [], []
    leaf = 0
    for p in range(R.NR):
        rows = int(rd.start[p + 1] - rd.start[p])
        nl = -(-rows // LEAF)
        w = np.flatnonzero(rd.piece == p)
        assert len(w) == -(-nl // WPL) and (len(w) == 0 or (rd.j[w] == np.arange(len(w))).all())
        wf0.append(None)
        nleaves.append(nl); leaf0.append(leaf); sb0.append(leaf // SB)
        leaf += -(-nl // SB) * SB
    # an empty piece has no window of its own: its first window is the next piece's (an exclusive scan says the same)
    nxt = len(rd.piece)
    for p in range(R.NR - 1, -1, -1):
        if (rd.piece == p).any():
            nxt = int(np.flatnonzero(rd.piece == p)[0])
        wf0[p] = nxt
    return {"nleaves": np.array(nleaves), "leaf0": np.array(leaf0), "sb0": np.array(sb0), "wf0": np.array(wf0 + [len(rd.piece)]), "nsb_total": leaf // SB}


def count_matrix(rd, new):
    """count[r][a] = symbols a the round inserted into piece r, from the array as it is and the flags of the new symbols"""
    c = np.zeros((R.NR, 6), np.int64)
    for p in range(R.NR):
        lo, hi = int(rd.start[p]), int(rd.start[p + 1])
        c[p] = np.bincount(new[lo:hi][rd.isnew[lo:hi]], minlength=6)
    return c


def next_buckets(count):
    """setup_body: bucket (a, b) of the next round = members of the pieces of rope b that inserted a; strings that inserted `$` are done"""
    c2 = np.zeros(R.NR, np.int64)
    for r in range(1, R.NR):
        a, b = rope_sym(r), (r - 1) % 6
        c2[r] = count[0][a] if b == 0 else sum(count[H.rope_of(b, x)][a] for x in range(6))
    return c2


def two_batch_job():
    rr = H.repetitive_reads(2600, seed=11)
    rnd = [r for r in H.splitmix_bases(2600, 23, seed=9)]
    return [rr[:1300] + rnd[:1300], rnd[1300:] + rr[1300:]]


@pytest.mark.parametrize("so", [0, 1, 2])
def test_a_piece_grows_by_its_bucket_and_the_layout_follows(so):
    m = R.RoundsModel()
    rounds = wrong_sizes = wrong_layouts = 0
    for k, reads in enumerate(two_batch_job()):
        buf = sorted_batch(reads, so)
        size = None
        bucket = np.zeros(R.NR, np.int64)
        bucket[0] = len(reads)                                      # round 0: every string in the bucket of rope `$`
        for rd in m.rounds(buf):
            if size is None:
                size = np.diff(rd.old_start)
            assert np.array_equal(size, np.diff(rd.old_start))
            after = np.diff(rd.start)
            assert np.array_equal(after, size + bucket), "round %d of batch %d: a piece grows by its bucket" % (rd.r, k)
            assert bucket.sum() == rd.isnew.sum()
            want, got = layout_of_round(rd), layout_from_sizes(size + bucket)
            for f in want:
                assert np.array_equal(want[f], got[f]), (rd.r, k, f)
            cnt = count_matrix(rd, m.bwt)
            assert np.array_equal(cnt.sum(axis=1), bucket)              # (a row of the matrix is a bucket, spread over the symbols)
            # the wrong rule: the sizes the SAME round's matrix column gives (the buckets of the next round)
            column = next_buckets(cnt)
            column[0] = bucket[0]                                       # (rope `$` has no column of its own: leave it right)
            if not np.array_equal(size + column, after):
                wrong_sizes += 1
                bad = layout_from_sizes(size + column)
                wrong_layouts += any(not np.array_equal(want[f], bad[f]) for f in want)
            size, bucket = after, next_buckets(cnt)
            rounds += 1
        if k == 0 and so:                                           # the rows of a first batch fed in sorted order are the sorted mode's own
            o = H.Oracle(so)
            o.insert_multi(H.encode_batch(reads))
            assert np.array_equal(m.bwt, o.bwt()) and np.array_equal(m.matrix(), o.counts())
            o.close()
    assert rounds > 60
    assert wrong_sizes > rounds // 2 and wrong_layouts > 0, (rounds, wrong_sizes, wrong_layouts)
