"""CPU check of what rb2_hip_merge rests on: taking the strings of an index B in the row order of its `$` block
and inserting them into an index A -- in one batch, in uneven batches or one string per batch -- gives, symbol for symbol, the BWT of
all strings built in one batch and in two, in every sorting order.  Also the (txt, off) format of the unpack model."""
import numpy as np
import pytest

import helpers as H
import merge_ref as M

CUTS = {"one": None, "uneven4": [1, 37, 5], "single": [1] * 400}


@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("seed", [3, 11])
def test_row_order_reinsertion_is_exact(so, seed):
    sa, sb = M.mixed_reads(90, seed), M.mixed_reads(70, seed + 1) + M.mixed_reads(90, seed)[:15]   # (strings of A again in B)
    ba, bb = H.encode_batch(sa), H.encode_batch(sb)
    one = M.oracle_bwt(so, [np.concatenate([ba, bb])])
    two = M.oracle_bwt(so, [ba, bb])
    assert np.array_equal(one, two)
    bwt_b = M.oracle_bwt(so, [bb])
    for name, sizes in CUTS.items():
        got, cnt = M.merge(so, [ba], bwt_b, sizes)
        assert len(M.cut(M.strings(bwt_b), sizes)) == {"one": 1, "uneven4": 4, "single": len(sb)}[name]
        assert np.array_equal(got, one), (so, seed, name)
        assert cnt.sum() == len(one)
    got, _ = M.merge(so, [], bwt_b, CUTS["uneven4"])                # an empty destination: src's strings, rebuilt
    assert np.array_equal(got, bwt_b)


@pytest.mark.parametrize("so", [0, 1, 2])
def test_unpack_model_format(so):
    reads = M.mixed_reads(60, 5)
    bwt = M.oracle_bwt(so, [H.encode_batch(reads)])
    txt, off = M.unpack(bwt)
    rtxt, roff = M.unpack(bwt, reversed=True)
    n = len(reads)
    assert len(off) == n + 1 and off[0] == 0 and off[-1] == len(txt) == sum(len(r) for r in reads) + n and np.array_equal(off, roff)
    assert (txt[off[1:] - 1] == 0).all() and (rtxt[off[1:] - 1] == 0).all() and (txt == 0).sum() == n
    got = [txt[off[i]:off[i + 1] - 1] for i in range(n)]
    for i in range(n):                                             # the pair is each other's per-string mirror
        assert np.array_equal(got[i][::-1], rtxt[off[i]:off[i + 1] - 1])
    if so == 0:                                                    # input order: the rows of the `$` block are the strings as inserted
        assert all(np.array_equal(a, b) for a, b in zip(got, reads))
        assert np.array_equal(rtxt, H.encode_batch(reads))
    else:
        assert sorted(g.tobytes() for g in got) == sorted(np.asarray(r, np.uint8).tobytes() for r in reads)
    assert np.array_equal(M.oracle_bwt(so, [rtxt]), bwt)            # the reversed text is a batch that rebuilds the index
    t2, o2 = M.unpack(bwt, 7, 20, False)
    assert np.array_equal(t2, txt[off[7]:off[27]]) and np.array_equal(o2, off[7:28] - off[7])
    t0, o0 = M.unpack(bwt, 5, 0)
    assert len(t0) == 0 and o0.tolist() == [0]
