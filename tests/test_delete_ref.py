"""The identity string deletion rests on, on the CPU: the oracle's BWT with the rows of the deleted strings' walks
removed (tests/delete_ref.py) equals, byte for byte, the oracle's BWT of the survivors inserted again in id order -- in all three
sorting orders, with one strand and with both, for survivors that come back in one batch and in two."""
import functools

import numpy as np
import pytest

import delete_ref as D
import helpers as H


def reads():
    """repetitive reads (duplicates, Ns, some empty) and two empty strings, in the three batches they are inserted in"""
    rep = H.repetitive_reads(300)
    empty = np.zeros(0, np.uint8)
    return [rep[:100], rep[100:180] + [empty], rep[180:] + [empty]]


@functools.lru_cache(maxsize=None)
def built(so, both):
    o = H.Oracle(so)
    for batch in reads():
        o.insert_multi(H.encode_batch(batch, True, both))
    bwt, cnt = o.bwt(), o.counts()
    o.close()
    bwt.setflags(write=False)
    return bwt, cnt


def delete_sets(n):
    return {"none": np.zeros(0, np.int64), "one": np.array([n // 3]), "third": np.flatnonzero(np.random.RandomState(5).rand(n) < 1 / 3),
            "all": np.arange(n)}


def oracle_of(so, strings, batches):
    """the oracle's BWT and counts of these walks, inserted in this order in `batches` batches"""
    o = H.Oracle(so)
    cut = [len(strings) * k // batches for k in range(batches + 1)]
    for a, b in zip(cut, cut[1:]):
        if b > a:
            o.insert_multi(D.buffer_of(strings[a:b]))
    bwt, cnt = o.bwt(), o.counts()
    o.close()
    return bwt, cnt


@pytest.mark.parametrize("which", ["none", "one", "third", "all"])
@pytest.mark.parametrize("both", [False, True], ids=["fwd", "both"])
@pytest.mark.parametrize("so", [0, 1, 2])
def test_deleted_bwt_is_the_bwt_of_the_survivors(so, both, which):
    bwt, _ = built(so, both)
    n = D.n_strings(bwt)
    assert n == 302 * (2 if both else 1)
    ids = delete_sets(n)[which]
    got, rows = D.delete(bwt, ids)
    gone = D.walks(bwt, ids)
    assert rows == sum(len(w) + 1 for w in gone) and len(got) == len(bwt) - rows
    keep = D.survivors(bwt, ids)
    assert len(keep) == n - len(ids)
    for batches in (1, 2):
        want, _ = oracle_of(so, keep, batches)
        assert np.array_equal(got, want), "so %d, %s, %d batches: the BWT without the walked rows is not the BWT of the survivors" % (so, which, batches)


def test_walks_are_the_inserted_strings():
    """in input order id k is the k-th string inserted, and its walk is its text in the buffer's order"""
    bwt, _ = built(0, True)
    buf = np.concatenate([H.encode_batch(b, True, True) for b in reads()])
    assert np.array_equal(D.buffer_of(D.walks(bwt)), buf)


def test_duplicate_ids_and_order_do_not_matter():
    bwt, _ = built(1, True)
    a, ra = D.delete(bwt, [5, 17, 200])
    b, rb = D.delete(bwt, [200, 5, 5, 17, 200])
    assert ra == rb and np.array_equal(a, b)
    assert D.new_ids(6, [1, 4]).tolist() == [0, -1, 1, 2, -1, 3]
