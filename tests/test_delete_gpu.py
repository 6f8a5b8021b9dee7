"""GPU tests of string deletion (rb2_hip_delete_strings, HipBwt.delete: csrc/rb2_delete.h).

The expected BWT always comes from the oracle built from the survivors -- the strings the numpy model (tests/delete_ref.py) walks out of the
oracle's BWT of everything, minus the deleted ids, in id order -- never from the library; the return value is the model's row count."""
import os
import subprocess
import sys

import numpy as np
import pytest

import delete_ref as D
import fmd_ref
import helpers as H
import locate_ref as LR
import query_ref as Q
from test_query_gpu import _Env
from test_query_layouts_gpu import FORCED, S_FIRST, S_REST, _n_reads

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def oracle_of(so, bufs):
    o = H.Oracle(so)
    for b in bufs:
        if len(b):
            o.insert_multi(b)
    bwt, cnt = o.bwt(), o.counts()
    o.close()
    return bwt, cnt


def expect(so, bwt, ids, more=()):
    """(oracle BWT, oracle counts, rows removed, survivors) of deleting ids from the index whose BWT is bwt, then inserting the buffers more"""
    keep = D.survivors(bwt, ids)
    want, cnt = oracle_of(so, [D.buffer_of(keep)] + list(more))
    return want, cnt, D.delete(bwt, ids)[1], keep


def check(g, want, cnt):
    assert np.array_equal(g.counts(), cnt)
    got = g.bwt()
    assert len(got) == len(want) and np.array_equal(got, want), "first differing row: %s" % np.flatnonzero(got[:len(want)] != want[:len(got)])[:1]


# ---- 1. small, all six ropes --------------------------------------------------------------------------------------------------

def small_reads():
    rep = H.repetitive_reads(300)
    empty = np.zeros(0, np.uint8)
    return [rep[:100], rep[100:180] + [empty], rep[180:] + [empty]]


_small = {}


def small_model(so):
    if so not in _small:
        bufs = [H.encode_batch(b, True, True) for b in small_reads()]
        bwt, cnt = oracle_of(so, bufs)
        _small[so] = (bufs, bwt, cnt, [len(w) for w in D.walks(bwt)])
    return _small[so]


def small_index(hip, so):
    bufs, bwt, cnt, _ = small_model(so)
    g = hip.HipBwt(so)
    for b in bufs:
        g.insert_multi(b)
    check(g, bwt, cnt)
    return g, bwt


def small_ids(so, which):
    _, bwt, _, lens = small_model(so)
    n = len(lens)
    assert n == 604 and (bwt == 5).any()
    if which == "one":
        return np.array([n // 3])
    if which == "empty":                                            # two strings of no symbols: a walk of one row each
        e = np.flatnonzero(np.array(lens) == 0)
        return np.array([2 * 180 + 1, n - 1]) if so == 0 else e[-2:]   # (input order: the two this fixture added, by their places)
    if which == "dups":
        return np.array([40, 7, 40, 301, 7, 7, 590, 301])
    if which == "alternate":
        return np.arange(0, n, 2)
    return np.arange(n)


@pytest.mark.parametrize("which", ["one", "empty", "dups", "alternate", "all"])
@pytest.mark.parametrize("so", [0, 1, 2])
def test_small_all_ropes(hip, so, which):
    g, bwt = small_index(hip, so)
    ids = small_ids(so, which)
    if which == "empty":
        assert all(small_model(so)[3][i] == 0 for i in ids)
    want, cnt, rows, keep = expect(so, bwt, ids)
    g.build_ssa(3)
    assert g.delete(ids) == rows
    assert not g.ssa_info()["valid"] and not g.layout_stats()["sparse_now"]
    assert g.delete_stats()["rows_removed"] == rows
    check(g, want, cnt)
    if which == "all":
        assert rows == len(bwt) and not g.counts().any() and len(g.bwt()) == 0
        fresh = H.encode_batch(H.repetitive_reads(120, seed=3), True, True)
        g.insert_multi(fresh)
        check(g, *oracle_of(so, [fresh]))
    elif so == 0:                                                   # the ids of the survivors closed ranks
        got = g.extract(np.arange(len(keep)), 64)
        assert all(np.array_equal(a, w[::-1]) for a, w in zip(got, keep))
    g.close()


@pytest.mark.parametrize("so", [0, 1, 2])
def test_deleting_nothing_changes_nothing(hip, so):
    g, bwt = small_index(hip, so)
    g.build_ssa(3)
    before = (g.rope_hashes(), g.layout_stats(), g.ssa_info())
    hits = g.locate([(0, 50)], 64)[0]
    assert g.delete([]) == 0 and g.delete(np.zeros(0, np.int32)) == 0
    assert (g.rope_hashes(), g.layout_stats(), g.ssa_info()) == before and before[2]["valid"]
    assert np.array_equal(g.locate([(0, 50)], 64)[0], hits)
    check(g, bwt, small_model(so)[2])
    g.close()


# ---- 2. pieces across superblocks; 6. afterwards the index is a normal index ---------------------------------------------------

class _Big:
    pass


@pytest.fixture(scope="module", params=[0, 2])
def big(request, hip):
    """the dense shape of tests/test_query_layouts_gpu.py, a quarter of its strings and the ids [1000, 3200) deleted"""
    so = request.param
    codes = H.splitmix_bases(9000, 100, seed=77)
    bufs = [H.encode_batch_fixed(codes[:4500], True, True), H.encode_batch_fixed(codes[4500:], True, True)]
    B = _Big()
    B.so = so
    B.bwt0, B.cnt0 = oracle_of(so, bufs)
    assert len(B.bwt0) == 1818000
    n = D.n_strings(B.bwt0)
    B.ids = np.union1d(np.flatnonzero(np.random.RandomState(1).rand(n) < 0.25), np.arange(1000, 3200))
    B.gone = D.gone_rows(B.bwt0, B.ids)
    B.want, B.cnt, B.rows, B.keep = expect(so, B.bwt0, B.ids)
    g = hip.HipBwt(so)
    for b in bufs:
        g.insert_multi(b)
    check(g, B.bwt0, B.cnt0)
    g.build_ssa(5)
    B.ret = g.delete(B.ids)
    B.ssa_after, B.stats, B.layout = g.ssa_info(), g.delete_stats(), g.layout_stats()
    B.got, B.got_cnt = g.bwt(), g.counts()
    B.g = g
    yield B
    g.close()


def test_pieces_across_superblocks(big, hip):
    B = big
    leaf = hip.HipBwt.layout()["leaf_syms"]
    # what the delete set does to the source, from the model: emptied groups and leaves, and pieces that stay longer than two superblocks
    assert leaf == 1024 and B.cnt[1:5, 1:5].min() > 2 * 32 * leaf, B.cnt
    n = D.n_strings(B.bwt0)
    dollar = B.gone[:n]                                             # rope $ is one piece: its groups and leaves count from row 0
    assert dollar[:n // 64 * 64].reshape(-1, 64).all(1).sum() >= 34
    assert dollar[:n // leaf * leaf].reshape(-1, leaf).all(1).sum() >= 2
    assert B.ret == B.rows == int(B.gone.sum())
    assert np.array_equal(B.got_cnt, B.cnt)
    assert len(B.got) == len(B.want) and np.array_equal(B.got, B.want)
    st = B.stats
    assert st["rows_removed"] == B.rows and 0 < st["groups_compressed"] <= st["groups"] and st["leaves_written"] < st["leaves_read"]
    assert not B.layout["sparse_now"]


def test_afterwards_a_normal_index(big, hip):
    B, g, so = big, big.g, big.so
    assert B.ssa_after["valid"] is False and B.ssa_after["samples"] == 0
    fm = Q.FM(B.want)
    rng = np.random.RandomState(11)
    pats = []
    for _ in range(500):
        s = B.keep[rng.randint(len(B.keep))][::-1]
        a = rng.randint(len(s))
        pats.append(s[a:a + rng.randint(1, 60)].copy())
    want = np.array([fm.count(p) for p in pats])
    assert (want > 0).all() and np.array_equal(g.count(pats), want)
    g.build_ssa(4)
    iv = []
    for p in pats[:200]:
        lo, hi, _ = fm.backward_search(p)
        iv.append((lo, hi))
    stored, hit, cnt = g.locate_raw(iv, 8)
    w_stored, w_hit, w_cnt = LR.locate_raw(fm, iv, 8)
    assert stored == w_stored and np.array_equal(cnt, w_cnt) and np.array_equal(hit, w_hit)
    # a second deletion, then a dense insert
    ids2 = np.random.RandomState(12).choice(D.n_strings(B.want), 100, replace=False)
    want2, cnt2, rows2, keep2 = expect(so, B.want, ids2)
    assert g.delete(ids2) == rows2 and not g.ssa_info()["valid"]
    check(g, want2, cnt2)
    more = H.encode_batch_fixed(H.splitmix_bases(1000, 100, seed=78), True, True)
    g.insert_multi(more)
    check(g, *oracle_of(so, [D.buffer_of(keep2), more]))
    assert not g.layout_stats()["sparse_now"]


# ---- 3. long runs ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_del", [6, 4])
def test_long_runs(hip, n_del):
    reads = [np.full(5000, 1, np.uint8)] * 6 + list(H.splitmix_bases(200, 100, seed=9))
    order = np.random.RandomState(2).permutation(len(reads))
    buf = H.encode_batch([reads[i] for i in order], True, False)
    bwt, cnt = oracle_of(1, [buf])
    lens = np.array([len(w) for w in D.walks(bwt)])
    ids = np.flatnonzero(lens == 5000)[:n_del]
    assert len(ids) == n_del and cnt[1, 1] > 29000                   # piece (A,A): some 30 000 consecutive rows
    gone = D.gone_rows(bwt, ids)
    if n_del == 6:                                                  # whole leaves of consecutive rows go
        edges = np.flatnonzero(np.diff(np.concatenate([[0], gone.astype(np.int8), [0]])))   # starts and ends of the runs of removed rows
        assert (edges[1::2] - edges[0::2]).max() > 20 * 1024
    want, wcnt, rows, _ = expect(1, bwt, ids)
    g = hip.HipBwt(1)
    g.insert_multi(buf)
    check(g, bwt, cnt)
    assert g.delete(ids) == rows == n_del * 5001
    check(g, want, wcnt)
    g.close()


# ---- 4. sparse source -----------------------------------------------------------------------------------------------------------

def test_sparse_source(hip):
    rng = np.random.RandomState(3)
    rest = list(H.splitmix_bases(*S_REST, seed=5))
    half = len(rest) // 2
    parts = [list(H.splitmix_bases(*S_FIRST, seed=4)), rest[:half] + _n_reads(rng, 4, 900, 1500), rest[half:] + _n_reads(rng, 4, 900, 1500)]
    bufs = [H.encode_batch(p, True, True) for p in parts]
    bwt, cnt = oracle_of(1, bufs)
    with _Env(**FORCED):
        g = hip.HipBwt(1)
    for b in bufs:
        g.insert_multi(b)
    assert g.layout_stats()["sparse_now"]
    assert np.array_equal(g.counts(), cnt)
    n = D.n_strings(bwt)
    ids = np.flatnonzero(np.random.RandomState(4).rand(n) < 1 / 3)
    more = H.encode_batch(H.repetitive_reads(150, seed=12, max_len=40), True, True)
    want, wcnt, rows, keep = expect(1, bwt, ids)
    assert g.delete(ids) == rows
    assert g.layout_stats()["sparse_now"] is False
    check(g, want, wcnt)
    g.insert_multi(more)
    check(g, *oracle_of(1, [D.buffer_of(keep), more]))
    g.close()


# ---- 5. loaded source -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rand300", "kat6"])
def test_loaded_source(hip, name):
    img, bwt = fmd_ref.fixture(name)
    g = hip.HipBwt(0)
    assert g.load_fmd(np.frombuffer(img, np.uint8)) == len(bwt)
    n = D.n_strings(bwt)
    ids = np.flatnonzero(np.random.RandomState(6).rand(n) < 1 / 3)
    assert len(ids) > 0
    want, rows = D.delete(bwt, ids)                                 # (the model on the fixture's decoded BWT: the file records no order to rebuild in)
    assert g.delete(ids) == rows
    got = g.bwt()
    assert len(got) == len(want) and np.array_equal(got, want)
    assert g.counts().sum() == len(want) and g.counts()[:, 0].sum() == n - len(ids)
    g.close()


# ---- 7. fatal conditions --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,msg", [("negative_id", "ids[1] = -1 is no string of the index"), ("id_is_count", "ids[0] = 40 is no string of the index (it holds 40)"),
                                      ("negative_n", "the number of ids must not be negative (got -1)")])
def test_fatal_conditions(hip, case, msg):
    p = subprocess.run([sys.executable, os.path.join(HERE, "delete_fatal_child.py"), case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    out, err = p.stdout.decode(), p.stderr.decode()[-2000:]
    assert p.returncode == 7, (p.returncode, out, err)
    assert "handler: [rb2_hip] delete_strings: " in out and msg in out, out
    assert "unchanged ok" in out and "in-range ok" in out, (out, err)
