"""GPU tests of the duplicate / containment query (include/rb2_hip.h: rb2_hip_contained[_dev], HipBwt.contained_raw / contained /
reduce; kernel k_contain in csrc/rb2_query.h): every record the device reports must equal the numpy model
(tests/contain_ref.py, itself checked against a brute force over string slices in test_contain_ref.py) on the BWT of the same index.
The shapes are the smallest that reach both layouts and every branch: the fixture *mixed* holds every flag and both ends of a walk; D and
S (test_query_layouts_gpu.py) put lo, hi and ahi deep inside pieces of several superblocks and into split sparse leaves -- their reads are
unique, so it is the run without the early exit that walks there."""
import os
import subprocess
import sys

import numpy as np
import pytest

import contain_ref as CR
import fmd_ref
import locate_ref as LR
import query_ref as Q
from ropebwt2_amd.hipbwt import encode_runs
from test_query_gpu import _Env
from test_query_layouts_gpu import _Idx, _Models, _build_dense, _build_sparse, _unchanged

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILL = -7                                                            # what the device variant finds in rec, and what must stay behind it
GUARD = 16                                                           # words behind rec that no record may touch


def dev_records(g, n, ids):
    """contained_dev on a buffer of n records and GUARD more words, all FILL: the (n, 5) records; the words behind them must be FILL still"""
    buf = np.full(5 * n + GUARD, FILL, np.int64)
    ids = None if ids is None else np.ascontiguousarray(np.asarray(ids, np.int64).reshape(-1))
    d_rec = g.dev_alloc(buf.nbytes)
    d_ids = g.dev_alloc(max(ids.nbytes, 8)) if ids is not None else None
    try:
        g.L.rb2_hip_memcpy(g.h, d_rec, buf.ctypes.data, buf.nbytes, 0)
        if ids is not None and len(ids):
            g.L.rb2_hip_memcpy(g.h, d_ids, ids.ctypes.data, ids.nbytes, 0)
        g.contained_dev(n, d_ids, d_rec)
        g.L.rb2_hip_memcpy(g.h, buf.ctypes.data, d_rec, buf.nbytes, 1)
    finally:
        g.dev_free(d_rec)
        if d_ids is not None:
            g.dev_free(d_ids)
    assert (buf[5 * n:] == FILL).all(), "a record was written behind rec"
    return buf[:5 * n].reshape(n, 5)


def mixed_index(hip, so, rev, extra=()):
    bufs, bwt = CR.mixed(so, rev, extra)
    g = hip.HipBwt(so)
    for b in bufs:
        g.insert_multi(b)
    assert np.array_equal(g.bwt(), bwt)
    return g, Q.FM(bwt)


class _Ctx:
    pass


@pytest.fixture(scope="module")
def models():
    ms = _Models()
    yield ms
    ms.made.clear()


@pytest.fixture(scope="module", params=["mixed-io", "mixed-rclo", "D", "S", "fmd"])
def idx(request, hip, models):
    """an index with a suffix array built on it, its model, and the model's records with and without the early exit (computed once)"""
    kind = request.param
    if kind.startswith("mixed"):
        g, fm = mixed_index(hip, 0 if kind == "mixed-io" else 2, True)
        ix = _Idx(kind, g, None, 1, False)
    elif kind == "D":
        ix = _build_dense(hip, models.get(0))
        g, fm = ix.g, ix.m.fm
    elif kind == "S":
        ix = _build_sparse(hip, models.get("S"))
        g, fm = ix.g, ix.m.fm
    else:
        img, bwt = fmd_ref.fixture("cov3000")
        g = hip.HipBwt(0)
        assert g.load_fmd(np.frombuffer(img, np.uint8)) == len(bwt)
        fm = Q.FM(bwt)
        ix = _Idx(kind, g, None, 1, False)
    cx = _Ctx()
    cx.kind, cx.ix, cx.g, cx.fm, cx.n = kind, ix, g, fm, int(fm.C[1])
    g.build_ssa(4)
    rng = np.random.RandomState(cx.n)
    lo = rng.randint(0, fm.N - 8, size=64)
    cx.iv = np.stack([lo, lo + rng.randint(1, 8, size=64)], 1).astype(np.int64)
    cx.places = LR.locate_raw(fm, cx.iv, 4)
    info = {}
    cx.want = {True: CR.contained(fm, info=info), False: CR.contained(fm, early=False)}
    cx.early = info["early"]
    yield cx
    g.close()


@pytest.mark.parametrize("early", [True, False])
def test_records_match_model(idx, early):
    cx, g, fm, n = idx, idx.g, idx.fm, idx.n
    want = cx.want[early]
    flags = np.bincount(want[:, 0], minlength=5).tolist()
    print("%s, early exit %s: %d strings, %d rows, flags %s, %d steps of %d symbols, %d walks ended early" % (
        cx.kind, early, n, fm.N, flags, want[:, 4].sum(), fm.N - n, cx.early if early else 0))
    if cx.kind == "fmd":                                            # the figures of the fixture: copies, nothing contained
        assert flags == [1534, 1466, 0, 0, 0] and fm.N - n == 180000 and cx.want[True][:, 4].sum() == 179769 and cx.early == 631
    if cx.kind.startswith("mixed"):
        assert flags == [256, 52, 177, 5, 8] and cx.want[True][:, 4].sum() == 12434 and cx.early == 214
    if cx.kind in ("D", "S"):                                       # unique reads: the full walks are what reach deep into the index
        assert flags[1:] == [0, 0, 0, 0] and cx.want[True][:, 4].sum() < (fm.N - n) // 4
    if not early:
        assert want[:, 4].sum() == fm.N - n                          # every row of the BWT lies on one walk
    with _unchanged(cx.ix), _Env(RB2_CONTAIN_EARLY=int(early)):
        got = g.contained_raw()
        dev = dev_records(g, n, None)
        again = np.zeros((n, 5), np.int64)
        flagged = g.L.rb2_hip_contained(g.h, n, None, again.ctypes.data)
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, "%s: %d of %d records differ; first: string %d got %s want %s" % (cx.kind, len(bad), n, bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())
    assert np.array_equal(dev, want) and np.array_equal(again, want)
    assert got[:, 4].sum() == want[:, 4].sum() and flagged == ((want[:, 0] >= 1) & (want[:, 0] <= 4)).sum()
    assert np.array_equal(g.contained(), want[:, 0])
    inf = g.ssa_info()                                              # the suffix array built beforehand still answers
    assert inf["valid"] and inf["log2_step"] == 4
    stored, hit, cnt = g.locate_raw(cx.iv, 4)
    assert stored == cx.places[0] and np.array_equal(hit, cx.places[1]) and np.array_equal(cnt, cx.places[2])


def test_subsets_and_bad_ids(hip):
    g, fm = mixed_index(hip, 1, False)
    n = int(fm.C[1])
    full = CR.contained(fm)
    assert np.array_equal(g.contained_raw(), full)
    ids = np.concatenate([np.random.RandomState(2).randint(0, n, size=300), [-1, n, 0, n - 1, -1, 2 ** 40, -2 ** 40]])
    assert len(np.unique(ids)) < len(ids) - 50                       # repeats
    want = CR.contained(fm, ids)
    assert np.array_equal(want[:300], full[ids[:300]]) and (want[[300, 301, 304, 305, 306]] == [-1, 0, 0, 0, 0]).all()
    assert np.array_equal(g.contained_raw(ids), want) and np.array_equal(dev_records(g, len(ids), ids), want)
    assert np.array_equal(g.contained(ids.tolist()), want[:, 0])
    rec = np.full((n + 3, 5), FILL, np.int64)                        # ids = NULL and a surplus: three trailing -1 records
    flagged = g.L.rb2_hip_contained(g.h, n + 3, None, rec.ctypes.data)
    assert np.array_equal(rec[:n], full) and (rec[n:] == [-1, 0, 0, 0, 0]).all() and flagged == (full[:, 0] > 0).sum()
    assert np.array_equal(dev_records(g, n + 3, None), rec)
    assert g.L.rb2_hip_contained(g.h, 0, None, None) == 0 and g.contained_raw([]).shape == (0, 5)
    dev_records(g, 0, None)
    e = hip.HipBwt(0)                                               # an empty index: every id is outside it
    assert e.contained_raw().shape == (0, 5) and e.contained_raw([0, 1]).tolist() == [[-1, 0, 0, 0, 0]] * 2
    e.close(); g.close()


def _child(stage):
    p = subprocess.run([sys.executable, os.path.join(HERE, "contain_child.py"), stage], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p.returncode, p.stdout.decode(), p.stderr.decode()[-1500:]


def test_chunked_staging(hip):
    rc, out, err = _child("chunk")
    assert rc == 0 and "STAGE OK" in out, (rc, out, err)


def test_sharded_handle_is_fatal(hip):
    rc, out, err = _child("shard")
    assert rc == 7 and "NOT FATAL" not in out, (rc, out, err)
    assert "contained ok" in out and "handler: [rb2_hip] rb2_hip_contained" in out and "sharded index" in out, out


def _strings(g, n):
    return g.extract(np.arange(n), 64)


def test_reduce_one_strand(hip):
    g, fm = mixed_index(hip, 0, False)
    n = int(fm.C[1])
    want = CR.contained(fm)
    strings = _strings(g, n)
    gone = g.reduce()
    assert gone.dtype == np.int64 and np.array_equal(gone, np.flatnonzero(want[:, 0] > 0)) and len(gone) == 26 + 88 + 2 + 4
    keep = [strings[k] for k in np.flatnonzero(want[:, 0] == 0)]
    assert np.array_equal(g.bwt(), CR.survivors_bwt(0, keep))
    assert not g.contained().any() and len(g.reduce()) == 0 and np.array_equal(g.bwt(), CR.survivors_bwt(0, keep))
    g.close()
    g, _ = mixed_index(hip, 0, False)                                # the copies alone: flags 1 and 3
    gone = g.reduce(contained=False, empty=False)
    assert np.array_equal(gone, np.flatnonzero((want[:, 0] == 1) | (want[:, 0] == 3))) and len(gone) == 28
    keep = [strings[k] for k in np.flatnonzero((want[:, 0] & 1) == 0)]
    assert np.array_equal(g.bwt(), CR.survivors_bwt(0, keep))
    flags = g.contained()
    assert sorted(set(flags.tolist())) == [0, 2, 4]
    g.close()
    g, _ = mixed_index(hip, 0, False)
    with pytest.raises(ValueError):
        g.reduce(pairs=True)                                        # 249 strings are no pairs
    assert int(g.counts()[:, 0].sum()) == n
    assert np.array_equal(g.reduce(duplicates=False, contained=False), np.flatnonzero(want[:, 0] == 4))
    g.close()


def test_reduce_pairs(hip):
    half = np.random.RandomState(5).randint(1, 5, size=12).astype(np.uint8)
    pal = np.concatenate([half, Q.revcomp(half)])                    # its own reverse complement: both strands are the same string
    assert len(pal) == 24 and np.array_equal(Q.revcomp(pal), pal)
    g, fm = mixed_index(hip, 0, True, extra=[pal])
    n = int(fm.C[1])
    want = CR.contained(fm)
    rec = g.contained_raw()
    assert np.array_equal(rec, want) and n == 500
    assert rec[n - 2:].tolist() == [[0, 2, 2, 0, 24], [1, 2, 2, 1, 24]]          # occ == 2: the read and its other strand
    strings = _strings(g, n)
    gone = g.reduce(pairs=True)
    sel = want[:, 0] > 0
    assert np.array_equal(gone, np.flatnonzero(np.repeat(sel[0::2] & sel[1::2], 2))) and len(gone) == sel.sum() - 1
    left = int(g.counts()[:, 0].sum())
    assert left == n - len(gone) and left % 2 == 0
    after = _strings(g, left)
    keep = [strings[k] for k in np.setdiff1d(np.arange(n), gone)]
    assert all(np.array_equal(a, b) for a, b in zip(after, keep))
    assert all(np.array_equal(after[k + 1], Q.revcomp(after[k])) for k in range(0, left, 2))     # every survivor's partner survives
    flags = g.contained()
    assert np.flatnonzero(flags).tolist() == [left - 1] and flags[left - 1] == 1 and np.array_equal(after[left - 1], pal)
    g.close()
    g, _ = mixed_index(hip, 0, True, extra=[pal])                    # without pairs the palindrome loses its partner
    gone = g.reduce()
    assert np.array_equal(gone, np.flatnonzero(sel)) and gone[-1] == n - 1 and (n - 2) not in gone
    assert not g.contained().any() and int(g.counts()[:, 0].sum()) % 2 == 1
    g.close()


def test_index_that_is_no_bwt_of_strings(hip):
    """load_ropes takes any six streams with consistent totals.  On such an index LF is still one-to-one and no row maps into the `$`
    block, so every walk from a string id ends at a `$` (test_contain_ref.py): flag -2 cannot be provoked through the loaders and stays
    a guard.  What can be checked: the call returns, nothing is written out of bounds (the guard words of dev_records), and the records
    are those of the model, whose arithmetic is defined whatever the streams hold"""
    _, bwt = CR.mixed(0, False)
    seen = 0
    for seed in (0, 1):
        bad = CR.shuffled_ropes(bwt, seed)
        fm = Q.FM(bad)
        cut = np.concatenate([fm.C, [fm.N]])
        g = hip.HipBwt(0)
        g.load_ropes([encode_runs(bad[cut[a]:cut[a + 1]]) for a in range(6)])
        n = int(fm.C[1])
        ids = np.concatenate([np.arange(n), [-1, n]])
        for early in (True, False):
            want = CR.contained(fm, ids, early=early)
            assert (want[:n, 0] >= 0).all()
            with _Env(RB2_CONTAIN_EARLY=int(early)):
                assert np.array_equal(g.contained_raw(ids), want) and np.array_equal(dev_records(g, len(ids), ids), want)
            seen += int((want[:n, 1] != CR.contained(Q.FM(bwt), early=early)[:, 1]).sum())
        g.close()
    assert seen > 100                                               # (the answers are not those of the BWT the streams were shuffled from)
