"""GPU tests of the k-mer enumeration (include/rb2_hip.h: rb2_hip_kmers; kernel k_kmer_expand in csrc/rb2_query.h): the k-mers and counts
the device reports must equal the brute force over the strings of the index (tests/kmer_ref.py: sliding windows and np.unique, never a
BWT), and every interval the backward search of its k-mer on the same handle.  The indexes are the five of test_overlap_gpu.py; their
strings are read back with extract.  What can go wrong is addressing -- the ranks of both layouts, the slots drawn per wave, the
segments of the walk, the record staging, the histogram bins in LDS and beyond -- not volume."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fmd_ref
import helpers as H
import kmer_ref as K
import locate_ref as LR
import query_ref as Q
from ropebwt2_amd.hipbwt import encode_runs, pack_kmer, unpack_kmers
from test_fmd_load_gpu import write_fmd
from test_locate_gpu import _small
from test_query_gpu import _Env
from test_query_layouts_gpu import _Models, _build_dense, _build_sparse

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILL = -7                                                            # what the call must leave in the record slots it does not write
KS = [1, 2, 11, 32]
HL = 256                                                             # the bins the kernel counts in LDS (KMER_HL, csrc/rb2_query.h)


@pytest.fixture(scope="module")
def models():
    ms = _Models()
    yield ms
    ms.made.clear()


class _Ctx:
    """an index, its strings by id (read back with extract) and the brute-force k-mers of them, computed once per k"""
    def __init__(self, kind, g, both):
        self.kind, self.g, self.both = kind, g, both
        n = int(g.counts()[:, 0].sum())
        for max_len in (128, 2048, 1 << 15):                        # (the longest strings: 100 in D, 1500 in S, 30000 in longA)
            self.strings = g.extract(np.arange(n), max_len)
            if all(s is not None for s in self.strings):
                break
        assert all(s is not None for s in self.strings)
        self.maxlen = max(len(s) for s in self.strings)
        self.memo = {}

    def brute(self, k, min_occ=1, canonical=False):
        if k not in self.memo:
            self.memo[k] = K.brute(self.strings, k)
        codes, cnt = self.memo[k]
        keep = cnt >= min_occ
        if canonical:
            keep &= K.is_canonical(codes, k)
        return codes[keep], cnt[keep]


@pytest.fixture(scope="module", params=["dense-io", "dense-rclo", "D", "S", "fmd"])
def idx(request, hip, models):
    """the five indexes of test_overlap_gpu.py: dense in input order and in RCLO, layout D (every piece longer than two superblocks),
    layout S (sparse, split leaves), and one loaded from a file the reference wrote (one strand)"""
    kind = request.param
    if kind.startswith("dense"):
        g, fm, _ = _small(hip, 0 if kind == "dense-io" else 2)
    elif kind == "D":
        g = _build_dense(hip, models.get(0)).g
    elif kind == "S":
        g = _build_sparse(hip, models.get("S")).g
    else:
        img, bwt = fmd_ref.fixture("cov3000")
        g = hip.HipBwt(0)
        assert g.load_fmd(np.frombuffer(img, np.uint8)) == len(bwt)
    cx = _Ctx(kind, g, kind != "fmd")
    yield cx
    g.close()


def _search(g, codes, k):
    """backward_search of the unpacked k-mers on the handle: (n, 3) = lo, hi, m (the arrays go to the library as they are)"""
    pat = np.ascontiguousarray(unpack_kmers(codes, k).reshape(-1))
    off = np.arange(len(codes) + 1, dtype=np.int64) * k
    out = np.zeros((len(codes), 3), np.int64)
    if len(codes):
        g.L.rb2_hip_backward_search(g.h, len(codes), pat.ctypes.data, off.ctypes.data, out.ctypes.data)
    return out


def _raw(g, k, min_occ, canonical, max_recs, hist_len, room=None):
    """rb2_hip_kmers on a record array of `room` slots filled with FILL: (found, rec, hist, info)"""
    rec = np.full((max_recs if room is None else room, 3), FILL, np.int64)
    hist = np.full(hist_len, FILL, np.int64)
    info = np.full(4, FILL, np.int64)
    found = g.L.rb2_hip_kmers(g.h, k, min_occ, int(canonical), max_recs, rec.ctypes.data if len(rec) else None, hist_len, hist.ctypes.data if hist_len else None,
                              info.ctypes.data)
    return int(found), rec, hist, info


def _same(got, want, what):
    codes, lo, hi = got
    assert len(codes) == len(want[0]), (what, len(codes), len(want[0]))
    assert np.array_equal(codes, want[0]) and np.array_equal(hi - lo, want[1]), what


@pytest.mark.parametrize("k", KS)
def test_parity_with_brute_force(idx, k):
    """1: the same codes and counts as the windows of the strings; every interval that of backward search; sorted by lo the codes strictly
    increase and the intervals are disjoint"""
    cx, g = idx, idx.g
    assert cx.maxlen >= 32                                          # every one of the five holds strings of 32 symbols: k = 32 runs as it is
    before = g.layout_stats()
    codes, lo, hi = g.kmers(k)
    want = cx.brute(k)
    print("%s k=%d: %d k-mers, %d occurrences" % (cx.kind, k, len(codes), int(want[1].sum())))
    assert len(want[0]) > 0
    _same((codes, lo, hi), want, (cx.kind, k))
    assert codes.dtype == np.uint64 and (codes[1:] > codes[:-1]).all() and (lo[1:] >= hi[:-1]).all() and (hi > lo).all()
    bs = _search(g, codes, k)
    assert np.array_equal(bs[:, 0], lo) and np.array_equal(bs[:, 1], hi) and (bs[:, 2] == k).all()
    assert g.layout_stats() == before, "the enumeration changed the layout"
    if k <= 2 and cx.both:
        assert len(codes) == 4 ** k
    assert int(pack_kmer(unpack_kmers(codes[:1], k)[0])) == int(codes[0])


@pytest.mark.parametrize("min_occ", [2, 3])
def test_min_occ_and_canonical(idx, min_occ):
    """2: min_occ prunes exactly; canonical, on the indexes of both strands, keeps the smaller of a k-mer and its reverse complement"""
    cx, g = idx, idx.g
    for k in (2, 11):
        every = cx.brute(k)
        want = cx.brute(k, min_occ)
        assert 0 < len(want[0]) and (k == 2 or len(want[0]) < len(every[0]))
        _same(g.kmers(k, min_occ), want, (cx.kind, k, min_occ))
        if cx.both:
            for mo in (1, min_occ):
                wc = cx.brute(k, mo, True)
                assert 0 < len(wc[0]) < len(cx.brute(k, mo)[0])
                _same(g.kmers(k, mo, True), wc, (cx.kind, k, mo, "canonical"))
                found, _, hist, info = g.kmers_raw(k, mo, True, 0, 4)
                assert found == len(wc[0]) and info[3] == len(cx.brute(k, mo)[0]) and np.array_equal(hist, K.spectrum(wc[1], 4))
    if cx.both:                                                     # palindromes (AT, CG, GC, TA) are reported, once
        codes = g.kmers(2, 1, True)[0]
        pals = K.pack(np.array([[1, 4], [2, 3], [3, 2], [4, 1]], np.uint8))
        assert np.isin(pals, codes).all() and len(np.unique(codes)) == len(codes) == 10


@pytest.fixture(scope="module")
def longA(hip):
    img, bwt = fmd_ref.fixture("longA")
    g = hip.HipBwt(0)
    assert g.load_fmd(np.frombuffer(img, np.uint8)) == len(bwt)
    cx = _Ctx("longA", g, False)
    yield cx
    g.close()


@pytest.mark.parametrize("hist_len", [1, 2, 4, HL, HL + 44, 100000])
def test_histogram_hot_bin_and_overflow(longA, hist_len):
    """3: runs of 30000 A: one k-mer with tens of thousands of occurrences, at k = 1 and 2 beside three with one; bins in LDS, bins beyond
    it, the last bin folded (the hot bins of many k-mers: test_histogram_on_the_indexes)"""
    cx, g = longA, longA.g
    for k in (1, 2, 32):
        codes, cnt = cx.brute(k)
        assert cnt.max() > 80000 and ((cnt == 1).sum() == 3 or k == 32)
        for min_occ in (1, 2):
            c = cnt[cnt >= min_occ]
            hist = g.kmer_spectrum(k, hist_len, min_occ)
            assert hist.sum() == len(c) and np.array_equal(hist, K.spectrum(c, hist_len)), (k, hist_len, min_occ, hist[:8], hist[-3:])
            assert hist[:min(min_occ, hist_len - 1)].sum() == 0
    assert np.array_equal(g.kmers_raw(5, 1, False, 0, 0)[2], np.zeros(0, np.int64))


@pytest.mark.parametrize("hist_len", [1, 4, HL, HL + 44])
def test_histogram_on_the_indexes(idx, hist_len):
    """3, on the five: at k = 11 nearly every k-mer of D and S falls into the first bins; at k = 1 and 2 counts lie beyond the LDS bins"""
    cx, g = idx, idx.g
    for k in (1, 2, 11):
        codes, cnt = cx.brute(k)
        if k <= 2:
            assert cnt.max() >= HL + 44
        hist = g.kmer_spectrum(k, hist_len)
        assert np.array_equal(hist, K.spectrum(cnt, hist_len)), (cx.kind, k, hist_len)
        found, rec, h2, info = g.kmers_raw(k, 1, False, 7, hist_len)                                     # the same beside records
        assert found == len(codes) and np.array_equal(h2, hist)


def _walk(g, k, env, **kw):
    with _Env(**env):
        found, rec, hist, info = g.kmers_raw(k, kw.get("min_occ", 1), kw.get("canonical", False), kw["max_recs"], 8)
    rec = rec[:min(found, kw["max_recs"])]
    return found, rec[np.argsort(rec[:, 1], kind="stable")], hist, info


def test_bounded_frontier(idx):
    """4: RB2_KMER_FRONTIER = 4 (one item per slice) on the smallest index, 64 on D and S: the same records as with the default, and info
    shows the slices; RB2_KMER_STAGE = 32 on top makes the record staging flush every few slices"""
    cx, g = idx, idx.g
    if cx.kind in ("dense-io", "dense-rclo"):
        F, k = 4, 11
    elif cx.kind in ("D", "S"):
        F, k = 64, 8
    else:
        F, k = 64, 11
    n = len(cx.brute(k)[0])
    found, rec, hist, info = _walk(g, k, {}, max_recs=n)
    assert found == n and info[0] == k and info[1] >= 1 and info[2] == 1 and info[3] == n              # the default: one slice per level
    for env in ({"RB2_KMER_FRONTIER": F}, {"RB2_KMER_FRONTIER": F, "RB2_KMER_STAGE": 32}):
        f2, r2, h2, i2 = _walk(g, k, env, max_recs=n)
        print(cx.kind, env, "info", i2.tolist())
        assert f2 == n and np.array_equal(r2, rec) and np.array_equal(h2, hist)
        assert i2[0] > k and 1 < i2[1] <= F and i2[2] > 1 and i2[3] == n
    f3, r3, h3, i3 = _walk(g, k, {"RB2_KMER_FRONTIER": F, "RB2_KMER_STAGE": 32}, max_recs=n, min_occ=2, canonical=cx.both)
    f4, r4, h4, i4 = _walk(g, k, {}, max_recs=n, min_occ=2, canonical=cx.both)
    assert f3 == f4 == len(cx.brute(k, 2, cx.both)[0]) > 0 and np.array_equal(r3, r4) and np.array_equal(h3, h4) and i3[3] == i4[3]
    with _Env(RB2_KMER_FRONTIER=1):                                  # below the minimum: 4
        f5, _, _, i5 = g.kmers_raw(3, 1, False, 0, 0)
    assert f5 == len(cx.brute(3)[0]) and i5[1] <= 4


def test_max_recs(idx):
    """5: whatever max_recs, the same return value and histogram; min(found, max_recs) distinct true records; the slots behind them untouched"""
    cx, g = idx, idx.g
    k = 11
    codes, cnt = cx.brute(k)
    n = len(codes)
    f0, rec0, hist0, info0 = _raw(g, k, 1, False, n, 16)
    rec0 = rec0[np.argsort(rec0[:, 1], kind="stable")]
    fc = rec0[:, 0].astype(np.uint64)
    assert f0 == n > 5 and np.array_equal(fc, codes) and np.array_equal(rec0[:, 2] - rec0[:, 1], cnt) and np.array_equal(hist0, K.spectrum(cnt, 16))
    cases = [({}, m) for m in (0, 1, n - 1, n, n + 5)]
    if cx.kind == "D":                                              # ... and cut while the staging buffer is flushed again and again
        cases.append(({"RB2_KMER_FRONTIER": 4096, "RB2_KMER_STAGE": 512}, n - 1))
    for env, max_recs in cases:
        with _Env(**env):
            found, rec, hist, info = _raw(g, k, 1, False, max_recs, 16, room=max_recs + 3)
        m = min(n, max_recs)
        assert found == n and np.array_equal(hist, hist0) and info[3] == n, (cx.kind, max_recs)
        assert (rec[m:] == FILL).all(), "records beyond min(found, max_recs) were written"
        got = rec[:m]
        gc = got[:, 0].astype(np.uint64)
        at = np.minimum(np.searchsorted(fc, gc), n - 1)
        assert len(np.unique(gc)) == m and np.array_equal(fc[at], gc) and np.array_equal(rec0[at, 1:], got[:, 1:])


def test_lifecycle(hip, tmp_path):
    """6: an empty index; a second insert left pending; a suffix array built before the call; the same index through load_fmd"""
    g = hip.HipBwt(0)
    found, rec, hist, info = _raw(g, 5, 1, False, 4, 6)
    assert found == 0 and (hist == 0).all() and (rec == FILL).all() and info.tolist() == [0, 0, 0, 0]
    assert g.kmers(3)[0].dtype == np.uint64 and len(g.kmers(3)[0]) == 0 and g.kmer_spectrum(3, 4).tolist() == [0, 0, 0, 0]
    a, b = H.repetitive_reads(200, seed=61, max_len=40), H.repetitive_reads(150, seed=62, max_len=40)
    g.insert_multi(H.encode_batch(a, True, True))
    sa = Q.inserted_strings(a, True, True)
    _same(g.kmers(9), K.brute(sa, 9), "first batch")
    g.set_lazy(1)
    g.insert_multi(H.encode_batch(b, True, True))                   # (lazy: the rounds may still be queued when the query begins)
    sab = sa + Q.inserted_strings(b, True, True)
    _same(g.kmers(9), K.brute(sab, 9), "grown index")
    assert len(K.brute(sab, 9)[0]) > len(K.brute(sa, 9)[0])
    # a sampled suffix array built before the enumeration is valid behind it, and the intervals of the records locate the k-mers
    g.build_ssa(3)
    inf = g.ssa_info()
    fm = Q.FM(g.bwt())
    sid, pos, _ = LR.suffix_array(fm)
    codes, lo, hi = g.kmers(9, 2)
    assert g.ssa_info() == inf and inf["valid"]
    hits = g.locate(np.stack([lo, hi], 1), max_hits=int((hi - lo).max()))
    w = unpack_kmers(codes, 9)
    for i in range(0, len(codes), 5):
        assert len(hits[i]) == hi[i] - lo[i] >= 2
        assert sorted(map(tuple, hits[i].tolist())) == sorted(zip(sid[lo[i]:hi[i]].tolist(), pos[lo[i]:hi[i]].tolist()))
        for s, p in hits[i].tolist():                                # input order: string s is the s-th inserted
            assert np.array_equal(sab[s][p:p + 9], w[i])
    # the same strings through an .fmd: the same records, intervals included
    want = g.kmers(12)
    g2 = hip.HipBwt(0)
    assert g2.load_fmd(write_fmd(tmp_path / "k.fmd", [encode_runs(r) for r in g.ropes()])) == fm.N
    got = g2.kmers(12)
    assert len(want[0]) > 100 and all(np.array_equal(x, y) for x, y in zip(got, want))
    assert np.array_equal(g2.kmer_spectrum(12, 300), g.kmer_spectrum(12, 300))
    g.reset()
    assert g.kmers_raw(4, 1, False, 0, 0)[0] == 0
    g.close()
    g2.close()


@pytest.mark.parametrize("stage,what", [("k0", "k must be"), ("k33", "k must be"), ("minocc0", "min_occ"), ("negrecs", "max_recs"), ("neghist", "hist_len"),
                                        ("nullrec", "rec is NULL"), ("nullhist", "hist is NULL"), ("shard", "sharded index")])
def test_fatal_parameters(hip, stage, what):
    """7: each leaves through the fatal handler with the function's name in the message"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "kmer_child.py"), stage], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 7 and "NOT FATAL" not in out, (p.returncode, out, p.stderr.decode()[-1500:])
    assert "kmers ok" in out and "handler: [rb2_hip] kmers:" in out and what in out, out
