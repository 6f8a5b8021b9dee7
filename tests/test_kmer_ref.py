"""CPU tests of the k-mer model (tests/kmer_ref.py): the level-wise expansion over a BWT against the brute force over the strings, which
never looks at a BWT, on the string sets of test_locate_ref.py (and one of longer strings, so that k = 32 is not empty) in the three
sorting orders; and of what the package exports for it.  No GPU needed."""
import numpy as np
import pytest

import kmer_ref as K
import query_ref as Q
from test_locate_ref import build, string_sets

KS = [1, 2, 5, 12, 32]
PAL12 = np.array([1, 2, 3, 4] * 3, np.uint8)                         # ACGTACGTACGT is its own reverse complement


def long_reads():
    """reads of 20 .. 70 symbols from a genome of 160 that holds a palindromic 12-mer; a few N, duplicates"""
    rng = np.random.RandomState(32)
    genome = rng.randint(1, 5, size=160).astype(np.uint8)
    genome[40:52] = PAL12
    out = []
    for _ in range(60):
        ln = rng.randint(20, 71)
        st = rng.randint(0, len(genome) - ln + 1)
        r = genome[st:st + ln].copy()
        if rng.rand() < 0.15:
            r[rng.randint(0, ln)] = 5
        out.append(r)
    out.append(genome[30:70].copy())                                # the palindrome for certain
    return out + [out[3].copy(), out[7].copy()]


def all_sets():
    s = dict(string_sets())
    s["long"] = (long_reads(), False)
    s["long-both"] = (long_reads(), True)
    return s


@pytest.fixture(scope="module", params=[(name, so) for name in ("repetitive", "repetitive-both", "tiny", "tiny-both", "long", "long-both") for so in (0, 1, 2)],
                ids=lambda p: "%s-so%d" % p)
def case(request):
    name, so = request.param
    reads, rev = all_sets()[name]
    fm, strings = build(reads, rev, so)
    return name, rev, fm, strings


def test_pack_unpack_revcomp():
    rng = np.random.RandomState(1)
    for k in range(1, 33):
        w = rng.randint(1, 5, size=(50, k)).astype(np.uint8)
        c = K.pack(w)
        assert np.array_equal(K.unpack(c, k), w)
        assert np.array_equal(np.argsort(c, kind="stable"), np.lexsort(w.T[::-1]))          # numeric order = lexicographic order
        rc = K.revcomp_codes(c, k)
        assert np.array_equal(K.unpack(rc, k), np.stack([Q.revcomp(x) for x in w]))
        assert np.array_equal(K.revcomp_codes(rc, k), c)
    assert int(K.pack(PAL12[None, :])[0]) == int(K.revcomp_codes(K.pack(PAL12[None, :]), 12)[0])
    assert int(K.pack(np.array([[4] * 32], np.uint8))[0]) == 2 ** 64 - 1 and int(K.pack(np.array([[1, 2, 3, 4]], np.uint8))[0]) == 0b00011011


@pytest.mark.parametrize("k", KS)
def test_model_against_brute_force(case, k):
    name, rev, fm, strings = case
    full = None
    for min_occ in (1, 2, 3):
        for canonical in ((False, True) if rev else (False,)):
            codes, lo, hi, pre = K.model(fm, k, min_occ, canonical)
            want, cnt = K.brute(strings, k, min_occ, canonical)
            assert np.array_equal(codes, want) and np.array_equal(hi - lo, cnt), (name, k, min_occ, canonical)
            assert (np.diff(codes.astype(object)) > 0).all() and (lo[1:] >= hi[:-1]).all()      # sorted by lo = sorted by code; disjoint
            assert pre == len(K.brute(strings, k, min_occ, False)[0])
            for c, a, b in list(zip(codes, lo, hi))[::7]:                                          # the interval is the one of backward search
                assert fm.backward_search(K.unpack([c], k)[0]) == (a, b, k)
            if canonical:                                           # both strands: a k-mer and its reverse complement occur equally often
                allc, allcnt = K.brute(strings, k, min_occ, False)
                d = dict(zip(allc.tolist(), allcnt.tolist()))
                rc = K.revcomp_codes(allc, k).tolist()
                assert all(d.get(r) == d[c] for c, r in zip(allc.tolist(), rc))
                assert len(codes) == sum(1 for c, r in zip(allc.tolist(), rc) if c <= r)
            if min_occ == 1 and not canonical:
                full = (codes, hi - lo)
    codes, cnt = full
    if k == 12 and not name.startswith("tiny"):
        assert (cnt >= 2).any() and (cnt == 1).any(), (name, np.bincount(cnt))
        two = K.brute(strings, k, 2)[0]
        assert 0 < len(two) < len(codes)
    if k == 32:
        assert (len(codes) > 0) == name.startswith("long")


def test_palindromes_are_reported_once():
    reads, rev = all_sets()["long-both"]
    fm, strings = build(reads, rev)
    pal = int(K.pack(PAL12[None, :])[0])
    codes, lo, hi, pre = K.model(fm, 12, 1, True)
    assert (codes == np.uint64(pal)).sum() == 1
    i = int(np.flatnonzero(codes == np.uint64(pal))[0])
    assert hi[i] - lo[i] == Q.brute_count(strings, PAL12) >= 2
    every = K.model(fm, 12, 1, False)[0]
    rc = K.revcomp_codes(every, 12)
    assert len(codes) == ((every < rc).sum() + (every == rc).sum()) and (every == rc).sum() >= 1
    reads, rev = all_sets()["repetitive-both"]                      # k = 2: AT, CG, GC, TA are palindromes
    fm, strings = build(reads, rev)
    codes = K.model(fm, 2, 1, True)[0]
    pals = K.pack(np.array([[1, 4], [2, 3], [3, 2], [4, 1]], np.uint8))
    assert np.isin(pals, codes).any() and len(set(codes.tolist())) == len(codes)


def test_spectrum_and_edges():
    assert K.spectrum([1, 1, 2, 5, 9], 4).tolist() == [0, 2, 1, 2]
    assert K.spectrum([1, 1, 2], 1).tolist() == [3] and K.spectrum([3], 0).tolist() == []
    fm = Q.FM(np.zeros(0, np.uint8))
    assert len(K.model(fm, 3)[0]) == 0 and K.model(fm, 3)[3] == 0
    assert len(K.brute([], 3)[0]) == 0 and len(K.brute([np.array([1, 2], np.uint8)], 3)[0]) == 0
    codes, cnt = K.brute([np.array([1, 5, 1, 1, 0 + 2], np.uint8)], 2)                # A N A A C: the windows with N are none
    assert K.unpack(codes, 2).tolist() == [[1, 1], [1, 2]] and cnt.tolist() == [1, 1]


def test_kmer_symbols_exported():
    from ropebwt2_amd import build_all, load_hip_lib
    build_all()
    assert hasattr(load_hip_lib(), "rb2_hip_kmers")
    from ropebwt2_amd import HipBwt
    from ropebwt2_amd.hipbwt import pack_kmer, unpack_kmers
    for m in ("kmers_raw", "kmers", "kmer_spectrum"):
        assert callable(getattr(HipBwt, m, None)), m
    rng = np.random.RandomState(2)
    for k in (1, 2, 31, 32):
        w = rng.randint(1, 5, size=(20, k)).astype(np.uint8)
        codes = np.array([pack_kmer(x) for x in w], np.uint64)
        assert np.array_equal(codes, K.pack(w)) and np.array_equal(unpack_kmers(codes, k), w)
    assert int(pack_kmer("acgt")) == 0b00011011 and int(pack_kmer(b"T" * 32)) == 2 ** 64 - 1
    for bad in ("", "A" * 33, "ACN", "AC$"):
        with pytest.raises(ValueError):
            pack_kmer(bad)
