"""CPU tests of the weighted-BWT model (tests/weighted_ref.py): the multiset claim against the oracle in the three sorting orders, the
views and the laws against query_ref.FM / locate_ref / overlap_ref on the expanded BWT, every *_ref module on the model against the same
module on the expanded BWT, and what the two fixtures of tests/test_big_rows_gpu.py are meant to provide.  No GPU needed."""
import numpy as np
import pytest

import approx_ref as AR
import contain_ref as CR
import fmd_streams as F
import helpers as H
import irreducible_ref as IR
import kmer_ref as KR
import locate_ref as LR
import overlap_ref as OV
import query_ref as Q
import smem_ref as SR
import weighted_ref as W
from test_locate_ref import patterns, string_sets

NAMES = ["repetitive", "repetitive-both", "tiny", "tiny-both"]
T32, T24 = 1 << 32, 1 << 24


def distinct(name):
    """the strings of a set of test_locate_ref.py (both strands where it says so), each once, and weights 1..7 drawn per string"""
    reads, rev = string_sets()[name]
    D, seen = [], set()
    for s in Q.inserted_strings(reads, True, rev):
        if s.tobytes() not in seen:
            seen.add(s.tobytes())
            D.append(s)
    return D, np.random.RandomState(len(D)).randint(1, 8, size=len(D))


def oracle_bwt(so, batches):
    o = H.Oracle(so)
    for b in batches:
        o.insert_multi(H.encode_batch(b, True, False))
    bwt = o.bwt()
    o.close()
    return bwt


_pairs = {}


def pair(name, so=1):
    """(the model, query_ref.FM of the expanded BWT), made once"""
    if (name, so) not in _pairs:
        D, w = distinct(name)
        m = W.from_strings(so, D, w)
        _pairs[name, so] = m, Q.FM(np.repeat(m.bwt0, m.wrow))
    return _pairs[name, so]


@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_multiset_claim_against_the_oracle(name, so):
    D, w = distinct(name)
    assert w.min() >= 1 and w.max() <= 7 and (w > 1).sum() >= 3
    m = W.from_strings(so, D, w)
    want = np.repeat(m.bwt0, m.wrow)
    rng = np.random.RandomState(so)
    cons = W.copies(D, w)
    shuf = [cons[i] for i in rng.permutation(len(cons))]
    extra = W.copies(D, w - 1)
    extra = [extra[i] for i in rng.permutation(len(extra))]
    got = [oracle_bwt(so, [cons]), oracle_bwt(so, [shuf]), oracle_bwt(so, [D, extra])]
    assert np.array_equal(got[0], want), "consecutive copies"
    if so == 0:                                                     # input order: the copies must be consecutive -- the limitation stays visible
        assert not np.array_equal(got[1], want) and not np.array_equal(got[2], want)
    else:
        assert np.array_equal(got[1], want), "shuffled copies"
        assert np.array_equal(got[2], want), "extra copies in a second batch"


@pytest.mark.parametrize("name", NAMES)
def test_views_against_the_expanded_bwt(name):
    m, big = pair(name)
    N = big.N
    assert m.N == N and np.array_equal(m.C, big.C) and m.n_strings == int(big.C[1])
    rows = np.arange(N + 1)
    assert np.array_equal(m.occ[rows], big.occ) and np.array_equal(m.bwt[rows[:-1]], big.bwt)
    assert m.start[0] == 0 and m.start[-1] == N and len(m.start) == m.n0 + 1
    for x in (0, 1, N // 2, N - 1, N):
        assert np.array_equal(m.occ[x], big.occ[x]) and m.block(x) == (int(np.searchsorted(m.start, x, "right")) - 1, x - int(m.start[m.block(x)[0]]))
        for c in range(6):
            assert m.occ[x, c] == big.occ[x, c]
        if x < N:
            assert m.bwt[x] == big.bwt[x]
    cs = rows % 6
    assert np.array_equal(m.occ[rows, cs], big.occ[rows, cs]) and np.array_equal(m.occ[rows, 0], big.occ[rows, 0])
    assert np.array_equal(m.occ[N, cs[:12]], big.occ[N, cs[:12]]) and np.array_equal(m.occ[:, 0][rows], big.occ[:, 0][rows])
    for bad in (-1, N + 1):
        with pytest.raises(AssertionError):
            m.occ[bad]
    with pytest.raises(TypeError):
        m.walk_all()
    with pytest.raises(TypeError):
        LR.suffix_array(m)
    with pytest.raises(TypeError):
        OV.head(m)
    pats = patterns(m.D, np.random.RandomState(len(m.D)))
    for p in pats + [np.array([1, 0, 2], np.uint8), np.array([7, 1], np.uint8)]:
        assert m.backward_search(p) == big.backward_search(p) == m.interval(p), p.tolist()
        assert m.count(p) == big.count(p)
    iks = np.stack([rows, rows[::-1], np.minimum(np.arange(N + 1) % 9, N - rows)], 1)
    for is_back in (0, 1):
        assert np.array_equal(m.extend_many(iks, is_back), big.extend_many(iks, is_back))
        for ik in iks[::7]:
            assert np.array_equal(m.extend(ik, is_back), big.extend(ik, is_back))
    for c in range(6):
        assert m.sym_interval(c) == big.sym_interval(c)
    for q in range(m.n_strings):
        assert np.array_equal(m.walk(q), big.walk(q)) and np.array_equal(m.text(q), big.walk(q))
    assert np.array_equal(W.counts(m), np.array([np.bincount(big.bwt[big.C[b]:(list(big.C) + [N])[b + 1]], minlength=6) for b in range(6)]))
    S = m.runs()
    F.check(S)
    assert np.array_equal(np.repeat([c for _, c in S], [l for l, _ in S]), big.bwt)


@pytest.mark.parametrize("name", NAMES)
def test_laws_against_the_expanded_bwt(name):
    m, big = pair(name)
    N, n = big.N, int(big.C[1])
    sid, pos, lens = LR.suffix_array(big)
    s, p = m.locate_rows(np.arange(N))
    assert np.array_equal(s, sid) and np.array_equal(p, pos)
    q0, t = m.string_of(np.arange(n))
    assert np.array_equal(q0, np.repeat(np.arange(len(m.wq)), m.wq)) and np.array_equal(t, np.arange(n) - m.start[q0])
    assert [len(m.text(k)) for k in range(n)] == lens.tolist()
    assert np.array_equal(m.head(np.arange(n)), OV.head(big))
    z = m.occ[np.arange(N + 1), 0]                                  # `$` ranks go through occ[.., 0]
    assert np.array_equal(z, big.occ[:, 0])
    iv = [(0, N), (0, 0), (N, N), (3, 9), (N - 2, N), (-1, 2), (0, N + 1), (5, 4)] + [(x, min(x + 4, N)) for x in range(0, N, 5)]
    for mh in (1, 5):
        for a, b in zip(m.locate_raw(iv, mh), LR.locate_raw(big, iv, mh)):
            assert np.array_equal(a, b)
    zv = [(0, n), (0, 0), (n, n), (1, min(4, n)), (-1, 2), (0, n + 1), (3, 2)] + [(x, min(x + 3, n)) for x in range(0, n, 2)]
    for mh in (1, 4):
        for a, b in zip(m.string_ids_raw(zv, mh), OV.string_ids_raw(big, zv, mh)):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("name", NAMES)
def test_ref_modules_run_on_the_model(name):
    m, big = pair(name)
    rng = np.random.RandomState(7)
    qs = [s for s in m.D if len(s)][:40] + [rng.randint(1, 6, size=rng.randint(1, 12)).astype(np.uint8) for _ in range(20)] + [np.array([1, 0, 2], np.uint8)]
    for mo in (1, 3):
        for a, b in zip(OV.overlap_raw(m, qs, mo, 8), OV.overlap_raw(big, qs, mo, 8)):
            assert np.array_equal(a, b)
        assert [OV.overlap(m, q, mo)[1] for q in qs[:10]] == [OV.overlap(big, q, mo)[1] for q in qs[:10]]
    for k, mo, canon in ((1, 1, False), (3, 2, False), (5, 1, True), (2, 6, False)):
        for a, b in zip(KR.model(m, k, mo, canon), KR.model(big, k, mo, canon)):
            assert np.array_equal(a, b)
    for mm, mo in ((1, 1), (2, 3)):
        ra, ca = AR.approx_raw(m, qs[:25] + qs[-5:], mm, mo)
        rb, cb = AR.approx_raw(big, qs[:25] + qs[-5:], mm, mo)
        assert ra == rb and np.array_equal(ca, cb) and (ca > 0).any()
    for q in qs[:15] + qs[-3:]:
        for ml, mo in ((1, 1), (3, 2)):
            a, b = SR.smems(m, q, ml, mo), SR.smems(big, q, ml, mo)
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b))
        if not SR.malformed(q):
            assert np.array_equal(SR.occ_table(m, q), SR.occ_table(big, q))
    for early in (True, False):
        ids = np.concatenate([np.arange(int(big.C[1])), [-1, int(big.C[1])]])
        assert np.array_equal(CR.contained(m, ids, early), CR.contained(big, ids, early))
    for a, b in zip(IR.irreducible_raw(m, qs, 2, 30), IR.irreducible_raw(big, qs, 2, 30)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["repetitive", "tiny-both"])
def test_copy_0_carries_no_duplicate_bit(name):
    """contain_ref on the model: copy t = 0 of a string is the first of its text, copies t >= 1 carry bit 0; n_equal is the weight"""
    m, _ = pair(name)
    n = m.n_strings
    rec = CR.contained(m, np.arange(n), early=False)
    q0, t = m.string_of(np.arange(n))
    live = rec[:, 0] != 4                                           # (the empty string has a record of its own)
    assert live.sum() >= n - m.wq.max()
    assert np.array_equal(rec[live, 0] & 1, (t[live] >= 1) * 1) and np.array_equal(rec[live, 3], t[live])
    assert np.array_equal(rec[live, 2], m.wq[q0[live]])


@pytest.mark.parametrize("name", NAMES)
def test_reweighted(name):
    """after a delete, an insert of copies or a merge the model is that of the new weights; a weight of 0 drops the string"""
    m, _ = pair(name)
    w = m.weights()
    assert np.array_equal(w, distinct(name)[1])
    rng = np.random.RandomState(3)
    w2 = np.maximum(w + rng.randint(-7, 4, size=len(w)), 0)
    assert (w2 == 0).any() and (w2 > w).any()
    m2 = m.reweighted(w2)
    keep = [m.D[j] for j in np.flatnonzero(w2)]
    assert np.array_equal(np.repeat(m2.bwt0, m2.wrow), oracle_bwt(1, [W.copies(keep, w2[w2 > 0])]))
    assert m2.n_strings == w2.sum() and np.array_equal(m2.weights(), w2[w2 > 0])
    m3 = m.reweighted(w + 2)                                        # (no string drops out: the same small index)
    assert np.array_equal(m3.bwt0, m.bwt0) and np.array_equal(m3.wrow, m.wrow + 2)


# ---- the fixtures of tests/test_big_rows_gpu.py ------------------------------------------------------------------------------------------

def _common(m):
    S = m.runs()
    F.check(S)
    assert sum(l for l, _ in S) == m.N and np.array_equal(F.counts(S), W.counts(m)) and np.array_equal(F.borders(S)[:6], m.C)
    assert len(S) < 10000 and m.so == 1
    assert len({s.tobytes() for s in m.D}) == len(m.D) == 300 - 150 * (m.name == "skewed")
    rows, size = W.piece_rows(m)
    assert size.sum() == m.N and (np.diff(rows) == size[:-1]).all()
    assert len(min(m.D, key=len)) <= 21 and len(max(m.D, key=len)) >= 198
    return rows, size


def test_fixture_even():
    m = W.fixture("even")
    rows, size = _common(m)
    assert 25000 < m.n0 < 40000
    assert m.N > 1.25 * T32
    assert (m.C[1:] >= T32).sum() >= 2 and (m.C[1:] < T32).sum() >= 2       # ropes that begin at or above 2^32, and below
    assert (size < T32).all()                                       # every piece below 2^32 symbols: an insert stores positions in 32 bits
    assert m.n_strings > 3 * T24
    assert all(np.array_equal(Q.revcomp(m.D[i]), m.D[i + 1]) for i in range(0, len(m.D), 2))     # both strands, pair by pair ...
    assert np.array_equal(m.weights()[0::2], m.weights()[1::2])             # ... with one weight per pair
    assert any((s == 5).any() for s in m.D) and all(12 <= len(s) <= 200 for s in m.D)
    r = int(np.searchsorted(rows, T32, "right")) - 1
    assert H.rope_sym(r) == 3 and rows[r] < T32 < rows[r] + size[r]         # row 2^32 lies inside a piece of rope G


def test_fixture_skewed():
    m = W.fixture("skewed")
    rows, size = _common(m)
    assert m.N > 2 * T32 and m.n_strings > 4 * T24
    assert size[H.rope_of(1, 1)] > T32                              # piece (A,A): wide positions in an insert, offsets past 32 bits in qrank
    assert all(20 <= len(s) <= 200 for s in m.D)
    sym = np.concatenate(m.D)
    assert 0.8 < (sym == 1).mean() < 0.9
