"""GPU tests of the approximate search with insertions and deletions (include/rb2_hip.h: rb2_hip_approx_ed[_dev]; kernel k_approx_ed in
csrc/rb2_edit.h): the records and counts the device reports must equal the trie model on the BWT of the same index (tests/approx_ed_ref.py,
which tests/test_approx_ed_ref.py holds against brute force), and for a part of the queries the brute force over the strings itself.  The
indexes are small -- the Python references are the limit, and what can go wrong is control flow, the band at its edges and the addressing
of the stacks, not volume: the whole query set runs at max_ed 0, 1, 2, and max_ed 3 and 4 on the queries of at most 10 symbols."""
import os
import subprocess
import sys

import numpy as np
import pytest

import approx_ed_ref as ER
import fmd_ref
import helpers as H
import locate_ref as LR
import query_ref as Q
from ropebwt2_amd.hipbwt import StepBudgetExceeded, pack_patterns
from test_locate_gpu import _small
from test_query_gpu import _Env, _batches
from test_query_layouts_gpu import FORCED

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILL = -7                                                            # what the device variant must leave in the slots it does not write
MALFORMED = [[1, 0], [0], [1, 0, 2], [7, 1], [3, 6], [1] * 8193]
STEPS = 1 << 20                                                      # a budget none of these queries uses up
SHORT = 10                                                           # max_ed 3 and 4 run on the queries of up to this many symbols


def row_bytes(L, max_ed):
    """edit_row_bytes of csrc/rb2_edit_plan.h"""
    P = L + max_ed
    return 72 * P + (P + 7) // 8 * 8 + (L + 7) // 8 * 8


def plant(rng, w, edits):
    """w with the edits (kind, at) planted, positions counted in w: 's' another symbol at `at`, 'd' the symbol at `at` deleted, 'i' a
    symbol inserted in front of `at`"""
    t = [int(c) for c in w]
    for kind, at in sorted(edits, key=lambda e: (-e[1], e[0] != "s")):
        if kind == "s":
            t[at] = 1 + (t[at] + rng.randint(3)) % 4
        elif kind == "d":
            del t[at]
        else:
            t.insert(at, int(rng.randint(1, 5)))
    return np.array(t, np.uint8)


class _Ctx:
    """an index, its model, its strings by id (read back with extract), the queries, which of them were planted from which word, and the
    model's answers, computed once per (max_ed, min_occ)"""
    def __init__(self, kind, g, fm, both, nq=10):
        self.kind, self.g, self.fm, self.both = kind, g, fm, both
        n = int(fm.C[1])
        lens = LR.suffix_array(fm)[2]
        self.strings = g.extract(np.arange(n), int(lens.max()))
        rng = np.random.RandomState(n)
        clean = [s for s in self.strings if len(s) >= 14 and not (s == 5).any()]
        # lengths 0 .. 3; N alone, at either end, in the middle
        qs = [np.array(q, np.uint8) for q in ([], [1], [4], [2, 3], [1, 1], [1, 2, 3], [5], [5, 5], [5, 1], [1, 5], [1, 5, 2])]
        self.planted = []                                            # (query, the word it was made from, edits planted away from the ends)

        def add(w, edits):
            self.planted.append((len(qs), w, len(edits)))
            qs.append(plant(rng, w, edits))

        for i in range(nq):
            s = clean[rng.randint(len(clean))]
            a = rng.randint(len(s) - 13)
            w = s[a:a + rng.randint(12, min(40, len(s) - a) + 1)].copy()
            L, m = len(w), len(w) // 2
            qs.append(s.copy() if i % 3 == 0 else w.copy())          # the full length of a string; a substring
            for at in (1, L - 2, m):                                 # one edit of each kind at the first places an indel may stand, and in the middle
                add(w, [("s", at)]); add(w, [("d", at)]); add(w, [("i", at if at != L - 2 else L - 1)])
            add(w, [("d", m), ("d", m + 1)])                         # two adjacent deletions
            add(w, [("i", m), ("s", m)])                             # an insertion next to a substitution
            add(w, [("s", 2), ("d", m), ("i", L - 2)])               # one of each (too long for max_ed = 3 here: parity at 0 .. 2 only)
            for edits in ([("s", 0)], [("s", L - 1)], [("d", 0)], [("d", L - 1)], [("i", 0)], [("i", L)]):   # at the ends: a substitution or nothing
                qs.append(plant(rng, w, edits))
            for at in (0, L - 1, m):                                 # N at either end and in the middle
                t = w.copy(); t[at] = 5; qs.append(t)
            v = w[:9].copy()                                         # short ones, which max_ed 3 and 4 take too: 8 .. 10 symbols
            add(v, [(("s", "d", "i")[i % 3], 4)])
            add(v, [("d", 2), ("i", 6)])
            add(v, [("s", 1), ("i", 4), ("d", 7)])
            add(v, [("d", 3), ("d", 4), ("s", 6)])
        longest = max(self.strings, key=len)
        qs.append(np.concatenate([longest, longest[:3]]).astype(np.uint8))                         # longer than every string
        qs.append(np.concatenate([clean[0], [1, 2, 3, 4] * 3, clean[1]]).astype(np.uint8))         # ... and with pieces in it
        qs.append(np.resize(np.concatenate([clean[0], clean[1]]), 8192).astype(np.uint8))          # the longest query there is
        self.n_well = len(qs)
        self.queries = qs + [np.array(q, np.uint8) for q in MALFORMED]
        self.short = [i for i, q in enumerate(self.queries) if len(q) <= SHORT]
        self.memo = {}

    def want(self, max_ed, min_occ=1):
        """the model's (records, cnt) of all queries at max_ed <= 2, of the short ones above"""
        key = (max_ed, min_occ)
        if key not in self.memo:
            self.memo[key] = ER.approx_ed_raw(self.fm, self.asked(max_ed), max_ed, min_occ)
        return self.memo[key]

    def asked(self, max_ed):
        return self.queries if max_ed <= 2 else [self.queries[i] for i in self.short]


def _forced_sparse(hip, rev):
    batches, _ = _batches(210, rev)
    with _Env(**FORCED):
        g = hip.HipBwt(0)
    for b in batches:
        g.insert_multi(b)
    assert g.layout_stats()["sparse_now"]
    return g


@pytest.fixture(scope="module", params=["dense-both", "dense-one", "sparse-both", "sparse-one", "fmd"])
def idx(request, hip):
    """a dense index of both strands (that of test_locate_gpu.py) and one of one strand; the same two kept in the sparse layout by the
    forced-sparse environment; an index loaded from a file the reference wrote (one strand)"""
    kind = request.param
    both = kind.endswith("both")
    if kind == "dense-both":
        g = _small(hip, 0)[0]
    elif kind == "dense-one":
        g = hip.HipBwt(0)
        for b in _batches(230, False)[0]:
            g.insert_multi(b)
        assert not g.layout_stats()["sparse_now"]
    elif kind.startswith("sparse"):
        g = _forced_sparse(hip, both)
    else:
        img, bwt = fmd_ref.fixture("cov3000")
        g = hip.HipBwt(0)
        assert g.load_fmd(np.frombuffer(img, np.uint8)) == len(bwt)
    cx = _Ctx(kind, g, Q.FM(g.bwt()), both)
    yield cx
    g.close()


def _sets(rec, cnt, max_recs):
    """the records stored for every query as sorted lists of tuples (None for a malformed query)"""
    have = np.minimum(np.where(cnt <= -2, -2 - cnt, np.maximum(cnt, 0)), max_recs)
    return [None if c == -1 else sorted(map(tuple, r[:k].tolist())) for r, k, c in zip(rec, have, cnt)]


def _check(queries, got, want, max_recs, what):
    """stored, rec, cnt of approx_ed_raw against the model's (records, cnt) with nothing cut; the slots behind the records are zeros"""
    stored, rec, cnt = got
    recs, wcnt = want
    assert np.array_equal(cnt, wcnt), (what, np.flatnonzero(cnt != wcnt)[:5].tolist(), cnt[cnt != wcnt][:5].tolist(), wcnt[cnt != wcnt][:5].tolist())
    assert wcnt.max() <= max_recs
    sets = _sets(rec, cnt, max_recs)
    for i, (a, b) in enumerate(zip(sets, recs)):
        assert a == b, (what, i, queries[i][:50].tolist(), a[:4] if a else a, b[:4] if b else b)
    live = np.arange(max_recs)[None, :] < np.maximum(cnt, 0)[:, None]
    assert (rec[~live] == 0).all() and stored == np.maximum(cnt, 0).sum()


def _to_dev(g, arrays):
    ptrs = [g.dev_alloc(max(a.nbytes, 8)) for a in arrays]
    for d, a in zip(ptrs, arrays):
        if a.nbytes:
            g.L.rb2_hip_memcpy(g.h, d, a.ctypes.data, a.nbytes, 0)
    return ptrs


def approx_ed_dev(g, queries, max_ed, min_occ, max_steps, max_recs):
    """approx_ed_dev on buffers filled with FILL: (rec, cnt) as the device left them"""
    qry, off = pack_patterns(queries)
    n = len(off) - 1
    rec = np.full((n, max_recs, 4), FILL, np.int64)
    cnt = np.full(n, FILL, np.int64)
    ptrs = _to_dev(g, (qry, off, rec, cnt))
    try:
        g.approx_ed_dev(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], max_ed, min_occ, max_steps, max_recs)
        for d, a in zip(ptrs[2:], (rec, cnt)):
            g.L.rb2_hip_memcpy(g.h, a.ctypes.data, d, a.nbytes, 1)
    finally:
        for d in ptrs:
            g.dev_free(d)
    return rec, cnt


@pytest.mark.parametrize("max_ed", [0, 1, 2, 3, 4])
def test_parity_with_the_model(idx, max_ed):
    """every query of the set (of the short ones at max_ed 3 and 4), none skipped: the same records as sets and the same counts; no edit
    allowed = backward search; the _dev variant the same, and FILL where it stores nothing; the index is left as it was"""
    cx, g = idx, idx.g
    qs = cx.asked(max_ed)
    recs, wcnt = cx.want(max_ed)
    max_recs = max(int(wcnt.max()), 1)
    bad = len(MALFORMED) - (max_ed > 2)                             # (the one of 8193 symbols is not among the short ones)
    assert wcnt[-bad:].tolist() == [-1] * bad and (wcnt[:-bad] >= 0).all() and wcnt[0] == 0 and wcnt[6] == (4 if max_ed else 0)
    other = sum(r[3] != len(q) for q, rs in zip(qs, recs) if rs for r in rs)
    print("%s max_ed=%d: %d queries, %d records, %d of another length than the query, the most %d" % (cx.kind, max_ed, len(qs), wcnt[wcnt > 0].sum(), other, max_recs))
    assert (other > 0) == (max_ed > 0)
    before, hashes = g.layout_stats(), g.rope_hashes()
    got = g.approx_ed_raw(qs, max_ed, 1, STEPS, max_recs)
    _check(qs, got, (recs, wcnt), max_recs, (cx.kind, max_ed))
    assert g.layout_stats() == before and g.rope_hashes() == hashes, "an approximate search changed the index"
    if max_ed == 0:                                                 # the backward search itself: N matches nothing, a word that is not there gives no record
        lo, hi, m = g.backward_search(cx.queries[:cx.n_well])
        for i, q in enumerate(cx.queries[:cx.n_well]):
            full = len(q) > 0 and m[i] == len(q) and not (q == 5).any()
            assert recs[i] == ([(int(lo[i]), int(hi[i]), 0, len(q))] if full else []), (i, q[:50].tolist())
    rec, cnt = approx_ed_dev(g, qs, max_ed, 1, STEPS, max_recs)
    assert np.array_equal(cnt, wcnt) and _sets(rec, cnt, max_recs) == recs
    live = np.arange(max_recs)[None, :] < np.maximum(cnt, 0)[:, None]
    assert (rec[~live] == FILL).all()


@pytest.mark.parametrize("k", [1, 2])
def test_matches_by_substitutions_are_matches(idx, k):
    """every match of approx at max_mm = k is a match here at max_ed = k, on the same interval with the length of the query and no more
    edits than substitutions"""
    cx, g = idx, idx.g
    qs = cx.queries[:cx.n_well]
    _, mrec, mcnt = g.approx_raw(qs, k, 1, STEPS, 64)
    _, erec, ecnt = g.approx_ed_raw(qs, k, 1, STEPS, max(int(cx.want(k)[1].max()), 1))
    assert (mcnt >= 0).all() and (mcnt <= 64).all() and (ecnt >= mcnt).all() and mcnt.sum() > cx.n_well // 2
    for q, mr, mc, er, ec in zip(qs, mrec, mcnt, erec, ecnt):
        here = {(lo, hi, n): e for lo, hi, e, n in er[:ec].tolist()}
        for lo, hi, n_mm, _ in mr[:mc].tolist():
            assert here.get((lo, hi, len(q)), 9) <= n_mm, (q[:50].tolist(), lo, hi, n_mm)


def test_a_planted_query_finds_its_source(idx):
    """a query made by e edits of a word w of the index, none of them at the ends: (the interval of w, ed <= e, |w|) is among the records
    at max_ed = e"""
    cx, g = idx, idx.g
    seen = {1: 0, 2: 0, 3: 0}
    for e in (1, 2, 3):
        pl = [(i, w) for i, w, k in cx.planted if k == e and (e <= 2 or len(cx.queries[i]) <= SHORT)]
        assert len(pl) >= 6
        stored, rec, cnt = g.approx_ed_raw([cx.queries[i] for i, _ in pl], e, 1, STEPS, 4096)
        lo, hi, m = g.backward_search([w for _, w in pl])
        for j, (i, w) in enumerate(pl):
            assert 1 <= cnt[j] <= 4096 and m[j] == len(w)
            assert any(r[0] == lo[j] and r[1] == hi[j] and r[2] <= e and r[3] == len(w) for r in rec[j, :cnt[j]].tolist()), (cx.kind, e, i, w.tolist(), cx.queries[i].tolist())
            seen[e] += 1
    print(cx.kind, "planted queries that found their source:", seen)


def test_brute_force_and_rows(idx):
    """every tenth query against the windows of the strings, which never look at a BWT; then n = 1, 15, 16, 17 queries (rows of a block, a
    last partial block) and the whole set on four rows of small stacks, each equal to its part of the whole; the _dev variant in two launches"""
    cx, g = idx, idx.g
    recs, wcnt = cx.want(2)
    memo = {}
    for i in range(0, cx.n_well, 10):
        assert ER.brute(cx.strings, cx.queries[i], 2, 1, fm=cx.fm, memo=memo) == recs[i], (cx.kind, i)
    max_recs = max(int(wcnt.max()), 1)
    for n in (1, 15, 16, 17):
        for first in (0, 9):
            qs = cx.queries[first:first + n]
            _check(qs, g.approx_ed_raw(qs, 2, 1, STEPS, max_recs), (recs[first:first + n], wcnt[first:first + n]), max_recs, (cx.kind, n, first))
    # 4 rows for all queries: 4 * the stack of the longest
    lmax = max(len(q) for q in cx.queries[:cx.n_well])
    assert lmax == 8192
    with _Env(RB2_APPROX_SCRATCH=4 * row_bytes(lmax, 2) + 8):
        _check(cx.queries, g.approx_ed_raw(cx.queries, 2, 1, STEPS, max_recs), (recs, wcnt), max_recs, (cx.kind, "4 rows"))
    # the _dev variant does not know the lengths: with this much scratch it takes the queries of up to 6 symbols in one launch and the
    # others on 16 rows with stacks for 8192 symbols in a second one
    assert 16384 * row_bytes(6, 2) <= 16 * row_bytes(8192, 2) < 16384 * row_bytes(7, 2)
    with _Env(RB2_APPROX_SCRATCH=16 * row_bytes(8192, 2)):
        rec, cnt = approx_ed_dev(g, cx.queries, 2, 1, STEPS, max_recs)
    assert np.array_equal(cnt, wcnt) and _sets(rec, cnt, max_recs) == recs


def test_min_occ(idx):
    """min_occ = 2, and one above the median size of the matches at min_occ = 1, which prunes about half of them: the indexes hold
    duplicated strings and repeats, so some matches stay and some go"""
    cx, g = idx, idx.g
    every = cx.want(2)
    sizes = np.array([r[1] - r[0] for rs in every[0] if rs for r in rs])
    big = int(np.median(sizes)) + 1
    assert sizes.min() < big <= sizes.max() and big > 2
    for min_occ in (2, big):
        recs, wcnt = cx.want(2, min_occ)
        assert wcnt[wcnt > 0].sum() == (sizes >= min_occ).sum() > 0
        max_recs = max(int(wcnt.max()), 1)
        _check(cx.queries, g.approx_ed_raw(cx.queries, 2, min_occ, STEPS, max_recs), (recs, wcnt), max_recs, (cx.kind, min_occ))
        assert all(r[1] - r[0] >= min_occ for rs in recs if rs for r in rs)
    assert (sizes >= big).sum() < len(sizes)


def test_step_budget(idx):
    """by properties, not by step counts: an exact substring of L symbols needs more than L - 1 steps (the bound alone takes L), so it ends
    with cnt <= -2; whatever is stored then is a subset of the model's records without repeats; a generous budget gives the model's answer;
    a query whose pieces alone exceed max_ed ends with 0 within L steps"""
    cx, g = idx, idx.g
    recs, wcnt = cx.want(1)
    full = [i for i in range(11, cx.n_well) if 12 <= len(cx.queries[i]) <= 64 and any(r[2] == 0 for r in recs[i])]
    assert len(full) >= 10
    ran_out = 0
    for i in full[:10]:
        q, L = cx.queries[i], len(cx.queries[i])
        for steps in (1, L - 1, 2 * L, 6 * L, 1000 * L):
            stored, rec, cnt = g.approx_ed_raw([q], 1, 1, steps, 8)
            if steps < L:
                assert cnt[0] <= -2
            if cnt[0] <= -2:
                have = _sets(rec, cnt, 8)[0]
                assert len(have) == min(-2 - cnt[0], 8) == stored and len(set(have)) == len(have) and set(have) <= set(recs[i]), (i, steps, cnt[0])
                assert (rec[0, len(have):] == 0).all() and steps < 1000 * L
                ran_out += 1
            else:
                assert cnt[0] == wcnt[i] and (_sets(rec, cnt, 8)[0] == recs[i] or cnt[0] > 8)
        with pytest.raises(StepBudgetExceeded) as e:
            g.approx_ed([q], 1, max_steps=L - 1)
        assert e.value.queries == [0] and len(e.value.results) == 1 and "approx_ed" in str(e.value) and "max_ed" in str(e.value)
    assert ran_out >= 20
    # two strings with twelve symbols of a period of four between them: the pieces alone are too many for max_ed = 0, so the query ends
    # within its L bound steps -- and with a budget of L it never runs out
    q = cx.queries[cx.n_well - 2]
    assert cx.want(0)[1][cx.n_well - 2] == 0
    assert g.approx_ed_raw([q], 0, 1, len(q), 4)[2].tolist() == [0]
    assert g.approx_ed_raw([q], 0, 1, 1, 4)[2].tolist() == [-2]


def test_chunked_staging(idx):
    """RB2_QUERY_CHUNK = 1 and 3, and a max_recs so large that the records of few queries fill a staging chunk: the unchunked result"""
    cx, g = idx, idx.g
    recs, wcnt = cx.want(1)
    max_recs = max(int(wcnt.max()), 1)
    for chunk in (1, 3):
        with _Env(RB2_QUERY_CHUNK=chunk):
            _check(cx.queries, g.approx_ed_raw(cx.queries, 1, 1, STEPS, max_recs), (recs, wcnt), max_recs, (cx.kind, "chunk", chunk))
    big = (256 << 20) // 32 // 3 + 1                                # three queries' records no longer fit 256 MiB: chunks of two
    qs = cx.queries[11:18]
    stored, rec, cnt = g.approx_ed_raw(qs, 1, 1, STEPS, big)
    assert np.array_equal(cnt, wcnt[11:18]) and stored == cnt.sum()
    assert [sorted(map(tuple, r[:k].tolist())) for r, k in zip(rec, cnt)] == recs[11:18] and all((r[k:k + 2] == 0).all() for r, k in zip(rec, cnt))


def test_python_layer(idx):
    """HipBwt.approx_ed: records as sorted tuples, None for a malformed query, text queries"""
    cx, g = idx, idx.g
    recs, wcnt = cx.want(2)
    got = g.approx_ed(cx.queries, 2, max_recs=max(int(wcnt.max()), 1))
    assert got == recs and got[-1] is None and got[0] == []
    i = 12
    txt = "".join("$ACGTN"[c] for c in cx.queries[i])
    assert g.approx_ed([txt], 2, max_recs=max(int(wcnt.max()), 1)) == [recs[i]] and g.approx_ed([], 2) == []


def _truncated(g, q, max_ed, want, caps):
    """with max_recs below the number of matches exactly max_recs records come back, each one of the reference's, none twice, and cnt is
    the whole number; the _dev variant leaves the slots behind them alone"""
    n = len(want)
    stored, rec, cnt = g.approx_ed_raw([q], max_ed, 1, STEPS, n + 3)
    assert cnt[0] == n == stored and sorted(map(tuple, rec[0, :n].tolist())) == want and (rec[0, n:] == 0).all()
    for max_recs in caps:
        assert max_recs < n
        stored, rec, cnt = g.approx_ed_raw([q, q], max_ed, 1, STEPS, max_recs)
        assert cnt.tolist() == [n, n] and stored == 2 * max_recs
        for r in rec:
            have = list(map(tuple, r.tolist()))
            assert len(set(have)) == max_recs and set(have) <= set(want)
        rec, cnt = approx_ed_dev(g, [q], max_ed, 1, STEPS, max_recs)
        have = list(map(tuple, rec[0].tolist()))
        assert cnt[0] == n and len(set(have)) == max_recs and set(have) <= set(want)
        rec, cnt = approx_ed_dev(g, [q], max_ed, 1, STEPS, n + 2)
        assert cnt[0] == n and (rec[0, n:] == FILL).all() and sorted(map(tuple, rec[0, :n].tolist())) == want


def test_truncation_with_many_matches(idx):
    """six symbols within three edits: hundreds of matches; also out of steps with more found than stored"""
    cx, g = idx, idx.g
    q = next(s for s in cx.strings if len(s) >= 12 and not (s == 5).any())[:6]
    want = ER.model(cx.fm, q, 3)
    n = len(want)
    assert n > 40
    _truncated(g, q, 3, want, (1, 7, n - 1))
    stored, rec, cnt = g.approx_ed_raw([q], 3, 1, 30, 5)
    assert cnt[0] <= -2 and stored == min(-2 - cnt[0], 5)
    have = list(map(tuple, rec[0, :stored].tolist()))
    assert len(set(have)) == stored and set(have) <= set(want) and (rec[0, stored:] == 0).all()


@pytest.fixture(scope="module")
def longA(hip):
    img, bwt = fmd_ref.fixture("longA")
    g = hip.HipBwt(0)
    assert g.load_fmd(np.frombuffer(img, np.uint8)) == len(bwt)
    yield g, Q.FM(bwt)
    g.close()


def test_the_homopolymer(longA):
    """three strings of 30000 A and one ACGTN.  A^2000 within two edits: the five words A^1998 .. A^2002 with ed = |len - 2000| on intervals
    of 84000 rows, at the end of a path of 2001 nodes: the deepest stack and the widest intervals in one case.  Then the same with a C at
    position 700 and a G at position 0: two pieces, so the bound alone ends it at max_ed = 1 within its L steps"""
    g, fm = longA
    q = np.ones(2000, np.uint8)
    want = ER.model(fm, q, 2)
    by_len = {n: (lo, hi, e) for lo, hi, e, n in want}
    assert sorted(by_len) == [1998, 1999, 2000, 2001, 2002] and len(want) == 5
    for n, (lo, hi, e) in by_len.items():
        assert e == abs(n - 2000) and hi - lo == 3 * (30000 - n + 1) and (lo, hi) == fm.backward_search(np.ones(n, np.uint8))[:2]
    assert g.approx_ed(["A" * 2000], 2) == [want]
    assert g.approx_ed(["A" * 2000], 0) == [[(by_len[2000][0], by_len[2000][1], 0, 2000)]]
    q[700], q[0] = 2, 3
    assert ER.model(fm, q, 1) == []
    assert g.approx_ed_raw([q], 1, 1, 2000, 8)[2].tolist() == [0]    # the bound alone ends it, within its L steps
    want = ER.model(fm, q, 2)
    assert len(want) >= 2 and {r[2] for r in want} == {2}
    assert g.approx_ed([q], 2, max_steps=4 * 2000) == [want]
    assert g.approx_ed_raw([q], 2, 1, 2000, 8)[2].tolist() == [-2]


def test_lifecycle(hip):
    """a suffix array built before the search stays valid and locates the matches: the text of len symbols at every place has the
    distance ed to the query, by the plain dynamic programme; after a lazy insert the next call sees the new index; an empty index"""
    g = hip.HipBwt(0)
    assert g.approx_ed_raw([[1, 2], []], 2)[2].tolist() == [0, 0]
    a, b = H.repetitive_reads(200, seed=61, max_len=40), H.repetitive_reads(150, seed=62, max_len=40)
    g.insert_multi(H.encode_batch(a, True, True))
    sa = Q.inserted_strings(a, True, True)
    g.build_ssa(3)
    inf, hashes, lay = g.ssa_info(), g.rope_hashes(), g.layout_stats()
    rng = np.random.RandomState(5)
    qs = [plant(rng, s[:20], [(("s", "d", "i")[k % 3], 5), (("d", "i", "s")[k % 3], 13)]) for k, s in enumerate(sa) if len(s) >= 20 and not (s == 5).any()][:30]
    res = g.approx_ed(qs, 2, max_recs=256)
    assert g.ssa_info() == inf and inf["valid"] and g.rope_hashes() == hashes and g.layout_stats() == lay
    fm = Q.FM(g.bwt())
    places = other = 0
    for q, rs in zip(qs, res):
        assert rs == ER.model(fm, q, 2) and len(rs) >= 1
        hits = g.locate([(lo, hi) for lo, hi, _, _ in rs], max_hits=max(hi - lo for lo, hi, _, _ in rs))
        for (lo, hi, e, n), h in zip(rs, hits):
            assert len(h) == hi - lo
            texts = {bytes(sa[s][p:p + n]) for s, p in h.tolist()}   # input order: string s is the s-th inserted
            assert len(texts) == 1 and all(p + n <= len(sa[s]) for s, p in h.tolist())
            S = np.frombuffer(texts.pop(), np.uint8)
            assert len(S) == n and ER.ed(S, q) == e
            places += len(h); other += n != len(q)
    assert places > 100 and other > 10
    g.set_lazy(1)
    g.insert_multi(H.encode_batch(b, True, True))                   # (lazy: the rounds may still be queued when the query begins)
    fm2 = Q.FM(g.bwt())
    res2 = g.approx_ed(qs, 2, max_recs=256)
    assert [ER.model(fm2, q, 2) for q in qs] == res2 and res2 != res
    assert not g.ssa_info()["valid"]
    g.close()


@pytest.mark.parametrize("stage,what", [("ed-1", "max_ed"), ("ed5", "max_ed"), ("minocc0", "min_occ"), ("steps0", "max_steps"), ("recs0", "max_recs"),
                                        ("dev-ed5", "max_ed"), ("dev-recs0", "max_recs"), ("shard", "sharded index")])
def test_fatal_parameters(hip, stage, what):
    """host-side argument checks that end the process before any kernel is launched: each leaves through the fatal handler with the
    function's name and the parameter in the message; n = 0 with bad parameters returns"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "approx_ed_child.py"), stage], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 7 and "NOT FATAL" not in out, (p.returncode, out, p.stderr.decode()[-1500:])
    assert "approx_ed ok" in out and "empty ok" in out and "handler: [rb2_hip] approx_ed" in out and what in out, out
