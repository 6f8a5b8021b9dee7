"""GPU tests of the approximate search (include/rb2_hip.h: rb2_hip_approx[_dev]; kernel k_approx in csrc/rb2_query.h): the records and
counts the device reports must equal the backtracking model on the BWT of the same index (tests/approx_ref.py, which tests/test_approx_ref.py
holds against brute force), and for a part of the queries the brute force over the strings itself.  The indexes are small -- the Python
references are the limit, and what can go wrong is control flow and addressing: the stacks in device memory, the record slots, the rows
of a launch -- not volume."""
import os
import subprocess
import sys

import numpy as np
import pytest

import approx_ref as AR
import fmd_ref
import helpers as H
import locate_ref as LR
import query_ref as Q
from ropebwt2_amd.hipbwt import StepBudgetExceeded, pack_patterns, unpack_subs
from test_locate_gpu import _small
from test_query_gpu import _Env, _batches
from test_query_layouts_gpu import FORCED

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILL = -7                                                            # what the device variant must leave in the slots it does not write
MALFORMED = [[1, 0], [0], [1, 0, 2], [7, 1], [3, 6], [1] * 8193]
STEPS = 1 << 20                                                      # a budget none of these queries uses up


def _mutate(rng, s, k, ends):
    """s with k substitutions at distinct positions, the first two of them at the ends when asked for"""
    t = s.copy()
    at = rng.choice(len(s), size=min(k, len(s)), replace=False)
    if ends and len(s) >= 2:
        at[:2] = (0, len(s) - 1)[:len(at[:2])]
        at = np.unique(at)
    for p in at:
        t[p] = 1 + (t[p] + rng.randint(3)) % 4 if t[p] < 5 else rng.randint(1, 5)
    return t


class _Ctx:
    """an index, its model, its strings by id (read back with extract), the queries, and the model's answers, computed once per
    (max_mm, min_occ)"""
    def __init__(self, kind, g, fm, both, nq=28):
        self.kind, self.g, self.fm, self.both = kind, g, fm, both
        n = int(fm.C[1])
        lens = LR.suffix_array(fm)[2]
        self.strings = g.extract(np.arange(n), int(lens.max()))
        rng = np.random.RandomState(n)
        clean = [s for s in self.strings if len(s) >= 12 and not (s == 5).any()]
        qs = [np.array(q, np.uint8) for q in ([1], [4], [2, 3], [1, 1], [5], [5, 5], [])]         # lengths 1 and 2, N alone, the empty query
        for i in range(nq):
            s = clean[rng.randint(len(clean))]
            a = rng.randint(len(s) - 11)
            w = s[a:a + rng.randint(12, len(s) - a + 1)]
            qs.append(s.copy() if i % 4 == 0 else w.copy())                                       # the full length of a string; a substring
            for k in (1, 2, 3, 4):                                                                 # planted substitutions, at the ends too
                qs.append(_mutate(rng, w, k, (i + k) % 2 == 0))
            for at in (0, len(w) - 1, len(w) // 2):                                               # N at either end and in the middle
                t = w.copy(); t[at] = 5; qs.append(t)
            t = _mutate(rng, w, 2, False); t[rng.randint(len(t))] = 5; qs.append(t)
        longest = max(self.strings, key=len)
        qs.append(np.concatenate([longest, longest[:3]]).astype(np.uint8))                         # longer than every string
        qs.append(np.concatenate([clean[0], [1, 2, 3, 4] * 3, clean[1]]).astype(np.uint8))         # ... and with pieces in it
        self.n_well = len(qs)
        self.queries = qs + [np.array(q, np.uint8) for q in MALFORMED]
        self.memo = {}

    def want(self, max_mm, min_occ=1):
        key = (max_mm, min_occ)
        if key not in self.memo:
            self.memo[key] = AR.approx_raw(self.fm, self.queries, max_mm, min_occ)
        return self.memo[key]


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


def _check(cx, queries, got, want, max_recs, what):
    """stored, rec, cnt of approx_raw against the model's (records, cnt) with nothing cut; the slots behind the records are zeros"""
    stored, rec, cnt = got
    recs, wcnt = want
    assert np.array_equal(cnt, wcnt), (what, np.flatnonzero(cnt != wcnt)[:5].tolist(), cnt[cnt != wcnt][:5].tolist(), wcnt[cnt != wcnt][:5].tolist())
    assert wcnt.max() <= max_recs
    sets = _sets(rec, cnt, max_recs)
    for i, (a, b) in enumerate(zip(sets, recs)):
        assert a == b, (what, i, queries[i].tolist(), a[:4] if a else a, b[:4] if b else b)
    live = np.arange(max_recs)[None, :] < np.maximum(cnt, 0)[:, None]
    assert (rec[~live] == 0).all() and stored == np.maximum(cnt, 0).sum()


def _to_dev(g, arrays):
    ptrs = [g.dev_alloc(max(a.nbytes, 8)) for a in arrays]
    for d, a in zip(ptrs, arrays):
        if a.nbytes:
            g.L.rb2_hip_memcpy(g.h, d, a.ctypes.data, a.nbytes, 0)
    return ptrs


def approx_dev(g, queries, max_mm, min_occ, max_steps, max_recs):
    """approx_dev on buffers filled with FILL: (rec, cnt) as the device left them"""
    qry, off = pack_patterns(queries)
    n = len(off) - 1
    rec = np.full((n, max_recs, 4), FILL, np.int64)
    cnt = np.full(n, FILL, np.int64)
    ptrs = _to_dev(g, (qry, off, rec, cnt))
    try:
        g.approx_dev(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], max_mm, min_occ, max_steps, max_recs)
        for d, a in zip(ptrs[2:], (rec, cnt)):
            g.L.rb2_hip_memcpy(g.h, a.ctypes.data, d, a.nbytes, 1)
    finally:
        for d in ptrs:
            g.dev_free(d)
    return rec, cnt


@pytest.mark.parametrize("max_mm", [0, 1, 2, 3, 4])
def test_parity_with_the_model(idx, max_mm):
    """every query of the set, none skipped: the same records as sets and the same counts; no substitution allowed = backward search; a
    planted query needs exactly what was planted or less; the _dev variant the same, and FILL where it stores nothing"""
    cx, g = idx, idx.g
    recs, wcnt = cx.want(max_mm)
    max_recs = max(int(wcnt.max()), 1)
    nq = len(cx.queries)
    assert wcnt[cx.n_well:].tolist() == [-1] * len(MALFORMED) and wcnt[6] == 0 and (wcnt[4:6] == 0).all() == (max_mm == 0)
    print("%s max_mm=%d: %d queries, %d records, the most %d" % (cx.kind, max_mm, nq, wcnt[wcnt > 0].sum(), max_recs))
    before, hashes = g.layout_stats(), g.rope_hashes()
    got = g.approx_raw(cx.queries, max_mm, 1, STEPS, max_recs)
    _check(cx, cx.queries, got, (recs, wcnt), max_recs, (cx.kind, max_mm))
    assert g.layout_stats() == before and g.rope_hashes() == hashes, "an approximate search changed the index"
    if max_mm == 0:                                                 # the backward search itself: N matches nothing, a word that is not there gives no record
        lo, hi, m = g.backward_search(cx.queries[:cx.n_well])
        for i, q in enumerate(cx.queries[:cx.n_well]):
            full = len(q) > 0 and m[i] == len(q) and not (q == 5).any()
            assert recs[i] == ([(int(lo[i]), int(hi[i]), 0, 0)] if full else []), (i, q.tolist())
    # exactly max_mm are needed by some query, and max_mm + 1 by some other (no record): the planted ones
    best = np.array([min((r[2] for r in rs), default=9) if rs is not None else -1 for rs in cx.want(4)[0]])
    assert (best == max_mm).any() and ((best == max_mm + 1).any() or max_mm == 4)
    for i in np.flatnonzero(best >= 0):
        assert (len(recs[i]) > 0) == (best[i] <= max_mm)
    # the _dev variant: the same, and what it does not store keeps the fill
    rec, cnt = approx_dev(g, cx.queries, max_mm, 1, STEPS, max_recs)
    assert np.array_equal(cnt, wcnt) and _sets(rec, cnt, max_recs) == recs
    live = np.arange(max_recs)[None, :] < np.maximum(cnt, 0)[:, None]
    assert (rec[~live] == FILL).all()


def test_brute_force_and_rows(idx):
    """a part of the queries against the windows of the strings, which never look at a BWT; then n = 1, 15, 16, 17 queries (rows of a
    block, a last partial block) and the whole set on few rows of small stacks, each equal to its part of the whole"""
    cx, g = idx, idx.g
    recs, wcnt = cx.want(2)
    memo = {}
    for i in range(0, cx.n_well, 10):
        assert AR.brute(cx.strings, cx.queries[i], 2, 1, fm=cx.fm, memo=memo) == recs[i], (cx.kind, i)
    max_recs = max(int(wcnt.max()), 1)
    for n in (1, 15, 16, 17):
        for first in (0, 7):
            qs = cx.queries[first:first + n]
            _check(cx, qs, g.approx_raw(qs, 2, 1, STEPS, max_recs), (recs[first:first + n], wcnt[first:first + n]), max_recs, (cx.kind, n, first))
    # 4 rows for all queries: 4 * the stack of the longest
    lmax = max(len(q) for q in cx.queries[:cx.n_well])
    with _Env(RB2_APPROX_SCRATCH=4 * (64 * lmax + 2 * ((lmax + 7) // 8 * 8)) + 8):
        _check(cx, cx.queries, g.approx_raw(cx.queries, 2, 1, STEPS, max_recs), (recs, wcnt), max_recs, (cx.kind, "4 rows"))
    # the _dev variant does not know the lengths: with this much scratch it takes the queries of up to 8 symbols in one launch and the
    # others on 16 rows with stacks for 8192 symbols in a second one
    with _Env(RB2_APPROX_SCRATCH=16 * 66 * 8192):
        rec, cnt = approx_dev(g, cx.queries, 2, 1, STEPS, max_recs)
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
        _check(cx, cx.queries, g.approx_raw(cx.queries, 2, min_occ, STEPS, max_recs), (recs, wcnt), max_recs, (cx.kind, min_occ))
        assert all(r[1] - r[0] >= min_occ for rs in recs if rs for r in rs)
    assert (sizes >= big).sum() < len(sizes)


def test_step_budget(idx):
    """an exact substring of L symbols needs at least L steps: with L - 1 the query ends with cnt <= -2 and what it stored is true; a query
    whose pieces alone exceed max_mm ends with 0 within L steps; a generous budget gives the model's answer"""
    cx, g = idx, idx.g
    recs, wcnt = cx.want(1)
    full = [i for i in range(7, cx.n_well) if len(cx.queries[i]) >= 12 and any(r[2] == 0 for r in recs[i])]
    assert len(full) >= 10
    for i in full[:10]:
        q, L = cx.queries[i], len(cx.queries[i])
        for steps in (1, L - 1, 2 * L, 5 * L):
            stored, rec, cnt = g.approx_raw([q], 1, 1, steps, 8)
            if steps < L:
                assert cnt[0] <= -2
            if cnt[0] <= -2:
                have = _sets(rec, cnt, 8)[0]
                assert len(have) == min(-2 - cnt[0], 8) == stored and len(set(have)) == len(have) and set(have) <= set(recs[i]), (i, steps, cnt[0])
                assert (rec[0, len(have):] == 0).all()
            else:
                assert cnt[0] == wcnt[i] and _sets(rec, cnt, 8)[0] == recs[i][:8] or cnt[0] > 8
        with pytest.raises(StepBudgetExceeded) as e:
            g.approx([q], 1, max_steps=L - 1)
        assert e.value.queries == [0] and len(e.value.results) == 1
    # the last query of the set: two strings with twelve symbols of a period of four between them; its pieces alone are too many for
    # max_mm = 0, so it ends within its L bound steps -- and with a budget of L it never runs out
    q = cx.queries[cx.n_well - 1]
    D, pieces = AR.bound(lambda w: cx.fm.count(np.array(w, np.uint8)) if len(w) else cx.fm.N, q)
    assert D[-1] >= 1 and cx.want(0)[1][cx.n_well - 1] == 0
    assert g.approx_raw([q], 0, 1, len(q), 4)[2].tolist() == [0]
    assert g.approx_raw([q], 0, 1, 1, 4)[2].tolist() == [-2]


def test_chunked_staging(idx):
    """RB2_QUERY_CHUNK = 1 and 3, and a max_recs so large that the records of few queries fill a staging chunk: the unchunked result"""
    cx, g = idx, idx.g
    recs, wcnt = cx.want(1)
    max_recs = max(int(wcnt.max()), 1)
    for chunk in (1, 3):
        with _Env(RB2_QUERY_CHUNK=chunk):
            _check(cx, cx.queries, g.approx_raw(cx.queries, 1, 1, STEPS, max_recs), (recs, wcnt), max_recs, (cx.kind, "chunk", chunk))
    big = (256 << 20) // 32 // 3 + 1                                # three queries' records no longer fit 256 MiB: chunks of two
    qs = cx.queries[7:14]
    stored, rec, cnt = g.approx_raw(qs, 1, 1, STEPS, big)
    assert np.array_equal(cnt, wcnt[7:14]) and stored == cnt.sum()
    assert [sorted(map(tuple, r[:k].tolist())) for r, k in zip(rec, cnt)] == recs[7:14] and all((r[k:k + 2] == 0).all() for r, k in zip(rec, cnt))


def test_python_layer(idx):
    """HipBwt.approx: records decoded and sorted, None for a malformed query, text queries"""
    cx, g = idx, idx.g
    recs, wcnt = cx.want(2)
    got = g.approx(cx.queries, 2, max_recs=max(int(wcnt.max()), 1))
    assert len(got) == len(cx.queries)
    for a, b in zip(got, recs):
        assert a == (None if b is None else [(lo, hi, mm, AR.unpack_subs(sb)) for lo, hi, mm, sb in b])
    i = cx.n_well - 3
    txt = "".join("$ACGTN"[c] for c in cx.queries[i])
    assert g.approx([txt], 2) == [got[i][:64]] and g.approx([], 2) == []
    assert unpack_subs(AR.pack_subs([(3, 1), (9, 2)])) == [(9, 2), (3, 1)]


@pytest.fixture(scope="module")
def longA(hip):
    img, bwt = fmd_ref.fixture("longA")
    g = hip.HipBwt(0)
    assert g.load_fmd(np.frombuffer(img, np.uint8)) == len(bwt)
    yield g, Q.FM(bwt)
    g.close()


def _truncated(g, q, max_mm, want, caps):
    """with max_recs below the number of matches exactly max_recs records come back, each one of the reference's, none twice, and cnt is
    the whole number; the _dev variant leaves the slots behind them alone"""
    n = len(want)
    stored, rec, cnt = g.approx_raw([q], max_mm, 1, STEPS, n + 3)
    assert cnt[0] == n == stored and sorted(map(tuple, rec[0, :n].tolist())) == want and (rec[0, n:] == 0).all()
    for max_recs in caps:
        assert max_recs < n
        stored, rec, cnt = g.approx_raw([q, q], max_mm, 1, STEPS, max_recs)
        assert cnt.tolist() == [n, n] and stored == 2 * max_recs
        for r in rec:
            have = list(map(tuple, r.tolist()))
            assert len(set(have)) == max_recs and set(have) <= set(want)
        rec, cnt = approx_dev(g, [q], max_mm, 1, STEPS, max_recs)
        have = list(map(tuple, rec[0].tolist()))
        assert cnt[0] == n and len(set(have)) == max_recs and set(have) <= set(want)
        rec, cnt = approx_dev(g, [q], max_mm, 1, STEPS, n + 2)
        assert cnt[0] == n and (rec[0, n:] == FILL).all() and sorted(map(tuple, rec[0, :n].tolist())) == want


def test_truncation_on_the_homopolymer(longA):
    """three strings of 30000 A and one ACGTN: the queries with the most matches there are A within one substitution (A C G T) and AA
    within two (AA AC CG GT), four each.  Then what the fixture is hard at: intervals of 90000 rows and a stack of 2000 positions"""
    g, fm = longA
    for q, max_mm in (([1], 1), ([1, 1], 2)):
        want = AR.model(fm, q, max_mm)
        assert len(want) == 4
        _truncated(g, np.array(q, np.uint8), max_mm, want, (1, 2, 3))
    q = np.ones(2000, np.uint8)
    want = AR.model(fm, q, 2)
    assert len(want) == 1 and want[0][1] - want[0][0] == 3 * 28001
    assert g.approx(["A" * 2000], 2) == [[(want[0][0], want[0][1], 0, [])]]
    q[700], q[0] = 2, 3                                             # two pieces, [700, 1999] and [0, 699]: two substitutions, and none less
    D, pieces = AR.bound(lambda w: fm.count(np.array(w, np.uint8)) if len(w) else fm.N, q)
    assert pieces == [(700, 1999), (0, 699)] and D[-1] == 2 and D[698] == 0 and D[699] == 1
    got = g.approx([q], 2, max_steps=3 * 2000)
    assert got == [[(want[0][0], want[0][1], 2, [(700, 1), (0, 1)])]] == [[(lo, hi, mm, AR.unpack_subs(sb)) for lo, hi, mm, sb in AR.model(fm, q, 2)]]
    assert g.approx_raw([q], 1, 1, 2000, 4)[2].tolist() == [0]      # the bound alone ends it, within its L steps
    assert g.approx_raw([q], 2, 1, 2000, 4)[2].tolist() == [-2]


def test_truncation_with_many_matches(idx):
    """six symbols within three substitutions: some hundreds of matches; also out of steps with more found than stored"""
    cx, g = idx, idx.g
    q = next(s for s in cx.strings if len(s) >= 12 and not (s == 5).any())[:6]
    want = AR.model(cx.fm, q, 3)
    n = len(want)
    assert n > 40
    _truncated(g, q, 3, want, (1, 7, n - 1))
    stored, rec, cnt = g.approx_raw([q], 3, 1, 30, 5)
    assert cnt[0] <= -2 and stored == min(-2 - cnt[0], 5)
    have = list(map(tuple, rec[0, :stored].tolist()))
    assert len(set(have)) == stored and set(have) <= set(want) and (rec[0, stored:] == 0).all()


def test_lifecycle(hip):
    """a suffix array built before the search stays valid and locates the matches: the text at every place differs from the query exactly
    at subs; after an insert the next call sees the new index; an empty index"""
    g = hip.HipBwt(0)
    assert g.approx_raw([[1, 2], []], 2)[2].tolist() == [0, 0]
    a, b = H.repetitive_reads(200, seed=61, max_len=40), H.repetitive_reads(150, seed=62, max_len=40)
    g.insert_multi(H.encode_batch(a, True, True))
    sa = Q.inserted_strings(a, True, True)
    g.build_ssa(3)
    inf, hashes, lay = g.ssa_info(), g.rope_hashes(), g.layout_stats()
    rng = np.random.RandomState(5)
    qs = [_mutate(rng, s[:20], 2, k % 2 == 0) for k, s in enumerate(sa) if len(s) >= 20 and not (s == 5).any()][:40]
    res = g.approx(qs, 2, max_recs=256)
    assert g.ssa_info() == inf and inf["valid"] and g.rope_hashes() == hashes and g.layout_stats() == lay
    fm = Q.FM(g.bwt())
    places = 0
    for q, rs in zip(qs, res):
        assert rs == [(lo, hi, mm, AR.unpack_subs(sb)) for lo, hi, mm, sb in AR.model(fm, q, 2)] and len(rs) >= 1
        hits = g.locate([(lo, hi) for lo, hi, _, _ in rs], max_hits=max(hi - lo for lo, hi, _, _ in rs))
        for (lo, hi, mm, subs), h in zip(rs, hits):
            assert len(h) == hi - lo and mm == len(subs)
            S = q.copy()
            for p, c in subs:
                S[p] = c
            for s, p in h.tolist():                                  # input order: string s is the s-th inserted
                assert np.array_equal(sa[s][p:p + len(q)], S) and np.flatnonzero(sa[s][p:p + len(q)] != q).tolist() == sorted(p for p, _ in subs)
                places += 1
    assert places > 100
    g.set_lazy(1)
    g.insert_multi(H.encode_batch(b, True, True))                   # (lazy: the rounds may still be queued when the query begins)
    fm2 = Q.FM(g.bwt())
    res2 = g.approx(qs, 2, max_recs=256)
    assert [[(lo, hi, mm, AR.unpack_subs(sb)) for lo, hi, mm, sb in AR.model(fm2, q, 2)] for q in qs] == res2 and res2 != res
    assert not g.ssa_info()["valid"]
    g.close()


@pytest.mark.parametrize("stage,what", [("mm-1", "max_mm"), ("mm5", "max_mm"), ("minocc0", "min_occ"), ("steps0", "max_steps"), ("recs0", "max_recs"),
                                        ("dev-mm5", "max_mm"), ("dev-recs0", "max_recs"), ("shard", "sharded index")])
def test_fatal_parameters(hip, stage, what):
    """each leaves through the fatal handler with the function's name and the parameter in the message; n = 0 with bad parameters returns"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "approx_child.py"), stage], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 7 and "NOT FATAL" not in out, (p.returncode, out, p.stderr.decode()[-1500:])
    assert "approx ok" in out and "empty ok" in out and "handler: [rb2_hip] approx" in out and what in out, out
