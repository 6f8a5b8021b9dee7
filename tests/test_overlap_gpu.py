"""GPU tests of the suffix-prefix overlap queries (include/rb2_hip.h: rb2_hip_overlap[_dev], rb2_hip_string_ids[_dev]; kernels k_overlap,
k_string_ids in csrc/rb2_query.h): every record and every id the device reports must equal the numpy model (tests/overlap_ref.py) on the
BWT of the same index, and through HipBwt.overlaps the brute force over string slices that never looks at a BWT.  The indexes are those
of test_locate_gpu.py: what can go wrong is addressing -- the `$` counts of both layouts, the record slots, head[] -- not volume."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fmd_ref
import locate_ref as LR
import overlap_ref as OR
import query_ref as Q
from ropebwt2_amd.hipbwt import pack_patterns
from test_locate_gpu import _small
from test_query_layouts_gpu import _Models, _build_dense, _build_sparse

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILL = -7                                                            # what the device variants must leave in the slots they do not write
MALFORMED = [[1, 0], [0], [1, 0, 2], [7, 1], [3, 6]]
BRUTE = 32                                                           # queries per index that go through overlaps() and the brute force


@pytest.fixture(scope="module")
def models():
    ms = _Models()
    yield ms
    ms.made.clear()


class _Ctx:
    """an index, its model, its strings by id (read back with extract) and the queries: every string, then the made-up ones"""
    def __init__(self, kind, g, fm):
        self.kind, self.g, self.fm = kind, g, fm
        self.n = n = int(fm.C[1])
        lens = LR.suffix_array(fm)[2]
        self.strings = g.extract(np.arange(n), int(lens.max()))
        assert [len(s) for s in self.strings] == lens.tolist()
        rng = np.random.RandomState(n)
        more = []
        for k in rng.choice(n, size=min(n, 150), replace=False):
            s = self.strings[k]
            if len(s) < 4:
                continue
            more += [s[:len(s) // 2].copy(), s[1:].copy(), s[len(s) // 3:len(s) - 1].copy()]                  # truncated
            t = s.copy(); t[rng.randint(len(s))] = 1 + (t[0] + rng.randint(3)) % 4; more.append(t)           # mutated
            t = s.copy(); t[rng.randint(1, len(s) - 1)] = 5; more.append(t)                                   # an N inside
            t = s.copy(); t[-1] = 5; more.append(t)                                                           # an N at the end: nothing
        more += [np.array(q, np.uint8) for q in ([5], [1, 5], [5, 2], [])] + [np.array(q, np.uint8) for q in MALFORMED]
        self.queries = list(self.strings) + more
        self.maxlen = max(len(q) for q in self.queries)
        self.memo = {}

    def want(self, min_ovlp, max_recs=None):
        """the model's overlap_raw of all queries (computed once); max_recs = None: as many as nothing is cut with"""
        key = (min_ovlp, max_recs)
        if key not in self.memo:
            self.memo[key] = OR.overlap_raw(self.fm, self.queries, min_ovlp, max_recs or max(self.maxlen - min_ovlp + 1, 1))
        return self.memo[key]


@pytest.fixture(scope="module", params=["dense-io", "dense-rclo", "D", "S", "fmd"])
def idx(request, hip, models):
    """the five indexes of test_locate_gpu.py: dense in input order and in RCLO, layout D (every piece longer than two superblocks),
    layout S (sparse, split leaves), and one loaded from a file the reference wrote (one strand, RLO)"""
    kind = request.param
    if kind.startswith("dense"):
        g, fm, _ = _small(hip, 0 if kind == "dense-io" else 2)
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
    cx = _Ctx(kind, g, fm)
    # the caps: most strings of the index overlap others at two or more lengths, and some range names two or more strings
    _, rec, cnt = cx.want(1)
    own = cnt[:cx.n]
    print("%s: %d strings, %d queries, %d records, %d strings with records at two or more lengths" % (kind, cx.n, len(cx.queries), cnt[cnt > 0].sum(), (own >= 2).sum()))
    assert 2 * (own >= 2).sum() > cx.n, (kind, (own >= 2).sum(), cx.n)
    assert ((rec[:, :, 2] - rec[:, :, 1]) >= 2).any()
    yield cx
    g.close()


def _to_dev(g, arrays):
    ptrs = [g.dev_alloc(max(a.nbytes, 8)) for a in arrays]
    for d, a in zip(ptrs, arrays):
        if a.nbytes:
            g.L.rb2_hip_memcpy(g.h, d, a.ctypes.data, a.nbytes, 0)
    return ptrs


def _from_dev(g, ptrs, arrays):
    for d, a in zip(ptrs, arrays):
        if a.nbytes:
            g.L.rb2_hip_memcpy(g.h, a.ctypes.data, d, a.nbytes, 1)


def overlap_dev(g, queries, min_ovlp, max_recs):
    """overlap_dev on buffers filled with FILL: (rec, cnt) as the device left them"""
    qry, off = pack_patterns(queries)
    n = len(off) - 1
    rec = np.full((n, max_recs, 3), FILL, np.int64)
    cnt = np.full(n, FILL, np.int64)
    ptrs = _to_dev(g, (qry, off, rec, cnt))
    try:
        g.overlap_dev(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], min_ovlp, max_recs)
        _from_dev(g, ptrs[2:], (rec, cnt))
    finally:
        for d in ptrs:
            g.dev_free(d)
    return rec, cnt


def string_ids_dev(g, ranges, max_hits):
    """string_ids_dev on buffers filled with FILL: (ids, cnt) as the device left them"""
    zv = np.ascontiguousarray(np.asarray(ranges, np.int64).reshape(-1, 2))
    n = len(zv)
    ids = np.full((n, max_hits), FILL, np.int64)
    cnt = np.full(n, FILL, np.int64)
    ptrs = _to_dev(g, (zv, ids, cnt))
    try:
        g.string_ids_dev(n, ptrs[0], ptrs[1], ptrs[2], max_hits)
        _from_dev(g, ptrs[1:], (ids, cnt))
    finally:
        for d in ptrs:
            g.dev_free(d)
    return ids, cnt


def _first_bad(cx, got, want):
    bad = np.flatnonzero((got[1] != want[1]).reshape(len(want[2]), -1).any(1) | (got[2] != want[2]))
    i = bad[0]
    k = max(int(want[2][i]), int(got[2][i]), 1)
    return "%s: %d of %d queries differ; first: query %d %s\n got cnt %d %s\nwant cnt %d %s" % (
        cx.kind, len(bad), len(want[2]), i, cx.queries[i].tolist(), got[2][i], got[1][i, :k].tolist(), want[2][i], want[1][i, :k].tolist())


def _same(cx, got, want):
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1]), _first_bad(cx, got, want)
    assert got[0] == want[0]


def _live(cnt, width):
    return np.arange(width)[None, :] < np.minimum(np.maximum(cnt, 0), width)[:, None]


@pytest.mark.parametrize("min_ovlp", [1, 3, 10 ** 6])
def test_overlap_matches_model(idx, min_ovlp):
    """every string of the index, truncated and mutated copies, N-bearing, empty and malformed queries, nothing cut"""
    cx, g, fm = idx, idx.g, idx.fm
    want = cx.want(min_ovlp)
    max_recs = want[1].shape[1]
    nq = len(cx.queries)
    assert want[2][-len(MALFORMED):].tolist() == [-1] * len(MALFORMED) and want[2][nq - len(MALFORMED) - 1] == 0 and (want[2] <= max_recs).all()
    if min_ovlp == 10 ** 6:
        assert want[0] == 0
    else:
        lens = np.array([len(s) for s in cx.strings], np.int64)      # a string without N finds itself: its last record is its full length
        ks = np.flatnonzero((lens >= min_ovlp) & np.array([not (s == 5).any() for s in cx.strings]))
        assert len(ks) > cx.n // 2 and (want[2][ks] >= 1).all() and (want[1][ks, want[2][ks] - 1, 0] == lens[ks]).all()
    before = g.layout_stats()
    _same(cx, g.overlap_raw(cx.queries, min_ovlp, max_recs), want)
    rec, cnt = overlap_dev(g, cx.queries, min_ovlp, max_recs)
    live = _live(want[2], max_recs)
    assert np.array_equal(cnt, want[2]) and np.array_equal(rec[live], want[1][live]) and (rec[~live] == FILL).all()
    assert g.layout_stats() == before, "an overlap query changed the layout"
    if cx.kind != "fmd" and min_ovlp == 1:                          # both strands: the strings that start with P are the strings that end in revcomp(P)
        rng = np.random.RandomState(7)
        who = rng.choice(np.flatnonzero(want[2] > 0), size=200)
        ks = [rng.randint(want[2][i]) for i in who]
        pats = [np.concatenate([Q.revcomp(cx.queries[i][len(cx.queries[i]) - want[1][i, k, 0]:]), [0]]).astype(np.uint8) for i, k in zip(who, ks)]
        sizes = np.array([want[1][i, k, 2] - want[1][i, k, 1] for i, k in zip(who, ks)])
        assert len(set(sizes.tolist())) > 3
        assert np.array_equal(g.count(pats), sizes)


@pytest.mark.parametrize("max_recs", [1, 3])
def test_truncated_records(idx, max_recs):
    cx, g = idx, idx.g
    for min_ovlp in (1, 3):
        want = OR.overlap_raw(cx.fm, cx.queries, min_ovlp, max_recs)
        assert (want[2] > max_recs).sum() > 0, "no query is truncated"
        full = cx.want(min_ovlp)
        assert np.array_equal(want[2], full[2]) and np.array_equal(want[1], full[1][:, :max_recs])        # the first records, all of them counted
        _same(cx, g.overlap_raw(cx.queries, min_ovlp, max_recs), want)
        rec, cnt = overlap_dev(g, cx.queries, min_ovlp, max_recs)
        live = _live(want[2], max_recs)
        assert np.array_equal(cnt, want[2]) and np.array_equal(rec[live], want[1][live]) and (rec[~live] == FILL).all()


@pytest.mark.parametrize("s", [0, 30])
def test_string_ids(idx, s):
    """every single rank, all of them at once, the empty range at the end, malformed ranges; cut at 1 and 3; the same at every sampling
    step: head[] does not depend on it (at 30 only row 0 is a sample)"""
    cx, g, fm, n = idx, idx.g, idx.fm, idx.n
    hd = OR.head(fm)
    before = g.layout_stats()
    g.build_ssa(s)
    q = np.arange(n, dtype=np.int64)
    stored, ids, cnt = g.string_ids_raw(np.stack([q, q + 1], 1), 1)
    assert stored == n and (cnt == 1).all() and np.array_equal(ids[:, 0], hd)
    stored, ids, cnt = g.string_ids_raw([(0, n), (n, n)], n)
    assert stored == n and cnt.tolist() == [n, 0] and np.array_equal(ids[0], hd) and (ids[1] == 0).all()
    ids, cnt = string_ids_dev(g, [(0, n), (n, n)], n)
    assert cnt.tolist() == [n, 0] and np.array_equal(ids[0], hd) and (ids[1] == FILL).all()
    zv = [(7, 7), (n, n), (11, 12), (n - 1, n), (100, 103), (0, 4), (20, n - 20), (-1, 2), (0, n + 1), (5, 4), (n - 3, n)]
    for max_hits in (1, 3):
        want = OR.string_ids_raw(fm, zv, max_hits)
        assert want[2].tolist() == [0, 0, 1, 1, 3, 4, n - 40, -1, -1, -1, 3] and (want[2] > max_hits).sum() >= 2
        got = g.string_ids_raw(zv, max_hits)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        ids, cnt = string_ids_dev(g, zv, max_hits)
        live = _live(want[2], max_hits)
        assert np.array_equal(cnt, want[2]) and np.array_equal(ids[live], want[1][live]) and (ids[~live] == FILL).all()
    assert g.string_ids_raw([], 4)[0] == 0
    assert g.layout_stats() == before, "building the array or a gather changed the layout"


def _brute(S, lens, q, min_ovlp):
    """overlap_ref.brute_overlaps on the strings as a padded matrix: the strings that begin with a suffix, one symbol column at a time"""
    out = set()
    for l in range(min_ovlp, len(q) + 1):
        suf = q[len(q) - l:]
        if (suf == 5).any():
            break
        cand = np.flatnonzero(lens >= l)
        for j in range(l):
            cand = cand[S[cand, j] == suf[j]]
            if len(cand) == 0:
                break
        out.update((int(k), l) for k in cand)
    return out


def test_overlaps_against_brute_force(idx):
    """records to string ids in one call, against slices of the strings; ids are rows of the $ block, whatever the order of the index"""
    cx, g = idx, idx.g
    lens = np.array([len(s) for s in cx.strings], np.int64)
    S = np.zeros((cx.n, int(lens.max()) + 1), np.uint8)
    for k, s in enumerate(cx.strings):
        S[k, :len(s)] = s
    rng = np.random.RandomState(3)
    well = len(cx.queries) - len(MALFORMED)
    pick = np.concatenate([rng.choice(cx.n, size=BRUTE - 8, replace=False), np.arange(well - 8, well)])     # strings of the index, made-up ones
    qs = [cx.queries[i] for i in pick]
    g.build_ssa(4)
    few = OR.brute_overlaps(cx.strings[:50], qs[0], 1)
    assert few == {p for p in _brute(S, lens, qs[0], 1) if p[0] < 50}      # the matrix form of the brute force against the plain one
    hits, both = 0, {}
    for min_ovlp in (1, 3):
        both[min_ovlp] = g.overlaps(qs, min_ovlp, max_hits=cx.n)
        for q, o in zip(qs, both[min_ovlp]):
            assert [l for _, l in o] == sorted((l for _, l in o), reverse=True)                             # longest first
            assert len(set(o)) == len(o) and set(o) == _brute(S, lens, q, min_ovlp), (q.tolist(), min_ovlp)
            hits += len(o)
    assert hits > 1000
    got = both[1]
    cut = g.overlaps(qs[:8], 1, max_hits=2)                          # max_hits caps every length
    assert all(set(c) <= set(o) and len(c) <= 2 * len({l for _, l in o}) for c, o in zip(cut, got)) and any(len(c) < len(o) for c, o in zip(cut, got))
    txt = "".join("$ACGTN"[c] for c in qs[0])
    assert g.overlaps([txt], 1, max_hits=cx.n)[0] == got[0]
    with pytest.raises(ValueError):
        g.overlaps([np.array(MALFORMED[0], np.uint8)], 1)
    assert g.overlaps([], 1) == []


def _child(stage):
    p = subprocess.run([sys.executable, os.path.join(HERE, "overlap_child.py"), stage], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p.returncode, p.stdout.decode(), p.stderr.decode()[-1500:]


def test_chunked_staging(hip):
    rc, out, err = _child("chunk")
    assert rc == 0 and "STAGE OK" in out, (rc, out, err)


def test_string_ids_without_array_is_fatal(hip):
    rc, out, err = _child("nossa")
    assert rc == 7 and "NOT FATAL" not in out, (rc, out, err)
    assert "'valid': False" in out and "overlap ok" in out and "handler: [rb2_hip] string_ids" in out and "rb2_hip_ssa_build" in out, out
