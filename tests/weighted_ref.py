"""The weighted BWT: an exact reference for indexes of more than 2^32 rows that never expands them.

Let D be a set of distinct strings with BWT bwt0 (n0 rows) and give string j a weight w_j >= 1.  With wrow[k] = the weight of the string
small row k belongs to, np.repeat(bwt0, wrow) is the BWT of the multiset that holds w_j copies of string j -- in input order when the
copies of a string are consecutive, in RLO and RCLO wherever the copies come from, later batches included (tests/test_weighted_ref.py
holds this against the oracle).  Small row k becomes the block of big rows [start[k], start[k + 1]); big row x = (k, t) is offset t of
block k.  Then

  occ(a, x) = occW[k][a] + t * [bwt0[k] == a]      a prefix sum over n0 values
  LF keeps t                                        so every query answer follows from the small index

WeightedFM duck-types query_ref.FM: N, C, and occ / bwt as views that answer occ[x], occ[x, c], occ[array], occ[array, c], occ[:, c][array],
bwt[x] and bwt[array] on demand by searchsorted on start.  backward_search, count, extend, extend_many, walk and sym_interval are inherited
unchanged, and overlap_ref, kmer_ref, approx_ref, smem_ref, contain_ref and irreducible_ref, which go through fm.occ, fm.bwt, fm.C and fm.N
only, run on it as they are.  What would allocate N entries (walk_all, locate_ref's _sa, overlap_ref's _head) raises; the laws at the end
of the class take their place.  Used by tests/test_weighted_ref.py (CPU) and tests/test_big_rows_gpu.py."""
import numpy as np

import helpers as H
import locate_ref as LR
import query_ref as Q

RUN_MAX = 1 << 32                         # fmd_streams.RUN_MAX: every run of runs() is shorter


class _Col:
    """occ[:, c]: one column, indexed by rows"""
    def __init__(self, fm, c):
        self.fm, self.c = fm, c

    def __getitem__(self, x):
        return self.fm._rank_of(x, self.c)


class _Occ:
    def __init__(self, fm):
        self.fm = fm

    def __getitem__(self, key):
        if isinstance(key, tuple):
            x, c = key
            if isinstance(x, slice):
                assert x == slice(None), "only occ[:, c]"
                return _Col(self.fm, c)
            return self.fm._rank_of(x, c)
        return self.fm._ranks(key)


class _Bwt:
    def __init__(self, fm):
        self.fm = fm

    def __getitem__(self, x):
        k, _ = self.fm.block(x)
        assert (np.asarray(k) < self.fm.n0).all(), "row N has no symbol"
        return self.fm.bwt0[k]


class WeightedFM(Q.FM):
    def __init__(self, bwt0, wrow):
        self.bwt0 = np.asarray(bwt0, dtype=np.uint8)
        self.wrow = np.asarray(wrow, dtype=np.int64)
        self.n0 = len(self.bwt0)
        assert len(self.wrow) == self.n0 and (self.wrow >= 1).all(), "one weight >= 1 per small row"
        self.start = np.concatenate([[0], np.cumsum(self.wrow)]).astype(np.int64)
        self.N = int(self.start[-1])
        self.occW = np.zeros((self.n0 + 1, 6), np.int64)
        if self.n0:
            self.occW[1:] = np.cumsum(np.eye(6, dtype=np.int64)[self.bwt0] * self.wrow[:, None], axis=0)
        self.C = np.concatenate([[0], np.cumsum(self.occW[self.n0])[:5]]).astype(np.int64)
        self._sym0 = np.concatenate([self.bwt0, [6]]).astype(np.int64)     # (block n0 = row N: no symbol)
        self.occ, self.bwt = _Occ(self), _Bwt(self)

    # ---- the views ------------------------------------------------------------------------------------------------------------------
    def block(self, x):
        """(k, t): big row x is offset t of block k; row N is (n0, 0).  Scalars or arrays"""
        x = np.asarray(x, dtype=np.int64)
        assert ((x >= 0) & (x <= self.N)).all(), "row outside [0, N]"
        k = np.searchsorted(self.start, x, "right") - 1
        t = x - self.start[k]
        return (int(k), int(t)) if x.ndim == 0 else (k, t)

    def _rank_of(self, x, c):
        k, t = self.block(x)
        c = np.asarray(c, dtype=np.int64)
        r = self.occW[k, c] + t * (self._sym0[k] == c)
        return int(r) if np.ndim(r) == 0 else r

    def _ranks(self, x):
        k, t = self.block(x)
        return self.occW[k] + np.asarray(t)[..., None] * (np.asarray(self._sym0[k])[..., None] == np.arange(6))

    def walk_all(self):
        raise TypeError("walk_all() would allocate N entries: use text()")

    @property
    def _sa(self):
        raise TypeError("locate_ref.suffix_array() would allocate N entries: use locate_rows()")

    @property
    def _head(self):
        raise TypeError("overlap_ref.head() would allocate C[1] entries: use head()")

    # ---- the big BWT as runs ---------------------------------------------------------------------------------------------------------------
    def runs(self):
        """the maximal runs (l, c) of the big BWT, as fmd_streams.cut, .counts and .image take them"""
        if self.n0 == 0:
            return []
        first = np.flatnonzero(np.concatenate([[True], self.bwt0[1:] != self.bwt0[:-1]]))
        l = np.add.reduceat(self.wrow, first)
        assert (l < RUN_MAX).all(), "a run of 2^32 symbols or more"
        return list(zip(l.tolist(), self.bwt0[first].tolist()))

    # ---- the laws (models made by from_strings) ----------------------------------------------------------------------------------------------
    @property
    def n_strings(self):
        return int(self.C[1])

    def interval(self, pat):
        """(lo, hi, m) of backward_search(pat) from the small index: [start[lo0], start[hi0]) with the same m"""
        lo0, hi0, m = self.fm0.backward_search(pat)
        return (-1, -1, -1) if m < 0 else (int(self.start[lo0]), int(self.start[hi0]), m)

    def string_of(self, ids):
        """(q0, t): big string id = copy t of small string q0 (the `$` block of the big index is the blocks of the small one's)"""
        ids = np.asarray(ids, dtype=np.int64)
        assert ((ids >= 0) & (ids < self.n_strings)).all(), "no string id"
        return self.block(ids)

    def text(self, sid):
        """the text of big string id (q0, t) is that of small string q0"""
        return self.texts0[self.string_of(int(sid))[0]]

    def locate_rows(self, x):
        """(string id, position) of the big rows x: row (k, t) lies on the walk of copy t of the string of block k"""
        k, t = self.block(x)
        return self.start[self.sid0[k]] + t, self.pos0[k]

    def locate(self, lo, hi, max_hits):
        """locate_ref.locate on the big index"""
        if lo < 0 or hi > self.N or lo > hi:
            return np.zeros((0, 2), np.int64), -1
        s, p = self.locate_rows(np.arange(lo, lo + min(hi - lo, max_hits), dtype=np.int64))
        return np.stack([s, p], 1).astype(np.int64), hi - lo

    def locate_raw(self, intervals, max_hits):
        """locate_ref.locate_raw on the big index"""
        iv = np.asarray(intervals, dtype=np.int64).reshape(-1, 2)
        hit = np.zeros((len(iv), max_hits, 2), np.int64)
        cnt = np.zeros(len(iv), np.int64)
        for i, (lo, hi) in enumerate(iv.tolist()):
            h, cnt[i] = self.locate(lo, hi, max_hits)
            hit[i, :len(h)] = h
        return int(np.minimum(np.maximum(cnt, 0), max_hits).sum()), hit, cnt

    def head(self, z):
        """head[z] = the string whose whole-string row holds the z-th `$` of the big BWT (overlap_ref.head), for an array of `$` ranks:
        the z-th `$` is offset t of a block whose small row holds a `$`, and occ[.., 0] at that block's start is where its ranks begin"""
        z = np.asarray(z, dtype=np.int64)
        assert ((z >= 0) & (z < self.n_strings)).all()
        i = np.searchsorted(self._zstart, z, "right") - 1
        return self.start[self.sid0[self._zrows[i]]] + (z - self._zstart[i])

    def string_ids(self, zlo, zhi, max_hits):
        """overlap_ref.string_ids on the big index"""
        if zlo < 0 or zhi > self.n_strings or zlo > zhi:
            return np.zeros(0, np.int64), -1
        return self.head(np.arange(zlo, zlo + min(zhi - zlo, max_hits), dtype=np.int64)), zhi - zlo

    def string_ids_raw(self, ranges, max_hits):
        zv = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
        ids = np.zeros((len(zv), max_hits), np.int64)
        cnt = np.zeros(len(zv), np.int64)
        for i, (zlo, zhi) in enumerate(zv.tolist()):
            h, cnt[i] = self.string_ids(zlo, zhi, max_hits)
            ids[i, :len(h)] = h
        return int(np.minimum(np.maximum(cnt, 0), max_hits).sum()), ids, cnt

    def weights(self):
        """the weight of every string of D, in the order of D"""
        w = np.zeros(len(self.D), np.int64)
        w[self.d_of_q] = self.wq
        return w

    def reweighted(self, w2):
        """the model of the same D with the weights w2 (in the order of D): after a delete, an insert of copies or a merge.  A string
        whose weight reaches 0 drops out: the model is rebuilt from the remaining strings with the oracle"""
        w2 = np.asarray(w2, dtype=np.int64)
        assert len(w2) == len(self.D) and (w2 >= 0).all()
        keep = np.flatnonzero(w2 > 0)
        return from_strings(self.so, [self.D[j] for j in keep], w2[keep])


def from_strings(so, D, w):
    """the model of w[j] copies of D[j] (distinct strings, text order) in sorting order so: the small BWT from helpers.Oracle(so), the
    rows assigned to strings by walking the small index.  Beside the WeightedFM: fm0 (the small query_ref.FM), sid0 / pos0 (per small
    row: small string id, position), texts0 (per small string id), wq (its weight), d_of_q (its index in D)"""
    D = [np.asarray(s, dtype=np.uint8).reshape(-1) for s in D]
    w = np.asarray(w, dtype=np.int64)
    index = {s.tobytes(): j for j, s in enumerate(D)}
    assert len(index) == len(D) == len(w), "distinct strings, one weight each"
    o = H.Oracle(so)
    o.insert_multi(H.encode_batch(D, True, False))
    bwt0 = o.bwt()
    o.close()
    fm0 = Q.FM(bwt0)
    sid0, pos0, _ = LR.suffix_array(fm0)
    texts0 = fm0.walk_all()[0]
    d_of_q = np.array([index[t.tobytes()] for t in texts0], np.int64)
    assert sorted(d_of_q.tolist()) == list(range(len(D)))
    if so == 0:
        assert (d_of_q == np.arange(len(D))).all()
    wq = w[d_of_q] if len(D) else np.zeros(0, np.int64)
    m = WeightedFM(bwt0, wq[sid0] if len(D) else np.zeros(0, np.int64))
    m.so, m.D, m.fm0, m.sid0, m.pos0, m.texts0, m.wq, m.d_of_q = so, D, fm0, sid0, pos0, texts0, wq, d_of_q
    m._zrows = np.flatnonzero(bwt0 == 0)
    m._zstart = m.occW[m._zrows, 0]
    return m


def copies(D, w):
    """w[j] consecutive copies of every D[j]: the strings of the multiset in the input order whose BWT the model is"""
    return [D[j] for j in range(len(D)) for _ in range(int(w[j]))]


# ---- counts and pieces of a model ----------------------------------------------------------------------------------------------------

def counts(fm):
    """M[b][a] = symbols a in rope b (what HipBwt.counts() returns)"""
    edge = fm.occ[np.concatenate([fm.C, [fm.N]])]
    return edge[1:] - edge[:-1]


def piece_rows(fm):
    """(first global row, symbols) of each of the 31 pieces: rope $, then (b,x) = the b's of rope x in the order of x"""
    M = counts(fm)
    rows, size = [0], [int(fm.C[1])]
    for b in range(1, 6):
        row = int(fm.C[b])
        for x in range(6):
            rows.append(row); size.append(int(M[x, b]))
            row += int(M[x, b])
    return np.array(rows, np.int64), np.array(size, np.int64)


# ---- the two fixtures of tests/test_big_rows_gpu.py (their properties are asserted in tests/test_weighted_ref.py) ---------------------

def _even():
    """some 150 distinct reads of 12-200 symbols from a 2500-symbol genome with a few N, each with its reverse complement (D[2i], D[2i+1]),
    no palindromes; one weight per pair from [M/2, 3M/2), M = 1.5 * 2^32 / n0"""
    pairs, seen = [], set()
    for r in H.repetitive_reads(600, seed=31, genome_len=2500, max_len=200):
        rc = Q.revcomp(r)
        a, b = r.tobytes(), rc.tobytes()
        if len(r) < 12 or a == b or a in seen or b in seen:
            continue
        seen |= {a, b}
        pairs.append((r, rc))
        if len(pairs) == 150:
            break
    D = [s for p in pairs for s in p]
    n0 = sum(len(s) + 1 for s in D)
    M = int(1.5 * 2 ** 32 / n0)
    w = np.repeat(np.random.RandomState(32).randint(M // 2, 3 * M // 2, size=len(pairs)), 2)
    return from_strings(1, D, w)


def _skewed():
    """one strand: 150 distinct strings of 20-200 symbols with 85 % A, weights from [M/2, 3M/2), M = 2.1 * 2^32 / n0"""
    rng = np.random.RandomState(41)
    D, seen = [], set()
    while len(D) < 150:
        ln = int(rng.randint(20, 201))
        s = np.where(rng.rand(ln) < 0.85, 1, rng.randint(2, 5, size=ln)).astype(np.uint8)
        if s.tobytes() not in seen:
            seen.add(s.tobytes())
            D.append(s)
    n0 = sum(len(s) + 1 for s in D)
    M = int(2.1 * 2 ** 32 / n0)
    return from_strings(1, D, rng.randint(M // 2, 3 * M // 2, size=len(D)))


_fixtures = {}


def fixture(name):
    """the model of fixture `even` or `skewed` (both RLO), made once per process"""
    if name not in _fixtures:
        _fixtures[name] = {"even": _even, "skewed": _skewed}[name]()
        _fixtures[name].name = name
    return _fixtures[name]
