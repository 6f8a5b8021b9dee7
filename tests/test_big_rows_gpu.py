"""GPU tests of the queries, delete, insert and merge on indexes of more than 2^32 rows and more than 2^24 strings: global rows that do
not fit 32 bits (qrank and every kernel on top of it), string ids above 2^24 (the second launch of k_ssa_build, the split launches of
k_locate and k_string_ids), a piece of more than 2^32 symbols.  Every expected value comes from the weighted-BWT model
(tests/weighted_ref.py, proven on the CPU by tests/test_weighted_ref.py) and the integers must be equal.

The two fixtures (weighted_ref.fixture; their properties are asserted on the CPU), both loaded into RLO handles from their runs:

  even     300 strings (150 reads and their reverse complements), n0 = 31 902 small rows, N = 6.59e9 rows = 1.53 x 2^32,
           6.17e7 strings = 3.68 x 2^24, 5 074 runs; every piece below 2^32 symbols, row 2^32 inside rope G
  skewed   150 strings of one strand with 85 % A, n0 = 16 453, N = 9.14e9 = 2.13 x 2^32, 8.21e7 strings = 4.89 x 2^24, 4 396 runs;
           piece (A,A) holds 1.52 x 2^32 symbols

Each family asserts on the CPU side, before it asks the device, that its inputs reach the regime it is about: a stated minimum of answers
with lo >= 2^32, with lo < 2^32 <= hi, with a string id >= 2^24 and >= 2 x 2^24, and (skewed) with a piece offset >= 2^32.  The inputs are
chosen so that the minima hold by construction: rows around 2^32 and around multiples of 2^25 in every piece, patterns that begin with
T (rope T begins above 2^32 in both fixtures) and prefixes of the suffix whose block holds row 2^32, string ids around 2^24 and 2 x 2^24.

Measured on one MI355X (the TIMING and MEMORY lines every test prints; device memory is the drop of rb2_hip_mem_info's free bytes):

                                        even                      skewed
  load_ropes from the runs              0.22 s, 3.04 GiB          0.03 s, 3.95 GiB
  build_ssa(7)                          0.50 s, 1.69 GiB          0.69 s, 2.29 GiB     (N LF steps: 13 G steps/s)
  peak, read-only families              7.04 GiB                  8.26 GiB
  delete (2.1e5 / 4.1e5 strings)        0.01 s, 5.26 GiB          0.04 s, 7.33 GiB
  insert, default policy                0.03 s, 8.03 GiB          0.06 s, 10.98 GiB    (in place: 201 / 197 sparse rounds)
  insert, forced sparse                 0.02 s, 8.03 GiB          0.06 s, 12.79 GiB
  insert, RB2_SPARSE_LAMBDA=0           0.19 s, 6.09 GiB          0.26 s, 8.42 GiB     (dense rounds)
  merge (470 / 242 strings)             0.03 s, 8.53 GiB          0.05 s, 11.48 GiB
  save_fmd + ranks + searches after a change                      0.16 - 0.21 s

Every read-only family spends under 0.05 s on the device (extend of 97 117 bi-intervals in both directions 0.03 s, skewed approx with two
mismatches 0.05 s, everything else below 0.02 s); the time of a test is the model's: 3.5 s for the SMEM tables of 43 queries, 2.2 s for
approx with two mismatches on skewed, under 0.5 s elsewhere.  The file: 49 tests in 17 s.  The memory estimate of need_bytes() (0.375 B
per symbol and side x 1.8, the suffix array, 4 GiB of room: 14 and 18 GiB) is above every measured figure.
"""
import time
from contextlib import contextmanager

import numpy as np
import pytest

import approx_ref as AR
import contain_ref as CR
import fmd_streams as F
import helpers as H
import irreducible_ref as IR
import kmer_ref as KR
import overlap_ref as OV
import smem_ref as SR
import weighted_ref as W
from fmd_save_ref import write_fmd
from test_query_gpu import _Env, _check_search, _patterns
from test_query_layouts_gpu import FORCED, WIDE

pytestmark = pytest.mark.gpu
T32, T24 = 1 << 32, 1 << 24
SSA_S = 7                                                            # log2_step: N / 128 samples of 16 bytes, 0.8 and 1.1 GB
GIB = 1 << 30
GRAPH = dict(min_ovlp=10, max_ext=200, max_steps=1 << 16, max_recs=64, max_hits=8)


# ---- the CPU side: inputs and expected values, from the model alone (nothing here touches a device) --------------------------------------

class _Model:
    """a fixture's model with its query sets and their answers, each made once"""
    def __init__(self, name):
        self.name, self.m = name, W.fixture(name)
        self.S = self.m.runs()
        self.memo = {}

    def get(self, what):
        if what not in self.memo:
            self.memo[what] = getattr(self, "_" + what)()
        return self.memo[what]

    def _rows(self):
        """the rows of the rank family: every block start - 1, + 0, + 1; around 2^32; the multiples of 2^25 inside every piece (one
        SbBase chunk of a dense piece) with their neighbours; every piece's first row +- 1; N - 1 and N"""
        return rank_rows(self.m)

    def _patterns(self):
        return search_patterns(self.m, np.random.RandomState(11))

    def _ids(self):
        """string ids: 0, 1, around 2^24 and 2 x 2^24, the last, some hundred random ones"""
        n = self.m.n_strings
        rng = np.random.RandomState(12)
        ids = [0, 1, T24 - 1, T24, T24 + 1, 2 * T24 - 1, 2 * T24, 2 * T24 + 1, n - 1] + rng.randint(0, n, size=100).tolist()
        return np.array(ids, np.int64)

    def _ranges(self):
        """id ranges (first, n) of a hundred sources: at the start, across 2^24, across 2 x 2^24, at the end"""
        n = self.m.n_strings
        return [(0, 100), (T24 - 50, 100), (2 * T24 - 50, 100), (n - 100, 100)]

    def _sources(self):
        """the ids of the ranges, and the first copy and the last of forty more strings: ten that begin with each of A C G T"""
        m = self.m
        ids = [np.arange(f, f + n) for f, n in self.get("ranges")]
        for c in (1, 2, 3, 4):
            q0 = [q for q in range(len(m.texts0)) if len(m.texts0[q]) and m.texts0[q][0] == c][:10]
            ids += [m.start[q0], m.start[np.array(q0) + 1] - 1]
        return np.concatenate(ids).astype(np.int64)

    def smems(self, q0, min_len, min_occ):
        key = ("smem", q0)
        q = self.m.texts0[q0][:80]
        if key not in self.memo:
            self.memo[key] = SR.occ_table(self.m, q)
        return SR.smems_from_table(self.m, q, self.memo[key], min_len, min_occ)

    def irreducible(self, q0, p=GRAPH):
        """(records, cnt) of the text of small string q0; equality is owed only where nothing is cut: asserted here"""
        key = ("irr", q0, p["min_ovlp"], p["max_ext"])
        if key not in self.memo:
            recs, cnt, steps = IR.irreducible(self.m, self.m.texts0[q0], p["min_ovlp"], p["max_ext"], p["max_steps"])
            assert 0 <= cnt <= p["max_recs"] and steps < p["max_steps"], (q0, cnt, steps)
            self.memo[key] = recs, cnt
        return self.memo[key]

    def edges(self, first, n, p=GRAPH):
        """(the rows src, dst, l, ext of the sources first .. first + n - 1, sorted; the records whose range holds more than max_hits)"""
        m = self.m
        q0s, _ = m.string_of(np.arange(first, first + n))
        rows, wide = [], 0
        for s, q0 in zip(range(first, first + n), q0s.tolist()):
            for l, ext, zlo, zhi in self.irreducible(q0, p)[0]:
                wide += zhi - zlo > p["max_hits"]
                rows += [(s, int(d), l, ext) for d in m.head(zlo + np.arange(min(zhi - zlo, p["max_hits"])))]
        return _sorted(rows), wide


def _sorted(rows):
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    return rows[np.lexsort(rows.T[::-1])]


def rank_rows(m):
    rows, size = W.piece_rows(m)
    xs = [m.start - 1, m.start, m.start + 1, T32 + np.array([-1025, -1024, -1, 0, 1, 1023, 1024]), rows - 1, rows, rows + 1, [m.N - 1, m.N]]
    for r0, sz in zip(rows.tolist(), size.tolist()):
        k = r0 + np.arange(0, sz, 1 << 25, dtype=np.int64)
        xs += [k - 1, k, k + 1]
    return np.unique(np.clip(np.concatenate([np.asarray(x, np.int64) for x in xs]), 0, m.N))


def piece_offsets(m, x):
    """offset of the rows x in their pieces (an empty piece shares its first row with the next one and holds no row)"""
    rows, size = W.piece_rows(m)
    rows = rows[size > 0]
    return x - rows[np.searchsorted(rows, x, "right") - 1]


def straddlers(m):
    """prefixes of the suffix whose block holds row 2^32: every one of their intervals holds that row"""
    k, _ = m.block(T32)
    suf = m.texts0[m.sid0[k]][m.pos0[k]:]
    return [suf[:l].copy() for l in range(1, min(len(suf), 30) + 1)]


def search_patterns(m, rng):
    """(patterns, the model's lo, hi, m): substrings of D, those from every string's first T on, suffixes with a trailing `$`, random
    patterns, the straddlers, the empty and the malformed patterns of test_query_gpu._patterns"""
    D = [s for s in m.D]
    pats = []
    for _ in range(300):
        s = D[rng.randint(len(D))]
        a = rng.randint(len(s))
        pats.append(s[a:a + rng.randint(1, 61)].copy())
    for s in D:                                                     # begin with T: rope T begins above 2^32
        t = np.flatnonzero(s == 4)
        if len(t):
            pats.append(s[t[0]:t[0] + 1 + len(pats) % 40].copy())
    for _ in range(100):
        s = D[rng.randint(len(D))]
        pats.append(np.concatenate([s[len(s) - rng.randint(1, 61):], [0]]).astype(np.uint8))
    pats += [rng.randint(1, 6, size=rng.randint(1, 31)).astype(np.uint8) for _ in range(100)]
    pats += [np.concatenate([p, [0]]).astype(np.uint8) for p in pats[:50]]
    pats += straddlers(m)
    pats += _patterns(D, rng, k=0)[-6:]
    want = np.array([m.interval(p) for p in pats], np.int64).reshape(-1, 3)
    full = want[:, 2] == [len(p) for p in pats]
    assert full[:300].all() and (want[-6:, 2] == [0, 1, -1, -1, -1, -1]).all() and (~full).sum() > 50
    assert (full & (want[:, 0] >= T32)).sum() >= 100, "matched patterns with lo >= 2^32"
    assert (full & (want[:, 0] < T32) & (want[:, 1] >= T32) & (want[:, 2] > 0)).sum() >= 3, "matched patterns with lo < 2^32 <= hi"
    return pats, want


class _Shim:
    """what test_query_gpu._check_search asks of a model"""
    def __init__(self, m):
        self.backward_search = m.interval


def check_ranks(g, m):
    """rank_batch per rope at every block start, the row before and the row behind, against the model (rope-relative rows)"""
    edge = np.concatenate([m.C, [m.N]])
    base = m.occ[edge[:6]]
    for b in range(6):
        lo, hi = int(edge[b]), int(edge[b + 1])
        if lo == hi:
            continue
        s = m.start[(m.start >= lo) & (m.start <= hi)]
        xs = np.unique(np.clip(np.concatenate([s - 1, s, s + 1, [lo, hi]]), lo, hi))
        got, want = g.rank_batch(b, xs - lo), m.occ[xs] - base[b]
        bad = np.flatnonzero((got != want).any(1))
        assert len(bad) == 0, "rope %d: %d of %d ranks differ; first at row %d: got %s want %s" % (b, len(bad), len(xs), xs[bad[0]] - lo, got[bad[0]], want[bad[0]])


# ---- the device side -----------------------------------------------------------------------------------------------------------------------

def mem_info(hip):
    a = np.zeros(2, np.int64)
    hip.load_hip_lib().rb2_hip_mem_info(0, a.ctypes.data, a.ctypes.data + 8)
    return int(a[0]), int(a[1])


def need_bytes(m):
    """an estimate: 0.375 B per symbol and side, 1.8 x in the sparse layout, the suffix array, and 4 GiB of room"""
    return int(m.N * 0.375 * 2 * 1.8) + (m.N >> SSA_S) * 16 + m.n_strings * 16 + 4 * GIB


def load(hip, mo):
    """a fresh RLO handle holding the fixture; skips when the device has too little free memory"""
    free, total = mem_info(hip)
    need = need_bytes(mo.m)
    if free < need:
        pytest.skip("%s needs some %.1f GiB of device memory, %.1f of %.1f GiB are free" % (mo.name, need / GIB, free / GIB, total / GIB))
    g = hip.HipBwt(1)
    g.load_ropes(F.cut(mo.S))
    return g


class _Ctx:
    pass


@pytest.fixture(scope="module")
def models():
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Model(name)
        return made[name]
    yield get
    made.clear()


@pytest.fixture(scope="module", params=["even", "skewed"])
def big(request, hip, models):
    """the handle of the read-only families"""
    t0 = time.time()
    mo = models(request.param)
    free0 = mem_info(hip)[0]
    g = load(hip, mo)
    cx = _Ctx()
    cx.name, cx.mo, cx.m, cx.g, cx.hip = mo.name, mo, mo.m, g, hip
    cx.counts0, cx.hashes0 = g.counts(), g.rope_hashes()
    assert np.array_equal(cx.counts0, W.counts(mo.m)) and not g.layout_stats()["sparse_now"]
    cx.free0, cx.low = free0, mem_info(hip)[0]
    print("TIMING %s: load %.2f s, %d runs, %d rows, %d strings, %.2f GiB of device memory" % (
        cx.name, time.time() - t0, len(mo.S), mo.m.N, mo.m.n_strings, (free0 - cx.low) / GIB))
    yield cx
    print("MEMORY %s: peak %.2f GiB with the suffix array and the queries' buffers" % (cx.name, (free0 - cx.low) / GIB))
    g.close()


@contextmanager
def family(cx, what):
    """a read-only family: counts() and rope_hashes() are what they were after the load; one TIMING line"""
    t0 = time.time()
    yield
    t1 = time.time()
    cx.low = min(cx.low, mem_info(cx.hip)[0])
    assert np.array_equal(cx.g.counts(), cx.counts0) and cx.g.rope_hashes() == cx.hashes0, "%s changed the index" % what
    print("TIMING %s %s: %.2f s (and %.2f s for counts and hashes)" % (cx.name, what, t1 - t0, time.time() - t1))


def ssa(cx):
    if not cx.g.ssa_info()["valid"]:
        cx.g.build_ssa(SSA_S)


def first_bad(got, want):
    bad = np.flatnonzero((got != want).reshape(len(want), -1).any(1))
    return "%d of %d differ; first: item %d got %s want %s" % (len(bad), len(want), bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())


EVEN_ONLY = pytest.mark.parametrize("big", ["even"], indirect=True)      # SMEMs, irreducible overlaps and the string graph need both strands


# ---- read-only families ------------------------------------------------------------------------------------------------------------------

def test_ranks_through_extend(big):
    cx, m, g = big, big.m, big.g
    N = m.N
    x = cx.mo.get("rows")
    iks = [np.stack([x, x, np.minimum(1, N - x)], 1)]
    rows, _ = W.piece_rows(m)
    for sz in WIDE:
        b = np.concatenate([rows - 1, rows, rows + 1, T32 + np.array([-sz, -1025, -1, 0, 1]), m.start[::97], [N - sz]])
        b = np.unique(np.clip(b, 0, N - sz))
        iks.append(np.stack([b, b, np.full(len(b), sz)], 1))
    iks = np.concatenate(iks).astype(np.int64)
    lo, hi = iks[:, 0], iks[:, 0] + iks[:, 2]
    assert (lo >= T32).sum() >= 20000 and ((lo < T32) & (hi >= T32)).sum() >= 6
    assert len(x) > 3 * m.n0 and (np.diff(x) > 0).all() and x[-1] == N
    if cx.name == "skewed":
        assert (piece_offsets(m, x) >= T32).sum() >= 100, "rows at a piece offset >= 2^32"
    with family(cx, "extend, %d bi-intervals, both directions" % len(iks)):
        for is_back in (1, 0):
            got, want = g.extend(iks, is_back), m.extend_many(iks, is_back)
            assert np.array_equal(got, want), "is_back=%d: %s" % (is_back, first_bad(got, want))


def test_backward_search(big):
    cx, g = big, big.g
    pats, want = cx.mo.get("patterns")
    with family(cx, "backward_search and _dev, %d patterns" % len(pats)):
        got = _check_search(g, _Shim(cx.m), pats)
    assert np.array_equal(got, want)


def test_extract(big):
    cx, m, g = big, big.m, big.g
    ids, n = cx.mo.get("ids"), m.n_strings
    assert (ids >= T24).sum() >= 50 and (ids >= 2 * T24).sum() >= 20 and n - 1 in ids
    texts = [m.text(s) for s in ids]
    lens = np.array([len(t) for t in texts])
    assert (lens > 50).sum() >= 20 and (lens <= 50).sum() >= 5
    with family(cx, "extract, %d ids" % len(ids)):
        got = g.extract(ids, 200)
        fit, out, ln = g.extract_raw(ids, 50)                       # a max_len that is too short
        _, _, bad = g.extract_raw([-1, n, n + 5, m.N + 3, 0], 50)   # rows outside the `$` block
        with pytest.raises(ValueError):
            g.extract([n], 5)
    for s, a, b in zip(ids.tolist(), got, texts):
        assert a is not None and np.array_equal(a, b), "string %d" % s
    assert np.array_equal(ln, np.where(lens > 50, -1, lens)) and fit == (lens <= 50).sum()
    for i in np.flatnonzero(lens <= 50):
        assert np.array_equal(out[i, :lens[i]], texts[i])
    assert bad.tolist() == [-2, -2, -2, -2, len(m.text(0)) if len(m.text(0)) <= 50 else -1]


def test_unpack(big):
    cx, m, g = big, big.m, big.g
    from test_merge_gpu import _unpack_dev
    ranges = cx.mo.get("ranges")
    assert sum(f + n > T24 for f, n in ranges) >= 3 and sum(f + n > 2 * T24 for f, n in ranges) >= 2
    with family(cx, "unpack and _dev, %d ranges" % len(ranges)):
        for first, n in ranges:
            want = [m.text(s) for s in range(first, first + n)]
            got = g.unpack(first, n)
            assert len(got) == n and all(np.array_equal(a, b) for a, b in zip(got, want)), (first, n)
            for rev in (False, True):
                wt = np.concatenate([np.concatenate([t[::-1] if rev else t, [0]]) for t in want]).astype(np.uint8)
                woff = np.concatenate([[0], np.cumsum([len(t) + 1 for t in want])])
                txt, off = g.unpack_raw(first, n, rev)
                assert np.array_equal(off, woff) and np.array_equal(txt, wt), (first, n, rev)
                size, dtxt, doff = _unpack_dev(g, first, n, rev, len(wt))
                assert size == len(wt) and np.array_equal(doff, woff) and np.array_equal(dtxt[:size], wt), (first, n, rev)


@EVEN_ONLY
def test_smem(big):
    cx, m, g = big, big.m, big.g
    src = cx.mo.get("sources")
    q0s, _ = m.string_of(src)
    assert (src >= T24).sum() >= 100 and (src >= 2 * T24).sum() >= 100
    uq = np.unique(q0s)
    qs = [m.texts0[q][:80] for q in uq]
    for min_len, min_occ in ((1, 1), (17, 1), (5, int(m.wq.min()) * 3)):
        want = [cx.mo.smems(q, min_len, min_occ) for q in uq]
        allw = np.concatenate(want)
        assert (allw[:, 2] >= T32).sum() >= 10 and (allw[:, 3] >= T32).sum() >= 10 and len(allw) >= len(uq) // 2, "SMEMs with x0, x1 >= 2^32"
        with family(cx, "smem, %d queries, min_len %d, min_occ %d" % (len(qs), min_len, min_occ)):
            stored, mem, cnt = g.smem_raw(qs, min_len, min_occ, 64)
        assert cnt.tolist() == [len(w) for w in want] and stored == cnt.sum()
        for i, w in enumerate(want):
            assert np.array_equal(mem[i, :len(w)], w) and (mem[i, len(w):] == 0).all(), (int(uq[i]), mem[i, :len(w) + 1].tolist(), w.tolist())


def test_build_ssa(big):
    """the first run of k_ssa_build with k0 > 0: strings 2^24 and up are walked by the second launch and those behind it"""
    cx, m, g = big, big.m, big.g
    assert m.n_strings > 3 * T24
    g.drop_ssa()
    with family(cx, "build_ssa(%d)" % SSA_S):
        ns = g.build_ssa(SSA_S)
    assert ns == -(-m.N // (1 << SSA_S))
    inf = g.ssa_info()
    assert inf["valid"] and inf["log2_step"] == SSA_S and inf["samples"] == ns and inf["device_bytes"] >= 16 * ns + 16 * m.n_strings
    print("suffix array of %s: %d samples, %.2f GiB" % (cx.name, ns, inf["device_bytes"] / GIB))


def test_locate(big):
    from test_locate_gpu import _locate_dev
    cx, m, g = big, big.m, big.g
    ssa(cx)
    pats, want = cx.mo.get("patterns")
    full = (want[:, 2] == [len(p) for p in pats]) & (want[:, 1] > want[:, 0])
    iv = np.concatenate([want[full, :2], [(-1, 2), (0, m.N + 1), (5, 4), (m.N, m.N)]])
    x = cx.mo.get("rows")
    x = x[x < m.N]
    s1, p1 = m.locate_rows(x)
    assert (x >= T32).sum() >= 20000 and (s1 >= T24).sum() >= 20000 and (s1 >= 2 * T24).sum() >= 10000
    if cx.name == "skewed":
        assert (piece_offsets(m, x) >= T32).sum() >= 100
    for mh in (1, 5):
        w_stored, w_hit, w_cnt = m.locate_raw(iv, mh)
        assert (w_hit[:, :, 0] >= 2 * T24).sum() >= 50 and (iv[:, 0] >= T32).sum() >= 100
        with family(cx, "locate and _dev, %d intervals, max_hits %d" % (len(iv), mh)):
            stored, hit, cnt = g.locate_raw(iv, mh)
            dhit, dcnt = _locate_dev(g, iv, mh)
        assert np.array_equal(cnt, w_cnt) and np.array_equal(dcnt, w_cnt) and stored == w_stored
        assert np.array_equal(hit, w_hit), first_bad(hit, w_hit)
        live = np.arange(mh)[None, :] < np.maximum(w_cnt, 0)[:, None]
        assert np.array_equal(dhit[live], w_hit[live])
    with family(cx, "locate, %d single rows" % len(x)):
        stored, hit, cnt = g.locate_raw(np.stack([x, x + 1], 1), 1)
    want1 = np.stack([s1, p1], 1)
    assert stored == len(x) and (cnt == 1).all() and np.array_equal(hit[:, 0], want1), first_bad(hit[:, 0], want1)


def whole_string_rank(m, ids):
    """the `$` rank of the whole-string row of the strings ids: head(z) = id"""
    q0, t = m.string_of(ids)
    k0 = np.full(len(m.texts0), -1, np.int64)
    rows = np.flatnonzero((m.pos0 == 0) & (m.bwt0 == 0))
    k0[m.sid0[rows]] = rows
    return m.occW[k0[q0], 0] + t


def test_string_ids(big):
    from test_overlap_gpu import string_ids_dev
    cx, m, g = big, big.m, big.g
    ssa(cx)
    n = m.n_strings
    ids = cx.mo.get("ids")
    z = whole_string_rank(m, ids)
    assert np.array_equal(m.head(z), ids)
    zv = [(int(a), int(a) + 1) for a in z]                          # ranges that name the ids around 2^24 and 2 x 2^24 ...
    zv += [(T24 - 3, T24 + 3), (2 * T24 - 3, 2 * T24 + 3), (0, 1000), (n - 2, n), (n, n), (5, 4), (-1, 2), (0, n + 1)]   # ... that cross them, wide, malformed
    w_stored, w_ids, w_cnt = m.string_ids_raw(zv, 8)
    assert (w_ids >= T24).sum() >= 50 and (w_ids >= 2 * T24).sum() >= 20 and w_cnt[-6:].tolist() == [1000, 2, 0, -1, -1, -1]
    with family(cx, "string_ids and _dev, %d ranges" % len(zv)):
        stored, got, cnt = g.string_ids_raw(zv, 8)
        dids, dcnt = string_ids_dev(g, zv, 8)
    assert stored == w_stored and np.array_equal(cnt, w_cnt) and np.array_equal(dcnt, w_cnt)
    assert np.array_equal(got, w_ids), first_bad(got, w_ids)
    live = np.arange(8)[None, :] < np.maximum(w_cnt, 0)[:, None]
    assert np.array_equal(dids[live], w_ids[live])


def test_find_and_overlaps(big):
    """end to end: backward search, then locate; overlap, then string_ids"""
    cx, m, g = big, big.m, big.g
    ssa(cx)
    pats, want = cx.mo.get("patterns")
    pick = np.concatenate([np.arange(0, 60), np.arange(300, 360), np.arange(len(pats) - 40, len(pats) - 4)])
    pp = [pats[i] for i in pick]
    w_find = [m.locate(lo, hi, 5)[0] if k == len(p) else np.zeros((0, 2), np.int64) for p, (lo, hi, k) in zip(pp, want[pick].tolist())]
    assert sum(len(w) and (w[:, 0] >= 2 * T24).any() for w in w_find) >= 10
    qs = [m.texts0[q] for q in np.unique(m.string_of(cx.mo.get("sources"))[0])]
    w_ov = []
    for q in qs:
        recs, _ = OV.overlap(m, q, 15)
        w_ov.append([(int(s), l) for l, zlo, zhi in recs.tolist()[::-1] for s in m.head(zlo + np.arange(min(zhi - zlo, 4)))])
    assert sum(1 for w in w_ov for s, _ in w if s >= 2 * T24) >= 10 and sum(1 for w in w_ov if w) >= len(w_ov) - 5
    with family(cx, "find, %d patterns, and overlaps, %d queries" % (len(pp), len(qs))):
        got = g.find(pp, 5)
        ov = g.overlaps(qs, 15, 4)
    for i, (a, b) in enumerate(zip(got, w_find)):
        assert np.array_equal(a, b), (pp[i].tolist(), a.tolist(), b.tolist())
    assert ov == w_ov


@pytest.mark.parametrize("min_ovlp", [1, 20])
def test_overlap(big, min_ovlp):
    from test_overlap_gpu import overlap_dev
    cx, m, g = big, big.m, big.g
    rng = np.random.RandomState(13)
    qs = list(m.texts0) + [rng.randint(1, 6, size=rng.randint(1, 60)).astype(np.uint8) for _ in range(30)]
    qs += [np.array([1, 0, 2], np.uint8), np.zeros(0, np.uint8)]
    cap = 256
    w_stored, w_rec, w_cnt = OV.overlap_raw(m, qs, min_ovlp, cap)
    live = np.arange(cap)[None, :] < np.maximum(w_cnt, 0)[:, None]
    assert w_cnt.max() <= cap and (w_rec[live][:, 2] >= 2 * T24).sum() >= 50 and (w_cnt > 0).sum() >= 50
    with family(cx, "overlap_raw and _dev, %d queries, min_ovlp %d" % (len(qs), min_ovlp)):
        stored, rec, cnt = g.overlap_raw(qs, min_ovlp, cap)
        drec, dcnt = overlap_dev(g, qs, min_ovlp, cap)
    assert stored == w_stored and np.array_equal(cnt, w_cnt) and np.array_equal(dcnt, w_cnt)
    assert np.array_equal(rec, w_rec), first_bad(rec, w_rec)
    assert np.array_equal(drec[live], w_rec[live])


@pytest.mark.parametrize("k", [1, 11, 32])
def test_kmers(big, k):
    cx, m, g = big, big.m, big.g
    wmin, wmax = int(m.wq.min()), int(m.wq.max())
    mid = wmax - 1                                                  # between the smallest and the largest weight, and above some counts
    cases = [(1, False), (mid, False), (m.N + 1, False)] + ([(1, True), (mid, True)] if cx.name == "even" else [])
    for min_occ, canon in cases:
        code, lo, hi, _ = KR.model(m, k, min_occ, canon)
        if min_occ == 1:
            assert (hi - lo).min() >= wmin and (canon or (lo >= T32).sum() >= (1 if k == 1 else 100)) and len(code) >= (4 if k == 1 else 1000) // (1 + canon)
        if min_occ > m.N:
            assert len(code) == 0
        with family(cx, "kmers, k %d, min_occ %d, canonical %d: %d k-mers" % (k, min_occ, canon, len(code))):
            gc, glo, ghi = g.kmers(k, min_occ, canon)
            hist = g.kmer_spectrum(k, 256, min_occ, canon)
        assert np.array_equal(gc, code) and np.array_equal(glo, lo) and np.array_equal(ghi, hi), (k, min_occ, canon)
        # every count is at least the smallest weight: the whole spectrum lands in the folded last bin
        assert np.array_equal(hist, KR.spectrum(hi - lo, 256)) and hist[255] == len(code) and hist[:255].sum() == 0
    if k > 1:
        n_mid = len(KR.model(m, k, mid, False)[0])
        assert 0 < n_mid < len(KR.model(m, k, 1, False)[0]), "min_occ between the smallest and the largest weight must drop some k-mers and keep some"


@pytest.mark.parametrize("max_mm", [1, 2])
def test_approx(big, max_mm):
    from test_approx_gpu import _sets, approx_dev
    cx, m, g = big, big.m, big.g
    rng = np.random.RandomState(14)
    qs = []
    for q0 in range(0, len(m.texts0), len(m.texts0) // 12):
        s = m.texts0[q0]
        q = s[:min(len(s), 18)].copy()
        q[rng.randint(len(q))] = rng.randint(1, 5)
        qs.append(q)
    t_lo = [s for s in m.D if (s[:12] == 4).any()][:4]             # matches that begin with T lie above 2^32
    qs += [s[int(np.flatnonzero(s == 4)[0]):][:16].copy() for s in t_lo] + [np.array([1, 0, 2], np.uint8)]
    cap = 512
    for min_occ in (1, int(m.wq.min()), int(m.wq.max()) * 4):      # min_occ in big units
        recs, w_cnt = AR.approx_raw(m, qs, max_mm, min_occ)
        assert w_cnt.max() <= cap and w_cnt[-1] == -1
        if min_occ == 1:
            assert sum(1 for r in recs[:-1] for lo, hi, _, _ in r if lo >= T32) >= 4 and (w_cnt > 0).sum() >= len(qs) - 2
        with family(cx, "approx and _dev, %d queries, max_mm %d, min_occ %d" % (len(qs), max_mm, min_occ)):
            stored, rec, cnt = g.approx_raw(qs, max_mm, min_occ, 1 << 16, cap)
            drec, dcnt = approx_dev(g, qs, max_mm, min_occ, 1 << 16, cap)
        assert np.array_equal(cnt, w_cnt) and np.array_equal(dcnt, w_cnt) and stored == np.maximum(w_cnt, 0).sum()
        assert _sets(rec, cnt, cap) == recs and _sets(drec, dcnt, cap) == recs


def test_contained(big):
    from test_contain_gpu import dev_records
    cx, m, g = big, big.m, big.g
    n = m.n_strings
    q0 = np.concatenate([[0, 1, 2], m.string_of(np.array([T24, 2 * T24, 3 * T24, n - 1]))[0], [len(m.wq) - 2]])
    ids = np.concatenate([m.start[q0], m.start[q0] + 1, m.start[q0 + 1] - 1, [n, -1, m.N]])     # copies t = 0, 1, last; ids that are no string
    assert (ids >= T24).sum() >= 12 and (ids >= 2 * T24).sum() >= 9 and ((ids < T24) & (ids >= 0)).sum() >= 6
    want = CR.contained(m, ids)
    k = len(q0)
    assert (want[:k, 0] & 1 == 0).all() and (want[k:3 * k, 0] & 1 == 1).all() and want[-3:, 0].tolist() == [-1, -1, -1]
    assert np.array_equal(want[2 * k:3 * k, 3], m.wq[q0] - 1) and np.array_equal(want[:3 * k, 2], np.tile(m.wq[q0], 3))
    with family(cx, "contained_raw and _dev, %d ids" % len(ids)):
        got = g.contained_raw(ids)
        dev = dev_records(g, len(ids), ids)
    assert np.array_equal(got, want), first_bad(got, want)
    assert np.array_equal(dev, want)


@EVEN_ONLY
def test_irreducible(big):
    cx, m, g = big, big.m, big.g
    ssa(cx)
    p = GRAPH
    src = cx.mo.get("sources")
    uq = np.unique(m.string_of(src)[0])
    qs = [m.texts0[q] for q in uq]
    want = [cx.mo.irreducible(int(q)) for q in uq]
    w_cnt = np.array([c for _, c in want])
    assert (w_cnt > 0).sum() >= len(uq) // 2 and sum(1 for r, _ in want for _, _, zlo, zhi in r if zhi > 2 * T24) >= 10
    w_py = [sorted((int(s), l, e) for l, e, zlo, zhi in r for s in m.head(zlo + np.arange(min(zhi - zlo, p["max_hits"])))) for r, _ in want]
    assert sum(1 for w in w_py for s, _, _ in w if s >= 2 * T24) >= 10
    with family(cx, "irreducible, %d queries" % len(qs)):
        stored, rec, cnt = g.irreducible_raw(qs, p["min_ovlp"], p["max_ext"], p["max_steps"], p["max_recs"])
        py = g.irreducible(qs, p["min_ovlp"], p["max_ext"], p["max_steps"], p["max_recs"], p["max_hits"], pairs=False)
    assert np.array_equal(cnt, w_cnt) and stored == w_cnt.sum()
    for i, (r, c) in enumerate(want):
        assert sorted(map(tuple, rec[i, :c].tolist())) == sorted(r) and (rec[i, c:] == 0).all(), int(uq[i])
    assert py == w_py


@EVEN_ONLY
def test_string_graph(big):
    from test_graph_gpu import graph_dev
    cx, m, g = big, big.m, big.g
    ssa(cx)
    total = over = 0
    for first, n in cx.mo.get("ranges"):
        want, wide = cx.mo.edges(first, n)
        total += len(want)
        over += int((want[:, 1] >= 2 * T24).sum())
        with family(cx, "string_graph and _dev, sources %d .. %d: %d edges" % (first, first + n - 1, len(want))):
            edges, info = g.string_graph(first, n, pairs=False, **GRAPH)
            dm, dinfo, rows = graph_dev(g, first, n, len(want), GRAPH, 0)
        assert info.tolist() == [len(want), len(want), 0, wide, 0, 0, 0, 0] and dinfo.tolist() == info.tolist() and dm == len(want)
        assert (np.diff(edges[:, 0]) >= 0).all() and np.array_equal(_sorted(edges), want), (first, n)
        assert np.array_equal(_sorted(rows[:dm]), want), (first, n)
    assert total >= 200 and over >= 50, "edges, and edges to a string id >= 2 x 2^24"


def test_fmd_image(big, tmp_path):
    """the encoder on the big index, and the loader on its image: save_fmd() is the host writer's image of the model's runs, and a handle
    that loads the image holds the ropes the run bytes gave"""
    cx, m, g = big, big.m, big.g
    img = write_fmd(tmp_path / "big.fmd", pushes=cx.mo.S)
    with family(cx, "save_fmd, %d bytes, and load_fmd" % len(img)):
        got = g.save_fmd()
        b = cx.hip.HipBwt(1)
        loaded = b.load_fmd(img)
        hashes, cnt = b.rope_hashes(), b.counts()
        b.close()
    assert len(got) == len(img) and np.array_equal(got, img)
    assert loaded == m.N and hashes == cx.hashes0 and np.array_equal(cnt, cx.counts0)


def test_queries_changed_nothing(big):
    cx = big
    with family(cx, "a few queries of every kind"):
        cx.g.extend(np.array([[T32, T32, 1]], np.int64), 1)
        cx.g.backward_search([cx.m.D[0]])
        cx.g.extract([T24], 200)


# ---- mutating tests, each on its own load --------------------------------------------------------------------------------------------------

def check_after(g, m2, pats, tmp, what):
    """what an index must answer after a change: counts, ranks at every block start of the new model, the backward searches, and its image"""
    assert np.array_equal(g.counts(), W.counts(m2)), what
    check_ranks(g, m2)
    want = np.array([m2.interval(p) for p in pats], np.int64).reshape(-1, 3)
    assert np.array_equal(_check_search(g, _Shim(m2), pats), want)
    assert (want[:, 0] >= T32).sum() >= 100
    img = write_fmd(tmp / "want.fmd", pushes=m2.runs())
    got = g.save_fmd()
    assert len(got) == len(img) and np.array_equal(got, img), "%s: save_fmd() is not the host writer's image of the model's runs" % what


@pytest.mark.parametrize("name", ["even", "skewed"])
def test_delete(hip, models, tmp_path, name):
    """for twenty strings some copies go, always t = 0 and the last, which leaves the ids non-contiguous; for one string all copies go"""
    t0 = time.time()
    mo, tmp = models(name), tmp_path
    m = mo.m
    rng = np.random.RandomState(15)
    q0 = np.unique(np.concatenate([[0, len(m.wq) - 1], m.string_of(np.array([T24, 2 * T24]))[0], rng.choice(len(m.wq), 18, replace=False)]))
    gone = int(q0[3])                                               # one string loses every copy
    ids, w2 = [], m.wq.copy()
    for q in q0.tolist():
        w = int(m.wq[q])
        t = np.arange(w) if q == gone else np.unique(np.concatenate([[0, w - 1], rng.randint(0, w, size=40)]))
        ids.append(m.start[q] + t)
        w2[q] -= len(t)
    ids = np.concatenate(ids)
    ids = ids[rng.permutation(len(ids))]
    assert (ids >= 2 * T24).sum() >= 40 and (ids < T24).sum() >= 40 and w2[gone] == 0 and (w2 >= 0).all()
    wD = np.zeros(len(m.D), np.int64)
    wD[m.d_of_q] = w2
    m2 = m.reweighted(wD)
    rows = int(sum((len(m.texts0[q]) + 1) * (m.wq[q] - w2[q]) for q in q0))
    assert m2.N == m.N - rows and m2.N > T32 and m2.n_strings == m.n_strings - len(ids)
    free0 = mem_info(hip)[0]
    g = load(hip, mo)
    t1 = time.time()
    assert g.delete(ids) == rows
    t2, used = time.time(), free0 - mem_info(hip)[0]
    check_after(g, m2, mo.get("patterns")[0], tmp, "delete")
    g.close()
    print("TIMING %s delete: %d strings, %d rows: model and load %.2f s, delete %.2f s, checks %.2f s; %.2f GiB of device memory behind the delete" % (
        mo.name, len(ids), rows, t1 - t0, t2 - t1, time.time() - t2, used / GIB))


ENVS = {"default": {}, "lambda0": dict(RB2_SPARSE_LAMBDA="0"), "forced": FORCED}


@pytest.mark.parametrize("env", sorted(ENVS))
@pytest.mark.parametrize("name", ["even", "skewed"])
def test_insert(hip, models, tmp_path, name, env):
    """a shuffled batch of extra copies of twenty strings, the shortest and the longest among them, into the loaded index: even with
    every piece below 2^32 symbols, skewed with piece (A,A) above (wide positions)"""
    t0 = time.time()
    mo = models(name)
    m = mo.m
    rng = np.random.RandomState(16)
    lens = np.array([len(s) for s in m.D])
    d = np.unique(np.concatenate([[int(lens.argmin()), int(lens.argmax())], rng.choice(len(m.D), 18, replace=False)]))
    add = np.zeros(len(m.D), np.int64)
    add[d] = rng.randint(5, 30, size=len(d))
    batch = W.copies(m.D, add)
    batch = [batch[i] for i in rng.permutation(len(batch))]
    assert 200 <= len(batch) <= 600
    m2 = m.reweighted(m.weights() + add)
    _, size = W.piece_rows(m)
    assert (size.max() > T32) == (name == "skewed")
    free0 = mem_info(hip)[0]
    with _Env(**ENVS[env]):
        g = load(hip, mo)
        t1 = time.time()
        g.insert_multi(H.encode_batch(batch, True, False))
        g.wait()
        t2, used = time.time(), free0 - mem_info(hip)[0]
        st = g.layout_stats()
        if env == "forced":
            assert st["sparse_now"], st
        check_after(g, m2, mo.get("patterns")[0], tmp_path, "insert (%s)" % env)
        g.close()
    print("TIMING %s insert (%s): %d strings, %d symbols: model and load %.2f s, insert %.2f s, checks %.2f s; %.2f GiB of device memory behind the insert; layout %s" % (
        name, env, len(batch), m2.N - m.N, t1 - t0, t2 - t1, time.time() - t2, used / GIB, st))


@pytest.mark.parametrize("name", ["even", "skewed"])
def test_merge(hip, models, tmp_path, name):
    """a small source handle holds the same D with weights 0 .. 3: merging it into the big destination adds the weights"""
    t0 = time.time()
    mo = models(name)
    m = mo.m
    add = np.random.RandomState(17).randint(0, 4, size=len(m.D))
    assert (add == 0).sum() >= 10 and (add == 3).sum() >= 10
    ms = m.reweighted(add)
    m2 = m.reweighted(m.weights() + add)
    free0 = mem_info(hip)[0]
    src = hip.HipBwt(1)
    src.load_ropes(F.cut(ms.runs()))
    dst = load(hip, mo)
    t1 = time.time()
    info = dst.merge(src)
    t2, used = time.time(), free0 - mem_info(hip)[0]
    assert info[0] == add.sum() and info[1] == ms.N - ms.n_strings, info
    assert np.array_equal(src.counts(), W.counts(ms))
    check_after(dst, m2, mo.get("patterns")[0], tmp_path, "merge")
    src.close(); dst.close()
    print("TIMING %s merge: %d strings: model and load %.2f s, merge %.2f s, checks %.2f s; %.2f GiB of device memory behind the merge" % (
        name, info[0], t1 - t0, t2 - t1, time.time() - t2, used / GIB))
