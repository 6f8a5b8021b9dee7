"""GPU tests of the FM-index queries (k_bsearch, k_extend, k_extract, k_smem: csrc/rb2_query.h) on the layouts where all four terms of
qrank() -- the piece's counts in front, the superblocks of the piece in front, the leaves of the superblock in front (LeafMeta or the
directory prefix), the popcount inside the leaf -- carry part of the answer:

  D  dense, every piece (b,x), b, x in A..T, longer than two superblocks; both strands; input order and RCLO
  L  the BWT of D loaded into a fresh handle: from run bytes (load_ropes) and from an .fmd image (load_fmd)
  S  sparse, grown in place under RLO until leaves were split into their superblocks' reserve slots and superblocks were re-spread

Every result must equal the numpy reference (tests/query_ref.py, tests/smem_ref.py) on the oracle's BWT of the same strings.  The rank
sweep asks k_extend for the ranks of EVERY row and every row + 1 (D in input order and S; a stride of 3 elsewhere), and extracting every
string reads every symbol of the BWT exactly once (query_ref.FM.walk_all)."""
from contextlib import contextmanager

import numpy as np
import pytest

import helpers as H
import query_ref as Q
import smem_ref as S
from ropebwt2_amd.hipbwt import encode_runs, pack_patterns
from test_fmd_load_gpu import write_fmd
from test_query_gpu import _Env, _chains, _patterns
from test_smem_gpu import MALFORMED, _compare, _queries

pytestmark = pytest.mark.gpu
FORCED = dict(RB2_SPARSE_LAMBDA="1e18", RB2_SPARSE_MAXPEN="0")       # every batch in place: the sparse layout (test_leaf_split_gpu.py)
SMEM_PARAMS = [(1, 1), (17, 1), (5, 3)]                              # (min_len, min_occ)
CHUNK = 1 << 19                                                      # bi-intervals per rb2_hip_extend call of a sweep (72 MiB of results)
WIDE = (1025, 40000)                                                 # interval sizes whose two ranks fall in different leaves / superblocks


class _Model:
    """the CPU side of an index: the strings, the oracle's BWT of them, the reference over it, and the query sets with the reference's
    answers, each computed once however many handles are held against it.  parts: the batches, each inserted as both strands; extra: one
    more batch, inserted behind them only to know the BWT an index must hold after it (bwt_after)."""
    def __init__(self, so, parts, seed, extra=None):
        self.so, self.seed = so, seed
        self.batches = [H.encode_batch_fixed(p, True, True) if isinstance(p, np.ndarray) else H.encode_batch(p, True, True) for p in parts]
        self.strings = [s for p in parts for s in Q.inserted_strings(p, True, True)]
        o = H.Oracle(so)
        for b in self.batches:
            o.insert_multi(b)
        self.ropes, self.counts = o.ropes(), o.counts()
        self.extra, self.bwt_after = extra, None
        if extra is not None:
            o.insert_multi(extra)
            self.bwt_after = o.bwt()
        o.close()
        self.bwt = np.concatenate(self.ropes)
        self.fm = Q.FM(self.bwt)
        self.memo = {}

    def get(self, what):
        if what not in self.memo:
            self.memo[what] = getattr(self, "_" + what)()
        return self.memo[what]

    def piece_rows(self):
        """first global row of each of the 31 pieces: rope $, then (b,x) = the b's of rope x in the order of x"""
        rows = [0]
        for b in range(1, 6):
            row = int(self.fm.C[b])
            for x in range(6):
                rows.append(row)
                row += int(self.counts[x, b])
        return np.array(rows, np.int64)

    def _sweep(self):
        """[x, x, 1] for every row x (the same array serves both directions) and [N, N, 0]; the wide intervals around every piece's first row"""
        N = self.fm.N
        wide = [[min(max(r0 + d, 0), N - sz)] * 2 + [sz] for r0 in self.piece_rows() for d in (-1, 0, 1) for sz in WIDE if sz <= N]
        return np.array([[N, N, 0]] + wide, np.int64)

    def _patterns(self):
        rng = np.random.RandomState(self.seed)
        pats = []
        for _ in range(1200):                                       # substrings of the strings, lengths 1..100
            s = self.strings[rng.randint(len(self.strings))]
            a = rng.randint(len(s))
            pats.append(s[a:a + rng.randint(1, 101)].copy())
        pats += [rng.randint(1, 6, size=rng.randint(1, 101)).astype(np.uint8) for _ in range(400)]   # random
        pats += [np.concatenate([p, [0]]).astype(np.uint8) for p in pats[:200]]                       # trailing $ ...
        for _ in range(200):                                        # ... and suffixes of strings with it: these do occur
            s = self.strings[rng.randint(len(self.strings))]
            pats.append(np.concatenate([s[len(s) - rng.randint(1, 101):], [0]]).astype(np.uint8))
        pats += _patterns(self.strings, rng, k=0)[-6:]              # the empty pattern, `$`, the malformed ones
        want = np.array([self.fm.backward_search(p) for p in pats], np.int64).reshape(-1, 3)
        full = want[:, 2] == [len(p) for p in pats]
        assert full[:1200].all() and (want[:1200, 1] > want[:1200, 0]).all()         # substrings occur ...
        assert full[1800:2000].all() and (~full[1200:1600]).sum() > 300             # ... suffixes with `$` too; long random patterns do not
        assert (want[-6:, 2] == [0, 1, -1, -1, -1, -1]).all(), want[-6:]
        return pats, want

    def _chains(self):
        fm = self.fm
        iks, qs = _chains(fm, self.strings, np.random.RandomState(self.seed + 1))
        assert len(iks) > 1000
        for ik, q in zip(iks, qs):                                  # x[0] = lo(Q), x[1] = lo(revcomp Q), x[2] = count(Q)
            lo, hi, m = fm.backward_search(q)
            assert m == len(q) and ik.tolist() == [lo, fm.backward_search(Q.revcomp(q))[0], hi - lo], q
        return iks

    def _smem(self):
        qs = [q[:100] for q in _queries(self.strings, np.random.RandomState(self.seed + 2), k=100)]
        tabs = [None if S.malformed(q) else S.occ_table(self.fm, q) for q in qs]
        want = {p: [None if t is None else S.smems_from_table(self.fm, q, t, *p) for q, t in zip(qs, tabs)] for p in SMEM_PARAMS}
        w11 = [w for w in want[1, 1] if w is not None]
        assert len(qs) - len(w11) == len(MALFORMED)
        assert sum(1 for w in w11 if len(w) >= 2) >= 20 and sum(1 for w in w11 if len(w) and (w[:, 4] > 1).any()) >= 20
        for p in SMEM_PARAMS[1:]:                                   # the stricter pairs still find matches, and other ones
            ws = [w for w in want[p] if w is not None]
            assert sum(len(w) for w in ws) >= 10 and sum(1 for a, b in zip(ws, w11) if not np.array_equal(a, b)) >= 20, p
        return qs, want

    def _walks(self):
        walked, visits = self.fm.walk_all()
        assert (visits == 1).all()                                  # extracting every string reads every row of the BWT once
        return [w.tobytes() for w in walked]


class _Idx:
    def __init__(self, name, g, m, stride, sparse):
        self.name, self.g, self.m, self.stride, self.sparse = name, g, m, stride, sparse
        self.stats0 = g.layout_stats()
        assert self.stats0["sparse_now"] == sparse
        self.hashes0 = None if sparse else g.rope_hashes()          # (a checksum makes a sparse index dense: S is checked at the end)


@contextmanager
def _unchanged(ix):
    """a query must leave the index and its layout as they were"""
    yield
    assert ix.g.layout_stats() == ix.stats0, "a query changed the layout"
    if not ix.sparse:
        assert ix.g.rope_hashes() == ix.hashes0, "a query changed the index"


def _dense_model(so):
    codes = H.splitmix_bases(9000, 100, seed=77)
    return _Model(so, [codes[:4500], codes[4500:]], seed=so)


def _n_reads(rng, n, lo, hi):
    """reads with runs of N (leaves that need their third bit plane)"""
    out = []
    for _ in range(n):
        r = rng.randint(1, 5, size=int(rng.randint(lo, hi))).astype(np.uint8)
        for _ in range(int(rng.randint(1, 3))):
            at = int(rng.randint(0, len(r) - 1))
            r[at:at + int(rng.randint(1, 300))] = 5
        out.append(r)
    return out


# reads x length of the first batch, of the two batches that multiply the index, and of the last, which adds 22 % (measured behind these
# batches: 235 reads split 8 leaves, 250 split 37, 270 split 171, 275 used up a superblock's reserve slots and ended in a re-spread)
S_FIRST, S_REST, S_TOP = (150, 400), (260, 1500), (250, 400)


def _sparse_model():
    rng = np.random.RandomState(3)
    rest = list(H.splitmix_bases(*S_REST, seed=5))
    half = len(rest) // 2
    parts = [list(H.splitmix_bases(*S_FIRST, seed=4)), rest[:half] + _n_reads(rng, 4, 900, 1500), rest[half:] + _n_reads(rng, 4, 900, 1500),
             list(H.splitmix_bases(*S_TOP, seed=6))]
    return _Model(1, parts, seed=5, extra=H.encode_batch(H.repetitive_reads(150, seed=12, max_len=40), True, True))


class _Models:
    """the models of this module, each built when first asked for and dropped with the module (a dense one holds some 200 MB)"""
    def __init__(self):
        self.made = {}

    def get(self, key):
        if key not in self.made:
            self.made[key] = _sparse_model() if key == "S" else _dense_model(key)
        return self.made[key]


@pytest.fixture(scope="module")
def models():
    ms = _Models()
    yield ms
    ms.made.clear()


def _build_dense(hip, m):
    so = m.so
    g = hip.HipBwt(so)
    for b in m.batches:
        g.insert_multi(b)
    cnt = g.counts()
    assert np.array_equal(cnt, m.counts)
    assert (cnt[1:5, 1:5] > 2 * 32 * hip.HipBwt.layout()["leaf_syms"]).all(), cnt     # every piece (b,x), b, x in A..T: at least three superblocks
    assert not g.layout_stats()["sparse_now"]
    assert np.array_equal(g.bwt(), m.bwt)
    return _Idx("D so=%d" % so, g, m, 1 if so == 0 else 3, False)


def _build_loaded(hip, m, how, tmp):
    if "rles" not in m.memo:
        m.memo["rles"] = [encode_runs(r) for r in m.ropes]
    g = hip.HipBwt(0)
    if how == "ropes":
        g.load_ropes(m.memo["rles"])
    else:
        assert g.load_fmd(write_fmd(tmp / "d.fmd", m.memo["rles"])) == m.fm.N
    assert np.array_equal(g.counts(), m.counts)
    assert np.array_equal(g.bwt(), m.bwt)
    return _Idx("L " + how, g, m, 3, False)


def _build_sparse(hip, m):
    """each of the two big batches multiplies the index: leaves split, superblocks run out of reserve slots and are re-spread.  The last
    batch is small: it splits leaves, and no re-spread and no void round follows (its two re-layouts are the dense rounds at the head of
    every batch, in front of its in-place rounds), so the queries find split leaves in the reserve slots."""
    with _Env(**FORCED):
        g = hip.HipBwt(1)
    st = []
    for b in m.batches:
        g.insert_multi(b)
        st.append(g.layout_stats())
    print("sparse fixture: %d symbols, after each batch:" % m.fm.N, [(s["leaf_splits"], s["respreads"], s["relayouts"], s["void_rounds"]) for s in st])
    assert st[-1]["sparse_now"] and st[-1]["leaf_splits"] > 0 and st[-1]["respreads"] > 0, st
    # split leaves must still sit in reserve slots when the queries run: the last batch split some, and nothing re-laid the index out behind
    # its in-place rounds.  If a change of the engine's layout policy trips this, resize S_TOP until the last batch splits leaves again
    # without a re-spread; do not drop the condition.
    last = {k: st[-1][k] - st[-2][k] for k in ("leaf_splits", "respreads", "void_rounds", "relayouts")}
    assert last["leaf_splits"] > 0, "the last batch split no leaf: %s" % last
    assert last["respreads"] == 0 and last["void_rounds"] == 0, "a re-spread or a void round in the last batch may have undone its splits: %s" % last
    assert last["relayouts"] <= 2, "more re-layouts in the last batch than the two around the dense rounds at its head: %s" % last
    assert np.array_equal(g.counts(), m.counts)
    return _Idx("S", g, m, 1, True)


@pytest.fixture(scope="module", params=["D-io", "D-rclo", "L-ropes", "L-fmd", "S"])
def idx(request, hip, models, tmp_path_factory):
    kind = request.param
    if kind.startswith("D"):
        ix = _build_dense(hip, models.get(0 if kind == "D-io" else 2))
    elif kind.startswith("L"):
        ix = _build_loaded(hip, models.get(0), kind[2:], tmp_path_factory.mktemp("layouts"))
    else:
        ix = _build_sparse(hip, models.get("S"))
    yield ix
    ix.g.close()


def _piece_of(m, row):
    r = int(np.searchsorted(m.piece_rows(), row, side="right")) - 1
    return "piece %d (%s,%s) + %d" % (r, "$ACGTN"[H.rope_sym(r)], "$ACGTN"[H.rope_prev(r)], row - m.piece_rows()[r])


def _extend_equal(ix, iks):
    fm = ix.m.fm
    for is_back in (1, 0):
        for i0 in range(0, len(iks), CHUNK):
            part = iks[i0:i0 + CHUNK]
            got, want = ix.g.extend(part, is_back), fm.extend_many(part, is_back)
            if not np.array_equal(got, want):
                bad = np.flatnonzero((got != want).reshape(len(part), -1).any(1))
                i = bad[0]
                fb = 0 if is_back else 1
                pytest.fail("%s, is_back=%d: %d of %d bi-intervals differ; first %s: ranks at %s and %s\n got %s\nwant %s" % (
                    ix.name, is_back, len(bad), len(part), part[i].tolist(), _piece_of(ix.m, part[i, fb]), _piece_of(ix.m, part[i, fb] + part[i, 2]),
                    got[i].tolist(), want[i].tolist()))


def test_rank_sweep_through_extend(idx):
    """the ranks of every row x and x + 1 ([x, x, 1], backward and forward): every leaf, every 64-symbol group edge, every leaf's last
    filled position, every superblock edge; wide intervals put the two ranks of one query in different leaves and superblocks"""
    fm = idx.m.fm
    rows = np.arange(0, fm.N, idx.stride, dtype=np.int64)
    extra = idx.m.get("sweep")
    assert len(extra) == 1 + 31 * 3 * len(WIDE)
    with _unchanged(idx):
        _extend_equal(idx, np.concatenate([np.stack([rows, rows, np.ones_like(rows)], 1), extra]))


def test_extract_everything(idx):
    """every string by LF steps: qrank(..., &sym) on every row of the BWT"""
    g, m = idx.g, idx.m
    want = m.get("walks")
    n = int(m.fm.C[1])
    assert n == len(m.strings) == len(want)
    with _unchanged(idx):
        got = [s.tobytes() for s in g.extract(np.arange(n), max(len(s) for s in m.strings))]
    bad = [k for k in range(n) if got[k] != want[k]]
    assert not bad, (idx.name, len(bad), bad[:5])
    mine = [np.asarray(s, np.uint8).tobytes() for s in m.strings]
    if m.so == 0:
        assert got == mine
    else:
        assert sorted(got) == sorted(mine)
    if m.so == 1:                                                   # RLO: the strings come out in reverse-lexicographic order
        rk = [s[::-1] for s in got]
        assert rk == sorted(rk)


def test_backward_search(idx):
    g, m = idx.g, idx.m
    pats, want = m.get("patterns")
    n = len(pats)
    with _unchanged(idx):
        got = np.stack(g.backward_search(pats), 1)
        pat, off = pack_patterns(pats)                              # the same through the device-pointer variant
        res = np.zeros((n, 3), np.int64)
        dp, do, dq = g.dev_alloc(len(pat)), g.dev_alloc(8 * (n + 1)), g.dev_alloc(24 * n)
        try:
            g.L.rb2_hip_memcpy(g.h, dp, pat.ctypes.data, len(pat), 0)
            g.L.rb2_hip_memcpy(g.h, do, off.ctypes.data, 8 * (n + 1), 0)
            g.backward_search_dev(n, dp, do, dq)
            g.L.rb2_hip_memcpy(g.h, res.ctypes.data, dq, 24 * n, 1)
        finally:
            for p in (dp, do, dq):
                g.dev_free(p)
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, (idx.name, [(pats[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:3]])
    assert np.array_equal(res, want)


def test_extend_chains(idx):
    """bi-intervals reached by chains of backward and forward extensions; the model holds ik == [lo(Q), lo(revcomp Q), count(Q)]"""
    with _unchanged(idx):
        _extend_equal(idx, idx.m.get("chains"))


@pytest.mark.parametrize("min_len,min_occ", SMEM_PARAMS)
def test_smems_match_model(idx, min_len, min_occ):
    qs, want = idx.m.get("smem")
    with _unchanged(idx):
        stored, mem, cnt = idx.g.smem_raw(qs, min_len, min_occ, 64)
    _compare(type("C", (), {"qs": qs}), want[min_len, min_occ], stored, mem, cnt, 64, 0)


def test_queries_changed_nothing(idx):
    """the checksums and the layout of the fixture are those it was built with, whichever of the tests above ran before (each of them
    checks the same behind its own queries); a few queries of every kind here, so that the test means something on its own.  The
    checksums of the sparse index cannot be taken (a checksum leaves the sparse layout): see the test below"""
    g, m = idx.g, idx.m
    with _unchanged(idx):
        g.extend(m.get("sweep"), 1)
        g.extract(np.arange(64), 1)
        g.backward_search(m.strings[:64])
        g.smem_raw(m.strings[:16])


def test_sparse_index_takes_a_batch_after_queries(hip, models):
    """in place of checksums before and after: a sparse index of its own (the one of S again) answers queries of every kind, is still
    sparse, takes one more both-strand batch in place and then holds the oracle's BWT of all batches"""
    m = models.get("S")
    ix = _build_sparse(hip, m)
    g = ix.g
    with _unchanged(ix):
        rows = np.arange(0, m.fm.N, 3, dtype=np.int64)
        _extend_equal(ix, np.concatenate([np.stack([rows, rows, np.ones_like(rows)], 1), m.get("sweep")]))
        g.extract(np.arange(64), 1500)
        g.backward_search(m.strings[:64])
        g.smem_raw([s[:100] for s in m.strings[:16]])
    g.insert_multi(m.extra)
    assert g.layout_stats()["sparse_now"]
    assert np.array_equal(g.bwt(), m.bwt_after)
    g.close()
