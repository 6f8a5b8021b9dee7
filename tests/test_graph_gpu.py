"""GPU tests of the string graph on the device (include/rb2_hip.h: rb2_hip_string_graph[_dev]; kernels in csrc/rb2_graph.h, the chunks in
csrc/rb2_graph_plan.h) and of HipBwt.string_graph / assemble.  The truth is HipBwt.edges() of the same index -- the host composition of
extract, irreducible and string_ids the call replaces --, rows compared as sorted arrays.  Equality is owed where no source is cut short:
every equality case first follows every source through the model (tests/irreducible_ref.py on the BWT the index holds) and asserts that
none finds more than max_recs records, none has a range wider than max_hits and none runs out of max_steps; info[2:6] must then be 0.
Where a source is cut short, the counters must be those irreducible_raw reports and every stored row a row of the untruncated run."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import irreducible_ref as IR
import query_ref as Q
import unitig_ref as U
from test_query_gpu import _Env
from test_query_layouts_gpu import _Models, _build_dense, _build_sparse
from test_unitig_gpu import _Tile, _as_lists

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILL = -7                                                            # what the calls must leave where they store nothing
P = dict(min_ovlp=U.MIN_OVLP, max_ext=64, max_steps=1 << 16, max_recs=16, max_hits=8)
WIDE = dict(max_steps=1 << 20, max_recs=64, max_hits=64)             # the untruncated run of the truncation cases


def _sorted(rows):
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    return rows[np.lexsort(rows.T[::-1])]


class _Ix:
    """an index with its suffix array, its strings by id (unpack), the model of its BWT, and the truth, computed once per question"""
    def __init__(self, g, fm=None):
        self.g = g
        self.n = g._n_strings()
        if not g.ssa_info()["valid"]:
            g.build_ssa(2)
        self.strings = g.unpack()
        self.fm = fm
        self.memo = {}

    def model(self):
        if self.fm is None:
            self.fm = Q.FM(self.g.bwt())
        return self.fm

    def owed(self, first, n, p):
        """equality is owed for these sources: the model finds none of them cut short by max_recs, max_hits, max_steps or its length"""
        key = ("owed", first, n, tuple(sorted(p.items())))
        if key not in self.memo:
            fm = self.model()
            for s in range(first, first + n):
                q = self.strings[s]
                assert len(q) <= IR.MAX_LEN, s
                recs, cnt, _ = IR.irreducible(fm, q, p["min_ovlp"], p["max_ext"], p["max_steps"])
                assert 0 <= cnt <= p["max_recs"], "source %d: cnt %d" % (s, cnt)
                assert all(zhi - zlo <= p["max_hits"] for _, _, zlo, zhi in recs), "source %d: a range wider than max_hits" % s
            self.memo[key] = True
        return True

    def truth(self, first, n, p, pairs):
        """HipBwt.edges() of the sources, sorted"""
        key = ("edges", first, n, tuple(sorted(p.items())), pairs)
        if key not in self.memo:
            self.memo[key] = _sorted(self.g.edges(np.arange(first, first + n), pairs=pairs, **p))
            self.memo[key].setflags(write=False)
        return self.memo[key]


def graph_dev(g, first, n, cap, p, pairs, null=False):
    """string_graph_dev on a buffer of cap + 2 rows filled with FILL: (m, info, the whole buffer as the device left it)"""
    rows = np.full((cap + 2, 4), FILL, np.int64)
    d = g.dev_alloc(rows.nbytes)
    try:
        g.L.rb2_hip_memcpy(g.h, d, rows.ctypes.data, rows.nbytes, 0)
        m, info = g.string_graph_dev(first, n, None if null else d, cap, pairs=pairs, **p)
        g.L.rb2_hip_memcpy(g.h, rows.ctypes.data, d, rows.nbytes, 1)
    finally:
        g.dev_free(d)
    assert m == info[0] and info[1] == min(m, cap) and (info[6:] == 0).all(), (m, info)
    assert (rows[min(m, cap):] == FILL).all(), "something was written behind the rows stored"
    return m, info, rows


def _equal(ix, first, n, p, pairs):
    """host and device variant against the truth; returns the truth"""
    assert ix.owed(first, n, p)
    want = ix.truth(first, n, p, pairs)
    edges, info = ix.g.string_graph(first, n, pairs=pairs, **p)
    print("string_graph(%d, %d, pairs=%d): %d edges, info %s" % (first, n, pairs, len(edges), info.tolist()))
    assert info.tolist() == [len(want), len(want), 0, 0, 0, 0, 0, 0]
    assert (np.diff(edges[:, 0]) >= 0).all(), "the rows do not come in increasing src"
    assert np.array_equal(_sorted(edges), want), "host variant"
    m, d_info, rows = graph_dev(ix.g, first, n, len(want), p, pairs)
    assert m == len(want) and d_info.tolist() == info.tolist()
    assert (np.diff(rows[:m, 0]) >= 0).all() and np.array_equal(_sorted(rows[:m]), want), "device variant"
    return want


@pytest.fixture(scope="module")
def tiles(hip):
    made = {}

    def get(name, circular=False):
        if (name, circular) not in made:
            t = _Tile(hip, name, circular)
            t.ix = _Ix(t.g)
            made[name, circular] = t
        return made[name, circular]
    yield get
    for t in made.values():
        t.g.close()


# ---- equality on small indexes ----

@pytest.mark.parametrize("pairs", [0, 1])
@pytest.mark.parametrize("name", sorted(U.TILES))
def test_tiles(tiles, name, pairs):
    """the reduced index of both strands of reads that tile a genome: every string a source"""
    t = tiles(name)
    want = _equal(t.ix, 0, t.n, P, pairs)
    assert len(want) == U.TILES[name][2]
    if pairs:
        assert want.tolist() == [list(r) for r in U.brute_edges(t.strings, P["min_ovlp"], P["max_ext"])]


@pytest.mark.parametrize("first,n", [(37, 61), (1, 1), (155, 1), (0, 0), (156, 0)])
def test_sub_range(tiles, first, n):
    """sources that start and end inside the index; one source; the last one; none"""
    t = tiles("repeat")
    want = _equal(t.ix, first, n, P, 1)
    assert len(want) > 50 or n <= 1
    assert not len(want) or (want[0, 0] >= first and want[-1, 0] < first + n)


def _mixed_reads():
    """tiled reads with, between them: an empty read, two reads with N, and a read that overlaps nothing"""
    _, reads = U.tile_reads(seed=11, glen=300, lo=40, hi=40, smax=5)
    rng = np.random.RandomState(12)
    loner = rng.randint(1, 5, size=45).astype(np.uint8)
    n_in = reads[20].copy()
    n_in[15] = 5                                                     # an N in the middle: the overlaps end in front of it
    n_end = np.concatenate([reads[30][:30], np.array([5], np.uint8)])   # an N at the end: no suffix to speak of
    return reads[:10] + [np.zeros(0, np.uint8)] + reads[10:25] + [loner] + reads[25:] + [n_in, n_end]


@pytest.fixture(scope="module")
def mixed(hip):
    g = hip.HipBwt(0)
    reads = _mixed_reads()
    half = len(reads) // 2
    for part in (reads[:half], reads[half:]):
        g.insert_multi(H.encode_batch(part, True, True))
    ix = _Ix(g)
    yield ix
    g.close()


@pytest.mark.parametrize("pairs", [0, 1])
def test_empty_string_n_and_a_loner(mixed, pairs):
    ix = mixed
    assert len(ix.strings[20]) == 0 and len(ix.strings[21]) == 0
    want = _equal(ix, 0, ix.n, P, pairs)
    srcs = set(want[:, 0].tolist())
    loner = 2 * 26                                                   # 10 reads, the empty one, 15 reads: read 26
    assert loner not in srcs and loner - 2 in srcs and loner + 2 in srcs, "no source without an edge between two with edges"
    assert 20 not in srcs and 21 not in srcs and len(want) > 100
    assert len(_equal(ix, loner, 1, P, pairs)) == 0                  # one source, no edge
    three = _equal(ix, loner - 2, 3, P, pairs)                       # three sources, the last one without an edge
    assert len(three) and set(three[:, 0].tolist()) <= {loner - 2, loner - 1}


@pytest.fixture(scope="module")
def models():
    ms = _Models()
    yield ms
    ms.made.clear()


@pytest.mark.parametrize("kind", ["D", "S"])
def test_layouts(hip, models, kind):
    """a range of sources inside layout D (dense, every piece longer than two superblocks; input order, so with pairs too) and layout S
    (sparse, split leaves; strings of up to 1500 symbols with runs of N) of test_query_layouts_gpu.py"""
    ix0 = _build_dense(hip, models.get(0)) if kind == "D" else _build_sparse(hip, models.get("S"))
    try:
        ix = _Ix(ix0.g, ix0.m.fm)
        before = ix.g.layout_stats()
        first, n, p = (1000, 400, dict(P, min_ovlp=7, max_ext=100)) if kind == "D" else (300, 60, dict(P, min_ovlp=5, max_ext=1500))
        for pairs in ((0, 1) if kind == "D" else (0,)):
            want = _equal(ix, first, n, p, pairs)
            assert len(want) > 40, len(want)
        assert ix.g.layout_stats() == before, "the call changed the layout"
    finally:
        ix0.g.close()


def test_pairs_needs_input_order(hip):
    g = hip.HipBwt(1)
    try:
        g.insert_multi(H.encode_batch(H.repetitive_reads(10, seed=3), True, True))
        g.build_ssa(2)
        with pytest.raises(ValueError):
            g.string_graph(pairs=True)
        with pytest.raises(ValueError):
            g.assemble(5)
    finally:
        g.close()


# ---- chunking ----

@pytest.mark.parametrize("env", [dict(RB2_GRAPH_CHUNK="1"), dict(RB2_GRAPH_CHUNK="3"), dict(RB2_GRAPH_CHUNK="50"), dict(RB2_GRAPH_CHUNK="50", RB2_IRRED_SCRATCH="200000")],
                         ids=["1", "3", "50", "50-few-rows"])
def test_chunks(tiles, env):
    """the same rows whatever the chunking: one source per chunk, three, fifty (every source of this index has an edge, so every
    boundary lies inside a run of sources with edges), and fifty with stacks for a few rows only, so that a row takes several sources"""
    t = tiles("repeat")
    want = _equal(t.ix, 0, t.n, P, 1)
    assert len(set(want[:, 0].tolist())) >= t.n - 4
    with _Env(**env):
        edges, info = t.g.string_graph(pairs=True, **P)
        m, d_info, rows = graph_dev(t.g, 0, t.n, len(want) + 5, P, 1)
    assert np.array_equal(_sorted(edges), want) and info.tolist() == [len(want), len(want), 0, 0, 0, 0, 0, 0]
    assert (np.diff(edges[:, 0]) >= 0).all()
    assert m == len(want) and np.array_equal(_sorted(rows[:m]), want)


@pytest.fixture(scope="module")
def long_tile(hip):
    """4400 strings, nearly all with an edge: reads of 30 symbols every 1 .. 4 symbols of a genome of 5600, both strands (reads of one
    length lie inside no other, so nothing needs to be reduced)"""
    _, reads = U.tile_reads(seed=21, glen=5600, lo=30, hi=30, smax=4)
    g = hip.HipBwt(0)
    g.insert_multi(H.encode_batch(reads, True, True))
    ix = _Ix(g)
    yield ix
    g.close()


LONG_P = dict(P, min_ovlp=16, max_ext=30)


def test_scan_crosses_a_block_sum(long_tile):
    """more than 4096 sources with edges in one chunk: the offsets of the sources behind the first 4096 need the block sums"""
    ix = long_tile
    want = _equal(ix, 0, ix.n, LONG_P, 1)
    with_edges = np.unique(want[:, 0])
    assert ix.n > 4200 and len(with_edges) > 4150 and (with_edges > 4096).sum() > 50
    with _Env(RB2_GRAPH_CHUNK="4097"):                               # and a chunk boundary right behind the first block
        edges, info = ix.g.string_graph(pairs=True, **LONG_P)
    assert np.array_equal(_sorted(edges), want) and info[0] == len(want)


# ---- cap ----

def _cut_inside_a_source(want):
    """a cap that ends inside the rows of a source with two edges or more: (cap, that source)"""
    srcs, first, counts = np.unique(want[:, 0], return_index=True, return_counts=True)
    k = int(np.flatnonzero((counts >= 2) & (first > 10))[0])
    return int(first[k]) + 1, int(srcs[k])


@pytest.mark.parametrize("which", ["0", "1", "m-1", "m", "m+3", "inside"])
def test_cap(tiles, which):
    """the return value and info[0] stay m; the rows stored are the first min(m, cap) in increasing src, every source below the one
    that is cut complete; nothing is written from row cap on, nor in two guard rows behind it; cap 0 passes NULL"""
    t = tiles("repeat")
    g = t.g
    want = _equal(t.ix, 0, t.n, P, 1)
    m = len(want)
    cap, cut_src = _cut_inside_a_source(want)
    cap = {"0": 0, "1": 1, "m-1": m - 1, "m": m, "m+3": m + 3, "inside": cap}[which]
    h_m, h_rows, h_info = g.string_graph_raw(0, t.n, cap, pairs=True, fill=FILL, **P)
    d_m, d_info, d_rows = graph_dev(g, 0, t.n, cap, P, 1, null=cap == 0)
    for got_m, rows, info in ((h_m, h_rows, h_info), (d_m, d_rows, d_info)):
        k = min(m, cap)
        assert got_m == m and info.tolist() == [m, k, 0, 0, 0, 0, 0, 0]
        assert (rows[k:] == FILL).all(), "a row at or above cap was written"
        got = rows[:k]
        assert (np.diff(got[:, 0]) >= 0).all()
        if k == 0:
            continue
        last = int(got[-1, 0])                                       # the source that is cut (or the last one, complete)
        assert np.array_equal(_sorted(got[got[:, 0] < last]), want[want[:, 0] < last]), "a source below the cut is not complete"
        tail, full = _sorted(got[got[:, 0] == last]).tolist(), want[want[:, 0] == last].tolist()
        assert all(r in full for r in tail) and len(set(map(tuple, tail))) == len(tail) and len(got[got[:, 0] < last]) + len(full) >= k
        if which == "inside":
            assert last == cut_src and 0 < len(tail) < len(full)
        if k == m:
            assert np.array_equal(_sorted(got), want)


# ---- truncation, each case alone ----

def _counters(g, strings, p):
    """info[2:6] and m as the parent's irreducible_raw gives them for these sources"""
    qs = [s if len(s) <= IR.MAX_LEN else np.array([1, 0], np.uint8) for s in strings]      # (a string too long is malformed: any malformed query stands for it)
    _, rec, cnt = g.irreducible_raw(qs, p["min_ovlp"], p["max_ext"], p["max_steps"], p["max_recs"])
    found = np.where(cnt <= -2, -2 - cnt, np.maximum(cnt, 0))
    have = np.minimum(found, p["max_recs"])
    live = np.arange(p["max_recs"])[None, :] < have[:, None]
    width = (rec[:, :, 3] - rec[:, :, 2])[live]
    too_long = sum(len(s) > IR.MAX_LEN for s in strings)
    return [int((found > p["max_recs"]).sum()), int((width > p["max_hits"]).sum()), int((cnt <= -2).sum()), too_long], int(np.minimum(width, p["max_hits"]).sum())


def _truncated(ix, p, which, pairs=1):
    """the call under p against the counters of irreducible_raw and the rows of the untruncated run; counter `which` must be the
    only one that is not 0"""
    g = ix.g
    ctr, m_want = _counters(g, ix.strings, p)
    print("counters by irreducible_raw:", ctr, "edges", m_want)
    assert ctr[which] > 0 and sum(ctr) == ctr[which], ctr
    full, f_info = g.string_graph(pairs=pairs, **dict(p, **WIDE))
    assert f_info[2:5].tolist() == [0, 0, 0]
    full = set(map(tuple, full.tolist()))
    edges, info = g.string_graph(pairs=pairs, **p)
    assert info.tolist() == [m_want, m_want] + ctr + [0, 0] and len(edges) == m_want
    m, d_info, rows = graph_dev(g, 0, ix.n, m_want + 3, p, pairs)
    assert m == m_want and d_info.tolist() == info.tolist()
    for got in (edges, rows[:m]):
        got = list(map(tuple, got.tolist()))
        assert len(set(got)) == len(got) and set(got) <= full, "a stored row is no row of the untruncated run"
        assert (np.diff(np.array(got)[:, 0]) >= 0).all()
    return len(full), m_want


@pytest.fixture(scope="module")
def copies(hip):
    """tiled reads, some of them three times: the neighbours of a read come in ranges of three strings"""
    _, reads = U.tile_reads(seed=31, glen=260, lo=36, hi=36, smax=6)
    g = hip.HipBwt(0)
    g.insert_multi(H.encode_batch(reads + reads[5:15] + reads[5:15], True, True))
    ix = _Ix(g)
    yield ix
    g.close()


def test_max_hits_cuts_a_range(copies):
    n_full, m = _truncated(copies, dict(P, max_hits=1), 1)
    assert m < n_full


def test_max_recs_cuts_a_branching_read(tiles):
    n_full, m = _truncated(tiles("repeat").ix, dict(P, max_recs=1), 0)
    assert m < n_full


def test_max_steps_ends_a_source(tiles):
    n_full, m = _truncated(tiles("plain").ix, dict(P, max_steps=90), 2)
    assert m < n_full


def test_a_string_too_long(hip):
    """one read of 8200 symbols (two strings): no record, no edge, counted; everybody else as ever"""
    _, reads = U.tile_reads(seed=41, glen=200, lo=40, hi=40, smax=6)
    long_read = np.random.RandomState(42).randint(1, 5, size=8200).astype(np.uint8)
    g = hip.HipBwt(0)
    try:
        g.insert_multi(H.encode_batch(reads[:8] + [long_read] + reads[8:], True, True))
        ix = _Ix(g)
        assert len(ix.strings[16]) == 8200 and len(ix.strings[17]) == 8200
        n_full, m = _truncated(ix, P, 3)
        edges, _ = g.string_graph(pairs=True, **P)
        assert m == n_full and not {16, 17} & set(edges[:, 0].tolist())
        short = [s for k, s in enumerate(ix.strings) if k not in (16, 17)]
        assert len(edges) == len(U.brute_edges(short, P["min_ovlp"], P["max_ext"]))
    finally:
        g.close()


# ---- the index stays what it was ----

def test_index_untouched_and_takes_an_insert(hip):
    _, reads = U.tile_reads(seed=51, glen=400, lo=40, hi=50, smax=6)
    more = H.encode_batch(H.repetitive_reads(40, seed=52), True, True)
    g, o = hip.HipBwt(0), H.Oracle(0)
    try:
        b = H.encode_batch(reads, True, True)
        g.insert_multi(b)
        o.insert_multi(b)
        g.build_ssa(3)
        before = g.rope_hashes(), g.layout_stats(), g.ssa_info()
        edges, info = g.string_graph(pairs=True, **P)
        m, _, _ = graph_dev(g, 0, g._n_strings(), 7, P, 0)
        assert len(edges) > 100 and m == len(edges)
        assert (g.rope_hashes(), g.layout_stats(), g.ssa_info()) == before
        g.insert_multi(more)
        o.insert_multi(more)
        assert np.array_equal(g.bwt(), o.bwt())
        assert not g.ssa_info()["valid"]
    finally:
        g.close()
        o.close()


# ---- assemble ----

@pytest.mark.parametrize("name,circular", [("plain", False), ("repeat", False), ("plain", True)])
def test_assemble(tiles, name, circular):
    """graph, chains and texts on the device: what unitigs() returns and what the brute force over string slices gives, on a plain
    genome, one with a repeat, and a circular one"""
    t = tiles(name, circular)
    for canonical in (True, False):
        got, info = t.g.assemble(U.MIN_OVLP, canonical=canonical)
        assert info[0] == len(t.edges) and info[2:].tolist() == [0] * 6
        assert _as_lists(got) == t.brute[canonical], (name, circular, canonical)
        assert _as_lists(got) == _as_lists(t.g.unitigs(U.MIN_OVLP, canonical=canonical))
    if circular:
        assert all(c for _, _, c in _as_lists(got))
    got, _ = t.g.assemble(U.MIN_OVLP, min_reads=5, max_ext=64, max_recs=8)
    assert _as_lists(got) == [r for r in t.brute[True] if len(r[1]) >= 5]


def test_assemble_empty_index(hip):
    g = hip.HipBwt(0)
    try:
        g.build_ssa(2)
        got, info = g.assemble(5)
        assert got == [] and info.tolist() == [0] * 8
        edges, info = g.string_graph()
        assert edges.shape == (0, 4) and info.tolist() == [0] * 8
    finally:
        g.close()


# ---- fatal argument checks: each fires before any kernel runs ----

FATAL = [("no_ssa", "rb2_hip_ssa_build"), ("no_ssa_dev", "rb2_hip_ssa_build"), ("rank", "sharded index"), ("negative_first", "no range of the index"),
         ("negative_n", "no range of the index"), ("range_past_end", "no range of the index"), ("negative_cap", "cap must not be negative"),
         ("null_edges", "edges is NULL"), ("min_ovlp", "min_ovlp must be at least 1"), ("max_ext_low", "max_ext must be 1 .. 8192"),
         ("max_ext_high", "max_ext must be 1 .. 8192"), ("max_steps", "max_steps must be at least 1"), ("max_recs", "max_recs must be at least 1"),
         ("max_hits", "max_hits must be at least 1"), ("odd_pairs", "pairs needs"), ("dev_max_hits", "max_hits must be at least 1")]


@pytest.mark.parametrize("case,what", FATAL, ids=[c for c, _ in FATAL])
def test_fatal_parameters(hip, case, what):
    """each leaves through the fatal handler with the function's name and a message of its own, the index and the buffers untouched"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "graph_fatal_child.py"), case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out, err = p.stdout.decode(), p.stderr.decode()[-1500:]
    assert p.returncode == 7 and "the call returned" not in out, (p.returncode, out, err)
    assert "handler: [rb2_hip] string_graph" in out and what in out and "unchanged ok" in out, out
