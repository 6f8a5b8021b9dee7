"""GPU tests of the unitig calls (include/rb2_hip.h: rb2_hip_unitig_chains[_dev], rb2_hip_unitig_text[_dev]; kernels in csrc/rb2_unitig.h).
vtx, urec and txt are deterministic by definition, so everything is compared exactly with the model (tests/unitig_ref.py, which
tests/test_unitig_ref.py holds against brute force), and through HipBwt.unitigs with the brute force over string slices itself.  The
graphs are made up where the point is the graph -- the degrees that decide what a link is, and chains long enough for pointer jumping to
go wrong: longer than one launch wave of threads, more than 16 doublings, cycles whose length is and is not a power of two -- and come
from reads that tile a genome where the point is the text."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import unitig_ref as U
from test_query_layouts_gpu import _Models, _build_dense, _build_sparse

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILL = -7                                                            # what the device variants must leave where they store nothing
TFILL = 7                                                            # the same for text bytes (no nt6 code)
E = lambda rows: np.array(rows, np.int64).reshape(-1, 4)


def _to_dev(g, arrays):
    ptrs = [g.dev_alloc(max(a.nbytes, 8)) for a in arrays]
    for d, a in zip(ptrs, arrays):
        if a.nbytes:
            g.L.rb2_hip_memcpy(g.h, d, a.ctypes.data, a.nbytes, 0)
    return ptrs


def chains_dev(g, n, edges):
    """unitig_chains_dev on buffers filled with FILL, two rows of room behind vtx and four words behind info, which must stay as they were"""
    edges = np.ascontiguousarray(edges, np.int64).reshape(-1, 4)
    vtx = np.full((n + 2, 4), FILL, np.int64)
    info = np.full(8, FILL, np.int64)
    ptrs = _to_dev(g, (edges, vtx, info))
    try:
        g.unitig_chains_dev(n, len(edges), ptrs[0], ptrs[1], ptrs[2])
        g.sync()
        for d, a in zip(ptrs[1:], (vtx, info)):
            g.L.rb2_hip_memcpy(g.h, a.ctypes.data, d, a.nbytes, 1)
    finally:
        for d in ptrs:
            g.dev_free(d)
    assert (vtx[n:] == FILL).all() and (info[4:] == FILL).all(), "something was written behind vtx or info"
    return vtx[:n], info[:4]


def text_dev(g, vtx, canonical, min_reads, cap_u, cap_txt):
    """unitig_text_dev on buffers filled with FILL / TFILL with room behind them, which must stay as it was: (stored, urec, txt, info)"""
    vtx = np.ascontiguousarray(vtx, np.int64).reshape(-1, 4)
    urec = np.full((cap_u + 2, 5), FILL, np.int64)
    txt = np.full(cap_txt + 64, TFILL, np.uint8)
    ptrs = _to_dev(g, (vtx, urec, txt))
    try:
        stored, info = g.unitig_text_dev(len(vtx), ptrs[0], ptrs[1], ptrs[2], canonical, min_reads, cap_u, cap_txt)
        for d, a in zip(ptrs[1:], (urec, txt)):
            g.L.rb2_hip_memcpy(g.h, a.ctypes.data, d, a.nbytes, 1)
    finally:
        for d in ptrs:
            g.dev_free(d)
    assert (urec[cap_u:] == FILL).all() and (txt[cap_txt:] == TFILL).all(), "something was written behind urec or txt"
    return stored, urec[:cap_u], txt[:cap_txt], info


@pytest.fixture(scope="module")
def g0(hip):
    """an empty index: the chains read none"""
    g = hip.HipBwt(0)
    yield g
    g.close()


def _graph(g, n, edges):
    """host and device variant against the model; returns the model's (vtx, info)"""
    edges = E(edges)
    want, winfo = U.chains(n, edges)
    vtx, info = g.unitig_chains(edges, n)
    assert info.tolist() == winfo.tolist()
    assert np.array_equal(vtx, want), np.flatnonzero((vtx != want).any(axis=1))[:5].tolist()
    d_vtx, d_info = chains_dev(g, n, edges)
    assert d_info.tolist() == winfo.tolist() and np.array_equal(d_vtx, want)
    return want, winfo


SMALL = {
    "open path": (5, [[3, 1, 9, 2], [1, 4, 9, 3], [4, 0, 9, 1], [0, 2, 9, 7]], [1, 0, 5, 0]),
    "two paths merging": (5, [[0, 2, 9, 1], [1, 2, 9, 1], [2, 3, 9, 2], [3, 4, 9, 2]], [3, 0, 3, 0]),
    "fork": (5, [[0, 1, 9, 1], [1, 2, 9, 2], [2, 3, 9, 1], [2, 4, 9, 1]], [3, 0, 3, 0]),
    "cycle": (4, [[2, 3, 9, 1], [3, 1, 9, 2], [1, 0, 9, 3], [0, 2, 9, 4]], [1, 1, 4, 0]),
    "cycle with a tail": (6, [[5, 4, 9, 1], [4, 2, 9, 1], [2, 3, 9, 2], [3, 1, 9, 3], [1, 2, 9, 4]], [3, 0, 3, 0]),
    "self loop": (3, [[1, 1, 9, 6], [0, 2, 9, 1]], [2, 1, 2, 0]),
    "duplicated edge": (3, [[0, 1, 9, 1], [0, 1, 9, 1], [1, 2, 9, 1]], [2, 0, 2, 0]),
    "ignored edges": (3, [[-1, 0, 9, 1], [0, 3, 9, 1], [0, 1, 9, 0], [1, 2, 9, 1], [2, -5, 9, 1], [1 << 40, 0, 9, 1]], [2, 0, 2, 5]),
    "no edges": (4, [], [4, 0, 1, 0]),
    "no vertices": (0, [[0, 0, 9, 1], [1, 2, 9, 1]], [0, 0, 0, 2]),
    "nothing": (0, [], [0, 0, 0, 0]),
    "one vertex": (1, [[0, 0, 9, 3]], [1, 1, 1, 0]),
    "one vertex, no edges": (1, [], [1, 0, 1, 0]),
    "three vertices, one edge": (3, [[0, 1, 9, 1]], [2, 0, 2, 0]),   # odd counts: the 32-bit degree arrays end inside a word
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_graphs(g0, name):
    n, edges, info = SMALL[name]
    want, winfo = _graph(g0, n, edges)
    assert winfo.tolist() == info, name
    if name == "cycle with a tail":                                  # vertex 2 has two edges into it: the cycle opens there
        assert want[2].tolist() == [2, 0, 0, -1] and want[1].tolist() == [2, 2, 5, 3] and want[5].tolist() == [5, 0, 0, -1] and want[4].tolist() == [5, 1, 1, 1]
    if name == "self loop":
        assert want[1].tolist() == [1, 0, 0, 6]
    if name == "cycle":
        assert want[0].tolist() == [0, 0, 0, 3] and want[1].tolist() == [0, 3, 7, 2]


def _paths(rng, n, lens, cyclic=False):
    """edges of the paths (or cycles) of these lengths over a shuffled numbering of n = sum(lens) vertices, shuffled themselves"""
    perm = rng.permutation(n)
    rows, at = [], 0
    for ln in lens:
        ids = perm[at:at + ln]
        at += ln
        src, dst = (ids, np.roll(ids, -1)) if cyclic else (ids[:-1], ids[1:])
        rows.append(np.stack([src, dst, np.full(len(src), 9), rng.randint(1, 6, size=len(src))], 1))
    ed = np.concatenate(rows).astype(np.int64) if rows else np.zeros((0, 4), np.int64)
    return ed[rng.permutation(len(ed))]


def test_one_long_chain(g0):
    """70 001 vertices in one open chain, ids shuffled: more threads than one launch wave holds and 17 doublings.  A jump that wrote
    the buffer it reads would see, for some vertices, a pointer that had already moved"""
    n = 70001
    want, info = _graph(g0, n, _paths(np.random.RandomState(1), n, [n]))
    assert info.tolist() == [1, 0, n, 0] and sorted(want[:, 1].tolist()) == list(range(n))


@pytest.mark.parametrize("n,extra", [(4097, 0), (4096, 0), (65537, 0), (4097, 300)])
def test_long_cycles(g0, n, extra):
    """cycles of 2^12 + 1, 2^12 (after 12 doublings every pointer is back at its own vertex) and 2^16 + 1 vertices; the smallest id
    sits in the middle of the list the cycle was made from; with extra lone vertices around it"""
    rng = np.random.RandomState(n + extra)
    ids = rng.permutation(n + extra)[:n]
    k = int(np.argmin(ids))
    ids[[k, n // 2]] = ids[[n // 2, k]]
    edges = np.stack([ids, np.roll(ids, -1), np.full(n, 9), rng.randint(1, 6, size=n)], 1)[rng.permutation(n)]
    want, info = _graph(g0, n + extra, edges)
    assert info.tolist() == [1 + extra, 1, n, 0]
    h = int(ids.min())
    assert want[h].tolist()[:3] == [h, 0, 0] and want[h, 3] >= 1 and (want[ids, 0] == h).all() and sorted(want[ids, 1].tolist()) == list(range(n))


def test_many_chains(g0):
    """10 000 chains of 1 .. 40 vertices and 50 cycles among them, everything shuffled"""
    rng = np.random.RandomState(4)
    lens = rng.randint(1, 41, size=10000)
    n1 = int(lens.sum())
    clens = rng.randint(2, 41, size=50)
    n = n1 + int(clens.sum())
    ed = np.concatenate([_paths(rng, n1, lens), _paths(rng, int(clens.sum()), clens, True) + np.array([n1, n1, 0, 0])])
    relabel = rng.permutation(n)
    ed[:, 0], ed[:, 1] = relabel[ed[:, 0]], relabel[ed[:, 1]]
    want, info = _graph(g0, n, ed)
    assert info.tolist() == [10050, 50, 40, 0]


# ---- texts ----

class _Tile:
    """the reduced index of both strands of a tile input with its suffix array, the strings by id, and the graph"""
    def __init__(self, hip, name, circular=False):
        _, reads, self.strings = U.tile_case(name, circular)
        self.g = g = hip.HipBwt(0)
        g.insert_multi(H.encode_batch(reads, True, True))
        gone = g.reduce(pairs=True)
        self.n = n = len(self.strings)
        assert 2 * len(reads) - len(gone) == n
        assert [s.tobytes() for s in g.extract(np.arange(n), 64)] == [s.tobytes() for s in self.strings]
        g.build_ssa(2)
        self.edges = g.edges(min_ovlp=U.MIN_OVLP, pairs=True)
        self.vtx, self.info = U.chains(n, self.edges)
        self.brute = {c: U.brute_unitigs(self.strings, U.MIN_OVLP, U.MAX_EXT, canonical=c) for c in (True, False)}


@pytest.fixture(scope="module")
def tiles(hip):
    made = {}

    def get(name, circular=False):
        if (name, circular) not in made:
            made[name, circular] = _Tile(hip, name, circular)
        return made[name, circular]
    yield get
    for t in made.values():
        t.g.close()


def _as_lists(us):
    return [(np.asarray(t, np.uint8).tobytes(), [int(v) for v in p], bool(c)) for t, p, c in us]


@pytest.mark.parametrize("name", sorted(U.TILES))
def test_tiles_against_brute_force(tiles, name):
    """reduce(pairs=True), edges(pairs=True), unitigs(): the edges and the unitigs of the brute force, and the counts the issue pins"""
    t = tiles(name)
    _, n_strings, n_edges, n_chains, canon = U.TILES[name]
    assert t.n == n_strings and t.edges.tolist() == [list(r) for r in U.brute_edges(t.strings, U.MIN_OVLP, U.MAX_EXT)] and len(t.edges) == n_edges
    vtx, info = t.g.unitig_chains(t.edges)
    assert np.array_equal(vtx, t.vtx) and info.tolist() == t.info.tolist() and info[0] == n_chains and info[1] == 0
    for canonical in (True, False):
        got = _as_lists(t.g.unitigs(U.MIN_OVLP, canonical=canonical))
        assert got == t.brute[canonical], (name, canonical)
    assert [(len(p), len(x)) for x, p, _ in _as_lists(t.g.unitigs(U.MIN_OVLP))] == canon
    assert _as_lists(t.g.unitigs(U.MIN_OVLP, min_reads=5)) == [r for r in t.brute[True] if len(r[1]) >= 5]


@pytest.mark.parametrize("canonical", [0, 1])
@pytest.mark.parametrize("min_reads", [1, 2, 5])
def test_selection_and_caps(tiles, canonical, min_reads):
    """urec and txt against the model; caps 0 size the buffers and touch nothing; one byte short of the last chain leaves it out, record
    and slice as they were; host and device variant alike"""
    t = tiles("repeat")
    g = t.g
    w_urec, w_txt, w_inf = U.texts(t.strings, t.vtx, canonical, min_reads)
    k, total = len(w_urec), len(w_txt)
    assert k >= 2 and (canonical or min_reads > 1 or k == 10)
    for call in (lambda cu, ct: g.unitig_text_raw(t.vtx, canonical, min_reads, cu, ct, fill=TFILL), lambda cu, ct: text_dev(g, t.vtx, canonical, min_reads, cu, ct)):
        stored, urec, txt, info = call(0, 0)
        assert stored == 0 and info.tolist() == [k, total, 0, 0]
        stored, urec, txt, info = call(k, 0)                         # (either cap 0: sizes only)
        assert stored == 0 and info.tolist() == [k, total, 0, 0] and (urec == urec[0, 0]).all() and urec[0, 0] in (FILL, TFILL)
        stored, urec, txt, info = call(k, total)
        assert stored == k and info.tolist() == [k, total, 0, k] and np.array_equal(urec, w_urec) and np.array_equal(txt, w_txt)
        stored, urec, txt, info = call(k + 3, total - 1)
        assert stored == k - 1 and info.tolist() == [k, total, 0, k - 1]
        last = int(w_urec[-1, 2])
        assert np.array_equal(urec[:k - 1], w_urec[:-1]) and np.array_equal(txt[:last], w_txt[:last])
        assert (urec[k - 1:] == urec[-1, 0]).all() and (txt[last:] == TFILL).all(), "the chain that does not fit was written"
        stored, urec, txt, info = call(k - 1, total)                 # one record short
        assert stored == k - 1 and info.tolist() == [k, total, 0, k - 1] and np.array_equal(urec, w_urec[:-1]) and (txt[last:] == TFILL).all()
    urec, txt = g.unitig_text(t.vtx, canonical, min_reads)
    assert np.array_equal(urec, w_urec) and np.array_equal(txt, w_txt)


def test_circular_genome(tiles):
    """reads that run on round the end of the genome: one circular chain per strand, cut at its smallest id"""
    t = tiles("plain", True)
    vtx, info = t.g.unitig_chains(t.edges)
    assert np.array_equal(vtx, t.vtx) and info.tolist() == [2, 2, t.n // 2, 0]
    for canonical in (True, False):
        got = _as_lists(t.g.unitigs(U.MIN_OVLP, canonical=canonical))
        assert got == t.brute[canonical] and all(c for _, _, c in got)
    urec, txt = t.g.unitig_text(vtx)
    assert (urec[:, 4] == 1).all() and urec[:, 0].tolist() == [0, 1]


def test_short_piece(tiles):
    """an ext larger than its read (an edge list that does not belong to this index): zeros in front of the piece, flag bit 1, the
    chain counted, and the other chain's slice as it always was"""
    t = tiles("plain")
    edges = t.edges.copy()
    k = int(np.flatnonzero(edges[:, 0] % 2 == 0)[5])                # a link of the even strand's chain
    edges[k, 3] = 100
    vtx, info = t.g.unitig_chains(edges)
    want, _ = U.chains(t.n, edges)
    assert np.array_equal(vtx, want)
    w_urec, w_txt, w_inf = U.texts(t.strings, want)
    assert w_urec[:, 4].tolist() == [2, 0] and w_inf.tolist() == [2, len(w_txt), 1]
    stored, urec, txt, info = t.g.unitig_text_raw(vtx, cap_u=2, cap_txt=len(w_txt), fill=TFILL)
    assert stored == 2 and info.tolist() == [2, len(w_txt), 1, 2] and np.array_equal(urec, w_urec) and np.array_equal(txt, w_txt)
    plain = U.texts(t.strings, t.vtx)[1]
    assert (txt == 0).sum() == 100 - len(t.strings[edges[k, 1]]) and txt[urec[1, 2]:].tobytes() == plain[len(plain) // 2:].tobytes()
    d = text_dev(t.g, vtx, False, 1, 2, len(w_txt))
    assert d[0] == 2 and np.array_equal(d[1], w_urec) and np.array_equal(d[2], w_txt) and d[3].tolist() == info.tolist()


@pytest.mark.parametrize("bad", [-1, "n", 1 << 50])
def test_damaged_rows(tiles, bad):
    """a row whose head is no vertex: its vertex is a chain of its own with the short-piece flag, and the call stays in bounds; a row
    whose off is no offset adds no piece"""
    t = tiles("repeat")
    vtx = t.vtx.copy()
    v = int(np.flatnonzero(vtx[:, 1] == 2)[0])                       # the third vertex of some chain
    w = int(np.flatnonzero((vtx[:, 1] == 1) & (vtx[:, 0] != vtx[v, 0]))[-1])   # the second of another
    vtx[v, 0] = t.n if bad == "n" else bad
    vtx[w, 2] = -3
    k = len(U.texts(t.strings, vtx)[0])
    assert k == 11
    for fill, call in ((0, lambda cu, ct: t.g.unitig_text_raw(vtx, cap_u=cu, cap_txt=ct, fill=TFILL)), (TFILL, lambda cu, ct: text_dev(t.g, vtx, False, 1, cu, ct))):
        # what no piece covers any more -- the places of the two pieces -- is 0 from the host variant and left alone by the device variant
        w_urec, w_txt, w_inf = U.texts(t.strings, vtx, fill=fill)
        assert w_inf[2] == 2 and (w_urec[:, 0] == v).sum() == 1 and (w_txt == fill).sum() >= 2
        stored, urec, txt, info = call(k, len(w_txt))
        assert stored == k and info.tolist() == [k, len(w_txt), 2, k]
        assert np.array_equal(urec, w_urec) and np.array_equal(txt, w_txt)


@pytest.fixture(scope="module")
def models():
    ms = _Models()
    yield ms
    ms.made.clear()


@pytest.mark.parametrize("kind", ["D", "S"])
def test_layouts(hip, models, kind):
    """made-up chains over the strings of layout D (dense, every piece longer than two superblocks) and layout S (sparse, split leaves)
    of test_query_layouts_gpu.py: the walks of the heads and of the pieces cross pieces, superblocks and split leaves"""
    ix = _build_dense(hip, models.get(0)) if kind == "D" else _build_sparse(hip, models.get("S"))
    g = ix.g
    try:
        n = int(g.counts()[:, 0].sum())
        strings = [np.asarray(s, np.uint8) for s in g.extract(np.arange(n), 2048)]
        rng = np.random.RandomState(n)
        lens = []
        while sum(lens) < n:
            lens.append(min(int(rng.randint(1, 30)), n - sum(lens)))
        edges = _paths(rng, n, lens)
        edges[:, 3] = [rng.randint(1, min(len(strings[d]), 80) + 1) if len(strings[d]) else 1 for d in edges[:, 1].tolist()]
        before = g.layout_stats()
        vtx, info = g.unitig_chains(edges)
        want, winfo = U.chains(n, edges)
        assert np.array_equal(vtx, want) and info.tolist() == winfo.tolist() and info[0] == len(lens)
        for canonical, min_reads in ((0, 1), (1, 3)):
            w_urec, w_txt, w_inf = U.texts(strings, vtx, canonical, min_reads)
            urec, txt = g.unitig_text(vtx, canonical, min_reads)
            assert np.array_equal(urec, w_urec) and np.array_equal(txt, w_txt), (kind, canonical, min_reads)
            assert len(urec) > 20 and w_inf[2] == (0 if all(len(s) for s in strings) else w_inf[2])
        assert g.layout_stats() == before, "the query changed the layout"
    finally:
        g.close()


def _child(stage):
    p = subprocess.run([sys.executable, os.path.join(HERE, "unitig_child.py"), stage], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p.returncode, p.stdout.decode(), p.stderr.decode()[-1500:]


def test_chunked_edges(hip):
    """RB2_QUERY_CHUNK=7 in a process of its own: the same chains and texts"""
    rc, out, err = _child("chunk")
    assert rc == 0 and "STAGE OK" in out, (rc, out, err)


@pytest.mark.parametrize("stage,what", [("reads0", "min_reads"), ("nstr", "n_str"), ("nstr-dev", "n_str"), ("capu", "cap_u"), ("capt", "cap_txt"),
                                        ("chains-n", "n_str"), ("chains-m", "n_str and m"), ("chains-dev-n", "n_str"), ("shard", "sharded index")])
def test_fatal_parameters(hip, stage, what):
    """each leaves through the fatal handler with the function's name and the parameter in the message"""
    rc, out, err = _child(stage)
    assert rc == 7 and "NOT FATAL" not in out, (rc, out, err)
    assert "unitig ok" in out and "handler: [rb2_hip] unitig_" in out and what in out, out
