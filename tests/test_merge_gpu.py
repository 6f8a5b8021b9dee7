"""GPU tests of rb2_hip_unpack[_dev] and rb2_hip_merge (include/rb2_hip.h; kernels k_unpack_len / k_unpack_text in csrc/rb2_unpack.h).

Unpack: the expected (txt, off) is the model (tests/merge_ref.py: query_ref.FM.walk_all on the oracle's BWT of the same strings), in
both directions, on the dense and the forced sparse layout, on loaded indexes and on pieces longer than two superblocks.
Merge: the expected index is the oracle's BWT of dst's strings followed by src's AND the device's own one-handle build of the same,
compared run byte for run byte and as .fmd images, whatever the batch budget.

One thing the issue asked for cannot be built: a loaded index whose walk from a string id never meets a `$`.  load_ropes takes any six
streams with consistent totals, and on such streams LF is one-to-one and maps no row into the `$` block, so every walk that starts
there ends (test_contain_ref.py proves it for the model; test_contain_gpu.py::test_index_that_is_no_bwt_of_strings met the same).  The
fatal walk guard stays a guard; test_loaded_streams_that_are_no_bwt checks what can be checked: the call returns what the model
gives for those streams and writes nothing outside txt and off."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import contain_ref as CR
import fmd_ref
import helpers as H
import merge_ref as M
import query_ref as Q
from ropebwt2_amd.hipbwt import encode_runs
from test_query_gpu import _Env

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FORCED = dict(RB2_SPARSE_LAMBDA="1e18", RB2_SPARSE_MAXPEN="0")       # every batch in place: the sparse layout (test_leaf_split_gpu.py)
DENSE = dict(RB2_SPARSE_LAMBDA="0")                                  # never leave the dense layout
CANARY = 0xAB


# ---- the string sets and their models, each computed once ---------------------------------------------------------------------------

def _long_reads(seed, n=12):
    """reads of 1500 .. 2600 symbols with runs of N: batches long enough for the index to stay in the sparse layout when it is forced"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        r = rng.randint(1, 5, size=int(rng.randint(1500, 2600))).astype(np.uint8)
        for _ in range(int(rng.randint(0, 3))):
            at = int(rng.randint(0, len(r) - 1))
            r[at:at + int(rng.randint(1, 300))] = 5
        out.append(r)
    return out


def _every_length(seed):
    """two strings of every length 0 .. 40, shuffled: every length mod 16, and (asserted where it is used) every offset mod 16"""
    rng = np.random.RandomState(seed)
    out = [rng.randint(1, 5, size=L).astype(np.uint8) for L in range(41) for _ in range(2)]
    return [out[i] for i in rng.permutation(len(out))]


@functools.lru_cache(maxsize=None)
def _set(name):
    """the batches (lists of strings) of a named string set"""
    if name == "U":                                                 # unpack: 82 + 204 short strings, then 12 long ones
        return (_every_length(1) + M.mixed_reads(100, 31), M.mixed_reads(100, 32), _long_reads(5))
    if name == "A":                                                 # merge destination
        return (M.mixed_reads(150, 41), _long_reads(6, 8))
    if name == "B":                                                 # merge source: strings of A again, empty strings, N
        return (M.mixed_reads(120, 42) + list(_set("A")[0][:40]), _long_reads(7, 8))
    if name == "small":
        return (M.mixed_reads(40, 43),)
    if name == "big":
        return (M.mixed_reads(400, 44),)
    if name == "C":
        return (M.mixed_reads(60, 45),)
    raise KeyError(name)


def _bufs(name):
    return [H.encode_batch(p) for p in _set(name)]


@functools.lru_cache(maxsize=None)
def _model(so, *names):
    """(the oracle's BWT of the sets' batches in this order, the (txt, off) of its strings in text order and reversed)"""
    bwt = M.oracle_bwt(so, [b for nm in names for b in _bufs(nm)])
    return bwt, M.unpack(bwt), M.unpack(bwt, reversed=True)


def _build(hip, so, names, sparse=False):
    with _Env(**(FORCED if sparse else DENSE)):
        g = hip.HipBwt(so)
    for nm in names:
        for b in _bufs(nm):
            g.insert_multi(b)
    assert g.layout_stats()["sparse_now"] == sparse
    return g


def _mirror(txt, rtxt, off):
    for i in range(len(off) - 1):
        assert txt[off[i + 1] - 1] == 0 and rtxt[off[i + 1] - 1] == 0
        assert np.array_equal(txt[off[i]:off[i + 1] - 1][::-1], rtxt[off[i]:off[i + 1] - 1]), i


def _check_unpack(g, want, wrev, ranges=()):
    """the whole index in both directions, and sub-ranges (first, n), against the model's (txt, off)"""
    txt, off = g.unpack_raw()
    rtxt, roff = g.unpack_raw(reversed=True)
    assert np.array_equal(off, want[1]) and np.array_equal(roff, want[1])
    assert np.array_equal(txt, want[0]) and np.array_equal(rtxt, wrev[0])
    _mirror(txt, rtxt, off)
    for first, n in ranges:
        for rev, w in ((False, want), (True, wrev)):
            t, o = g.unpack_raw(first, n, rev)
            assert np.array_equal(o, w[1][first:first + n + 1] - w[1][first]), (first, n, rev)
            assert np.array_equal(t, w[0][w[1][first]:w[1][first + n]]), (first, n, rev)


def _to_dev(g, a):
    d = g.dev_alloc(max(a.nbytes, 8))
    if a.nbytes:
        g.L.rb2_hip_memcpy(g.h, d, a.ctypes.data, a.nbytes, 0)
    return d


def _unpack_dev(g, first, n, rev, cap, room=64):
    """unpack_dev into canary-filled buffers with room behind them: (SIZE, txt with its room, off with two words of room)"""
    txt = np.full(max(cap, 0) + room, CANARY, np.uint8)
    off = np.full(n + 3, -7, np.int64)
    dt, do = _to_dev(g, txt), _to_dev(g, off)
    try:
        size = g.unpack_dev(first, n, rev, cap, dt, do)
        g.sync()
        g.L.rb2_hip_memcpy(g.h, txt.ctypes.data, dt, txt.nbytes, 1)
        g.L.rb2_hip_memcpy(g.h, off.ctypes.data, do, off.nbytes, 1)
    finally:
        g.dev_free(dt); g.dev_free(do)
    assert (off[n + 1:] == -7).all(), "something was written behind off"
    return size, txt, off[:n + 1]


# ---- unpack ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("so", [0, 1, 2])
def test_unpack_orders_and_layouts(hip, so, sparse):
    bwt, want, wrev = _model(so, "U")
    n = len(want[1]) - 1
    lens = np.diff(want[1]) - 1
    assert n == 342 and set(lens[lens <= 40] % 16) == set(range(16)) and set(want[1][:-1] % 16) == set(range(16)) and lens.max() > 1500
    g = _build(hip, so, ["U"], sparse)
    g.build_ssa(4)
    before = g.layout_stats(), g.ssa_info()
    ranges = [(0, k) for k in (1, 15, 16, 17, 257)] + [(n - k, k) for k in (1, 15, 16, 17, 257)] + [(41, 0), (n, 0), (100, 33)]
    _check_unpack(g, want, wrev, ranges)
    assert [s.tobytes() for s in g.unpack(3, 20)] == [want[0][want[1][i]:want[1][i + 1] - 1].tobytes() for i in range(3, 23)]
    for rev, w in ((False, want), (True, wrev)):                    # the device variant, the same slices
        size, txt, off = _unpack_dev(g, 7, 257, rev, int(w[1][264] - w[1][7]))
        assert size == w[1][264] - w[1][7] and np.array_equal(off, w[1][7:265] - w[1][7])
        assert np.array_equal(txt[:size], w[0][w[1][7]:w[1][264]]) and (txt[size:] == CANARY).all()
    assert (g.layout_stats(), g.ssa_info()) == before and before[1]["valid"], "unpack changed the layout or the suffix array"
    assert np.array_equal(g.bwt(), bwt)                             # (leaves the sparse layout: last)
    g.close()


def test_unpack_one_long_string_among_short_ones(hip):
    rng = np.random.RandomState(8)
    reads = M.mixed_reads(30, 51) + [rng.randint(1, 5, size=20011).astype(np.uint8)] + M.mixed_reads(30, 52)
    buf = H.encode_batch(reads)
    for so in (0, 1):
        bwt = M.oracle_bwt(so, [buf])
        g = hip.HipBwt(so)
        g.insert_multi(buf)
        _check_unpack(g, M.unpack(bwt), M.unpack(bwt, reversed=True), [(25, 17)])
        g.close()


def test_unpack_cap_chunks_and_state(hip):
    so = 0
    bwt, want, wrev = _model(so, "U")
    n, size = len(want[1]) - 1, len(want[0])
    g = _build(hip, so, ["U"])
    hashes = g.rope_hashes()
    for rev, w in ((False, want), (True, wrev)):
        # host variant: cap == SIZE - 1 writes off and not one byte of txt; cap == SIZE fills exactly SIZE bytes
        txt, off = np.full(size + 64, CANARY, np.uint8), np.full(n + 3, -7, np.int64)
        call = lambda cap: g.L.rb2_hip_unpack(g.h, 0, n, int(rev), cap, txt.ctypes.data, off.ctypes.data)
        assert call(size - 1) == size and (txt == CANARY).all() and np.array_equal(off[:n + 1], w[1]) and (off[n + 1:] == -7).all()
        assert call(0) == size and (txt == CANARY).all()
        assert call(size) == size and np.array_equal(txt[:size], w[0]) and (txt[size:] == CANARY).all() and (off[n + 1:] == -7).all()
        assert g.L.rb2_hip_unpack(g.h, 0, n, int(rev), size, None, None) == size                    # sizes only
        # device variant: the same
        got, txt, off = _unpack_dev(g, 0, n, rev, size - 1)
        assert got == size and (txt == CANARY).all() and np.array_equal(off, w[1])
        got, txt, off = _unpack_dev(g, 0, n, rev, size)
        assert got == size and np.array_equal(txt[:size], w[0]) and (txt[size:] == CANARY).all() and np.array_equal(off, w[1])
        with _Env(RB2_QUERY_CHUNK=7):                                # the chunked staging and the chunked launches: the same bytes
            t7, o7 = g.unpack_raw(reversed=rev)
            assert np.array_equal(t7, w[0]) and np.array_equal(o7, w[1])
            t7, o7 = g.unpack_raw(5, 100, rev)
            assert np.array_equal(t7, w[0][w[1][5]:w[1][105]]) and np.array_equal(o7, w[1][5:106] - w[1][5])
            got, txt, off = _unpack_dev(g, 0, n, rev, size)
            assert got == size and np.array_equal(txt[:size], w[0]) and (txt[size:] == CANARY).all() and np.array_equal(off, w[1])
    assert g.rope_hashes() == hashes
    g.close()


@pytest.mark.parametrize("so", [0, 1, 2])
def test_unpack_dev_feeds_insert_multi_dev(hip, so):
    """the reversed text is a batch: straight from unpack_dev into insert_multi_dev of a fresh handle, it reproduces the index"""
    bwt, want, wrev = _model(so, "A")
    g = _build(hip, so, ["A"])
    n, size = len(want[1]) - 1, len(want[0])
    dt = g.dev_alloc(size + 64)
    f = hip.HipBwt(so)
    try:
        assert g.unpack_dev(0, n, True, size, dt, None) == size
        g.sync()
        f.insert_multi_dev(dt, size)
        f.sync()
    finally:
        g.dev_free(dt)
    assert f.rope_hashes() == g.rope_hashes() and np.array_equal(f.bwt(), bwt)
    g.close(); f.close()


def test_unpack_tiny_indexes(hip):
    for so in (0, 2):
        for reads in ([np.array([1, 2, 3, 4, 4, 5, 1], np.uint8)], [np.zeros(0, np.uint8)], [np.zeros(0, np.uint8)] * 37):
            buf = H.encode_batch(reads)
            bwt = M.oracle_bwt(so, [buf])
            g = hip.HipBwt(so)
            g.insert_multi(buf)
            _check_unpack(g, M.unpack(bwt), M.unpack(bwt, reversed=True), [(0, 1), (len(reads) - 1, 1)])
            g.close()
    g = hip.HipBwt(0)                                               # an empty index: no strings, SIZE 0
    txt, off = g.unpack_raw()
    assert len(txt) == 0 and off.tolist() == [0] and g.unpack() == []
    g.close()


@pytest.mark.parametrize("name", fmd_ref.FIXTURES)
def test_unpack_loaded_fmd(hip, name):
    img, bwt = fmd_ref.fixture(name)
    g = hip.HipBwt(0)
    assert g.load_fmd(np.frombuffer(img, np.uint8)) == len(bwt)
    want, wrev = M.unpack(bwt), M.unpack(bwt, reversed=True)
    n = len(want[1]) - 1
    _check_unpack(g, want, wrev, [(n // 3, min(17, n - n // 3))])
    g.close()


def test_unpack_pieces_longer_than_two_superblocks(hip):
    """both strands of 9000 reads of 100 symbols: every piece (b,x), b, x in A..T, spans more than two superblocks (test_query_layouts_gpu.py: D)"""
    codes = H.splitmix_bases(9000, 100, seed=77)
    bufs = [H.encode_batch_fixed(codes[:4500], True, True), H.encode_batch_fixed(codes[4500:], True, True)]
    bwt = M.oracle_bwt(0, bufs)
    g = hip.HipBwt(0)
    for b in bufs:
        g.insert_multi(b)
    for rev in (False, True):
        txt, off = g.unpack_raw(reversed=rev)
        assert np.array_equal(off, np.arange(18001, dtype=np.int64) * 101)
        assert np.array_equal(txt, np.concatenate(bufs) if rev else M.unpack(bwt)[0])               # (input order: the reversed text is the batches themselves)
    g.close()


def test_loaded_streams_that_are_no_bwt(hip):
    """six streams with consistent totals that are the BWT of no strings: every walk from the `$` block still ends (see the module's
    docstring), so the call is not fatal; it returns what the model gives for these streams"""
    bwt, _, _ = _model(0, "small")
    shorter = 0
    for seed in (0, 1):
        bad = CR.shuffled_ropes(bwt, seed)
        fm = Q.FM(bad)
        cut = np.concatenate([fm.C, [fm.N]])
        g = hip.HipBwt(0)
        g.load_ropes([encode_runs(bad[cut[a]:cut[a + 1]]) for a in range(6)])
        want, wrev = M.unpack(bad), M.unpack(bad, reversed=True)
        total = int(want[1][-1])
        assert len(want[1]) - 1 == fm.C[1] and total <= len(bad)     # (every walk ends; rows on cycles of LF behind the `$` block lie on none)
        shorter += total < len(bad)
        _check_unpack(g, want, wrev)
        size, txt, off = _unpack_dev(g, 0, len(want[1]) - 1, True, total)
        assert size == total and np.array_equal(txt[:size], wrev[0]) and (txt[size:] == CANARY).all() and np.array_equal(off, want[1])
        g.close()
    assert shorter > 0                                              # (the streams are not those of the strings they were shuffled from)


FATAL = [("range_past_end", "unpack: strings 30 .. 30 + 11 are no range of the index (it holds 40)"), ("negative_first", "are no range of the index"),
         ("negative_n", "are no range of the index"), ("negative_cap", "unpack: cap must not be negative (got -1)"),
         ("rank_unpack", "unpack: this handle holds only its own sub-ropes of a sharded index"),
         ("dst_is_src", "merge: dst and src must be two different handles"), ("negative_batch", "merge: batch_bytes must not be negative (got -1)"),
         ("rank_dst", "merge: dst holds only its own sub-ropes of a sharded index"), ("rank_src", "merge: src holds only its own sub-ropes of a sharded index")]


@pytest.mark.parametrize("case,msg", FATAL, ids=[c for c, _ in FATAL])
def test_fatal_conditions(hip, case, msg):
    p = subprocess.run([sys.executable, os.path.join(HERE, "merge_fatal_child.py"), case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    out, err = p.stdout.decode(), p.stderr.decode()[-2000:]
    assert p.returncode == 7, (p.returncode, out, err)
    assert "handler: [rb2_hip] " in out and msg in out and "unchanged ok" in out, out


# ---- merge ----------------------------------------------------------------------------------------------------------------------------

def _greedy(strs, budget):
    """batches of whole strings of at most budget bytes (each string and its 0), a longer string alone"""
    n, cur = 0, 0
    for s in strs:
        if cur and cur + len(s) + 1 > budget:
            n, cur = n + 1, 0
        cur += len(s) + 1
    return n + (cur > 0)


def _image(g):
    return [g.rope_rle(b).tobytes() for b in range(6)], g.save_fmd().tobytes()


def _n_strings(*names):
    return sum(len(p) for nm in names for p in _set(nm))


def _n_symbols(*names):
    return sum(len(s) for nm in names for p in _set(nm) for s in p)


@pytest.mark.parametrize("src_sparse", [False, True], ids=["src_dense", "src_sparse"])
@pytest.mark.parametrize("dst_sparse", [False, True], ids=["dst_dense", "dst_sparse"])
@pytest.mark.parametrize("so", [0, 1, 2])
def test_merge_orders_and_layouts(hip, so, dst_sparse, src_sparse):
    bwt, want, _ = _model(so, "A", "B")
    bwt_b = _model(so, "B")[0]
    dst, src = _build(hip, so, ["A"], dst_sparse), _build(hip, so, ["B"], src_sparse)
    one = _build(hip, so, ["A", "B"])                               # the device's own build of the same strings in one handle
    src.build_ssa(3); dst.build_ssa(3)
    src_before = src.layout_stats(), src.ssa_info(), (None if src_sparse else src.rope_hashes())
    nb, sb = _n_strings("B"), _n_symbols("B")
    info = dst.merge(src)
    assert info[:3] == (nb, sb, 1) and info[3] == nb + sb, info
    assert (src.layout_stats(), src.ssa_info()) == src_before[:2] and src.ssa_info()["valid"], "the merge changed src"
    assert not dst.ssa_info()["valid"], "dst kept a suffix array of other rows"
    # dst answers for strings of both origins
    pats = [s for s in list(_set("A")[0][:15]) + list(_set("B")[0][:15]) if len(s)]
    fm = Q.FM(bwt)
    assert dst.count(pats).tolist() == [fm.count(p) for p in pats] and min(dst.count(pats)) >= 1
    n = len(want[1]) - 1
    rows = [0, 1, n // 2, n - 2, n - 1]
    assert [s.tobytes() for s in dst.extract(rows, 3000)] == [want[0][want[1][r]:want[1][r + 1] - 1].tobytes() for r in rows]
    assert np.array_equal(dst.bwt(), bwt)
    assert _image(dst) == _image(one) and dst.rope_hashes() == one.rope_hashes()
    assert np.array_equal(src.bwt(), bwt_b)
    if not src_sparse:
        assert src.rope_hashes() == src_before[2]
    for g in (dst, src, one):
        g.close()


@pytest.mark.parametrize("so", [0, 1, 2])
def test_merge_batch_budgets(hip, so):
    """RB2_MERGE_BATCH at 1 (every string a batch of its own), at a value that cuts a few batches, unset, and batch_bytes itself:
    the same index, other batch counts"""
    bwt = _model(so, "big", "small")[0]
    one = _build(hip, so, ["big", "small"])
    want = _image(one)
    src = _build(hip, so, ["small"])
    n, syms = _n_strings("small"), _n_symbols("small")
    counts = []
    for env, arg in (({"RB2_MERGE_BATCH": 1}, 0), ({"RB2_MERGE_BATCH": (n + syms) // 4 + 1}, 0), ({}, 0), ({"RB2_MERGE_BATCH": 1}, (n + syms) // 2 + 1)):
        dst = _build(hip, so, ["big"])
        with _Env(**env):
            info = dst.merge(src, arg)
        assert info[:2] == (n, syms) and 1 <= info[3] <= max(arg or int(env.get("RB2_MERGE_BATCH", n + syms)), 41), info
        counts.append(info[2])
        assert _image(dst) == want and np.array_equal(dst.bwt(), bwt), (so, env, arg)
        dst.close()
    assert counts[0] == n and 3 <= counts[1] <= 5 and counts[2] == 1 and 2 <= counts[3] <= 3, counts
    src.close(); one.close()


def test_merge_special_shapes(hip):
    so = 1
    empty = hip.HipBwt(so)
    # an empty src: 0, dst as it was, its suffix array still valid
    dst = _build(hip, so, ["small"])
    dst.build_ssa(2)
    hashes, ssa = dst.rope_hashes(), dst.ssa_info()
    assert dst.merge(empty) == (0, 0, 0, 0) and dst.L.rb2_hip_merge(dst.h, empty.h, 0, None) == 0
    assert dst.rope_hashes() == hashes and dst.ssa_info() == ssa and ssa["valid"]
    # an empty dst: src's strings, rebuilt in dst's sorting order (src was built in another)
    src0 = _build(hip, 0, ["small"])
    with _Env(RB2_MERGE_BATCH=300):
        info = empty.merge(src0)
    assert info[0] == _n_strings("small") and info[2] > 2 and np.array_equal(empty.bwt(), _model(so, "small")[0])
    assert np.array_equal(src0.bwt(), _model(0, "small")[0])
    src0.close(); empty.close()
    # src larger than dst (dst larger than src: test_merge_batch_budgets)
    big = _build(hip, so, ["big"])
    ret = dst.L.rb2_hip_merge(dst.h, big.h, 0, None)
    assert ret == _n_strings("big") + _n_symbols("big")
    assert np.array_equal(dst.bwt(), _model(so, "small", "big")[0])
    # three indexes chained: (small + big) + C
    c = _build(hip, so, ["C"])
    with _Env(RB2_MERGE_BATCH=500):
        dst.merge(c)
    one = _build(hip, so, ["small", "big", "C"])
    assert np.array_equal(dst.bwt(), _model(so, "small", "big", "C")[0]) and _image(dst) == _image(one)
    for g in (dst, big, c, one):
        g.close()


def test_merge_golden_fmd(hip, tmp_path):
    """rand300.fmd and kat6.fmd in two handles, merged; then the same through tools/fmd_merge.py on two written files"""
    (img_a, bwt_a), (img_b, bwt_b) = fmd_ref.fixture("rand300"), fmd_ref.fixture("kat6")
    sa, sb = M.strings(bwt_a), M.strings(bwt_b)
    want = M.oracle_bwt(0, [M.pack(sa, True)[0], M.pack(sb, True)[0]])
    dst, src = hip.HipBwt(0), hip.HipBwt(0)
    dst.load_fmd(np.frombuffer(img_a, np.uint8)); src.load_fmd(np.frombuffer(img_b, np.uint8))
    assert dst.merge(src) == (len(sb), sum(len(s) for s in sb), 1, len(sb) + sum(len(s) for s in sb))
    assert np.array_equal(dst.bwt(), want) and np.array_equal(src.bwt(), bwt_b)
    image = dst.save_fmd().tobytes()
    dst.close(); src.close()
    pa, pb, po = (str(tmp_path / f) for f in ("a.fmd", "b.fmd", "out.fmd"))
    open(pa, "wb").write(bytes(img_a)); open(pb, "wb").write(bytes(img_b))
    with _Env(RB2_MERGE_BATCH=20):
        p = subprocess.run([sys.executable, os.path.join(H.ROOT, "tools", "fmd_merge.py"), po, pa, pb, "--so", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, (p.stdout.decode(), p.stderr.decode()[-2000:])
    assert _greedy(sb, 20) >= 2
    assert "%d strings, %d symbols, %d batches" % (len(sb), sum(len(s) for s in sb), _greedy(sb, 20)) in p.stdout.decode(), p.stdout.decode()
    assert open(po, "rb").read() == image
