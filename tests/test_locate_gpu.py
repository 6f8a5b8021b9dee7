"""GPU tests of the sampled suffix array (include/rb2_hip.h: rb2_hip_ssa_build / _drop / _info, rb2_hip_locate[_dev]; kernels k_ssa_build,
k_locate in csrc/rb2_query.h): every place the device reports must equal the numpy model (tests/locate_ref.py) on the BWT of the same
index, and through HipBwt.find the brute-force places that never look at a BWT.  Small shapes: what can go wrong is addressing -- the
sample slots, the head[] of the whole-string rows, leaves and superblocks of both layouts -- not volume."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fmd_ref
import helpers as H
import locate_ref as LR
import query_ref as Q
from test_locate_ref import patterns, string_sets
from test_query_gpu import _Env, _batches
from test_query_layouts_gpu import _Models, _build_dense, _build_sparse

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = [0, 3, 5, 30]                                                # 0: every row is a sample; 30: 2^s > N, only row 0 is, every answer comes through head[]
FILL = -7                                                            # what the device variant must leave in the records it does not write


@pytest.fixture(scope="module")
def models():
    ms = _Models()
    yield ms
    ms.made.clear()


def _small(hip, so):
    batches, strings = _batches(200 + so, True)
    g = hip.HipBwt(so)
    for b in batches:
        g.insert_multi(b)
    return g, Q.FM(g.bwt()), strings


@pytest.fixture(scope="module", params=["dense-io", "dense-rclo", "D", "S", "fmd"])
def idx(request, hip, models):
    """(handle, model): a dense index of some thousands of symbols in input order and in RCLO; layout D (every piece longer than two
    superblocks) and layout S (sparse, split leaves) of test_query_layouts_gpu.py; an index loaded from a file the reference wrote"""
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
    g.kind = kind
    yield g, fm
    g.close()


@pytest.fixture(scope="module")
def small(hip):
    g, fm, strings = _small(hip, 0)
    assert fm.N > 5000
    g.build_ssa(3)
    yield g, fm
    g.close()


def _locate_dev(g, iv, max_hits):
    """locate_dev on buffers filled with FILL: (hit, cnt) as the device left them"""
    iv = np.ascontiguousarray(np.asarray(iv, np.int64).reshape(-1, 2))
    n = len(iv)
    hit = np.full((n, max_hits, 2), FILL, np.int64)
    cnt = np.full(n, FILL, np.int64)
    di, dh, dc = g.dev_alloc(iv.nbytes), g.dev_alloc(hit.nbytes), g.dev_alloc(cnt.nbytes)
    try:
        for d, a in ((di, iv), (dh, hit), (dc, cnt)):
            g.L.rb2_hip_memcpy(g.h, d, a.ctypes.data, a.nbytes, 0)
        g.locate_dev(n, di, dh, dc, max_hits)
        g.L.rb2_hip_memcpy(g.h, hit.ctypes.data, dh, hit.nbytes, 1)
        g.L.rb2_hip_memcpy(g.h, cnt.ctypes.data, dc, cnt.nbytes, 1)
    finally:
        for d in (di, dh, dc):
            g.dev_free(d)
    return hit, cnt


def _first_bad(got, want):
    bad = np.flatnonzero((got != want).any(1))
    return "%d of %d rows differ; first: row %d got %s want %s" % (len(bad), len(want), bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.parametrize("s", STEPS)
def test_every_row(idx, s):
    """[x, x + 1) for every row x, and [0, N) with max_hits = N, exactly as the model"""
    g, fm = idx
    N, n = fm.N, int(fm.C[1])
    sid, pos, lens = LR.suffix_array(fm)
    want = np.stack([sid, pos], 1)
    before = g.layout_stats()
    assert g.build_ssa(s) == (N + (1 << s) - 1) >> s
    inf = g.ssa_info()
    assert inf == {"valid": True, "log2_step": s, "samples": (N + (1 << s) - 1) >> s, "device_bytes": 16 * inf["samples"] + 16 * n}, inf
    x = np.arange(N, dtype=np.int64)
    stored, hit, cnt = g.locate_raw(np.stack([x, x + 1], 1), 1)
    assert stored == N and (cnt == 1).all()
    assert np.array_equal(hit[:, 0], want), _first_bad(hit[:, 0], want)
    stored, hit, cnt = g.locate_raw([(0, N)], N)
    assert stored == N and cnt.tolist() == [N]
    assert np.array_equal(hit[0], want), _first_bad(hit[0], want)
    dh, dc = _locate_dev(g, [(0, N), (N, N)], N)                     # the device-pointer variant, and the empty interval at the very end
    assert dc.tolist() == [N, 0] and np.array_equal(dh[0], want) and (dh[1] == FILL).all()
    assert g.layout_stats() == before, "building or locating changed the layout"


@pytest.mark.parametrize("max_hits", [1, 3])
def test_truncation_and_malformed_intervals(small, max_hits):
    g, fm = small
    N = fm.N
    iv = [(7, 7), (N, N), (11, 12), (N - 1, N), (100, 103), (0, 4), (2000, 3000), (-1, 2), (0, N + 1), (5, 4), (N - 3, N)]
    sizes = [hi - lo for lo, hi in iv[:7]]
    assert sorted(set(sizes)) == [0, 1, 3, 4, 1000]
    w_stored, w_hit, w_cnt = LR.locate_raw(fm, iv, max_hits)
    assert w_cnt.tolist() == sizes + [-1, -1, -1, 3]
    assert w_stored == sum(min(c, max_hits) for c in w_cnt if c >= 0)
    stored, hit, cnt = g.locate_raw(iv, max_hits)
    assert stored == w_stored and np.array_equal(cnt, w_cnt)
    assert np.array_equal(hit, w_hit)                               # zeros beyond min(cnt, max_hits), and for the malformed intervals
    dh, dc = _locate_dev(g, iv, max_hits)
    assert np.array_equal(dc, w_cnt)
    live = np.arange(max_hits)[None, :] < np.minimum(np.maximum(w_cnt, 0), max_hits)[:, None]
    assert np.array_equal(dh[live], w_hit[live]) and (dh[~live] == FILL).all()
    with pytest.raises(ValueError):
        g.locate(iv, max_hits)
    got = g.locate(iv[:7], max_hits)
    assert [len(h) for h in got] == [min(c, max_hits) for c in sizes]
    assert g.locate([], max_hits) == []


def test_chunked_staging(small):
    g, fm = small
    rng = np.random.RandomState(4)
    lo = rng.randint(0, fm.N, size=100)
    iv = np.stack([lo, np.minimum(lo + rng.randint(0, 12, size=100), fm.N)], 1)
    iv[17] = (5, 4)
    want = LR.locate_raw(fm, iv, 5)
    plain = g.locate_raw(iv, 5)
    with _Env(RB2_QUERY_CHUNK=7):
        chunked = g.locate_raw(iv, 5)
        dh, dc = _locate_dev(g, iv, 5)
    for got in (plain, chunked):
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    live = np.arange(5)[None, :] < np.maximum(want[2], 0)[:, None]
    assert np.array_equal(dc, want[2]) and np.array_equal(dh[live], want[1][live])


@pytest.mark.parametrize("name", ["repetitive-both", "tiny-both"])
def test_find_against_brute_force(hip, name):
    """patterns to places in one call; input order, so string k is the k-th string inserted and brute force over the strings applies"""
    reads, rev = string_sets()[name]
    strings = Q.inserted_strings(reads, True, rev)
    g = hip.HipBwt(0)
    half = len(reads) // 2
    for part in (reads[:half], reads[half:]):
        g.insert_multi(H.encode_batch(part, True, rev))
    N = sum(len(s) + 1 for s in strings)
    g.build_ssa(2)
    pats = patterns(strings, np.random.RandomState(len(strings)))
    pats += [np.array([1, 0, 2], np.uint8)]                         # malformed: no places
    got = g.find(pats, max_hits=N)
    hits = 0
    for p, h in zip(pats, got):
        places = set(map(tuple, h.tolist()))
        want = set() if (np.asarray(p[:-1]) == 0).any() else LR.brute_places(strings, p)
        assert len(places) == len(h) and places == want, p.tolist()
        hits += bool(len(h))
    assert hits > 100 or name == "tiny-both"
    few = g.find(pats[:20], max_hits=2)                              # max_hits caps every pattern
    assert all(len(a) == min(len(b), 2) and np.array_equal(a, b[:2]) for a, b in zip(few, got))
    txt = "".join("$ACGTN"[c] for c in pats[0])
    assert np.array_equal(g.find([txt], max_hits=N)[0], got[0])
    g.close()


def _child(stage):
    p = subprocess.run([sys.executable, os.path.join(HERE, "locate_lifecycle_child.py"), stage], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p.returncode, p.stdout.decode(), p.stderr.decode()[-1500:]


def test_locate_before_build_is_fatal(hip):
    rc, out, err = _child("before")
    assert rc == 7 and "NOT FATAL" not in out, (rc, out, err)
    assert "'valid': False" in out and "handler: [rb2_hip] locate" in out and "rb2_hip_ssa_build" in out, out


def test_insert_drops_the_array(hip):
    rc, out, err = _child("stale")
    assert rc == 7 and "NOT FATAL" not in out, (rc, out, err)
    assert "built {'valid': True, 'log2_step': 3" in out and "located [4]" in out, out
    assert "after insert {'valid': False, 'log2_step': 0, 'samples': 0, 'device_bytes': 0}" in out, out
    assert "handler: [rb2_hip] locate" in out and "rb2_hip_ssa_build" in out, out


def test_lifecycle(hip):
    """an empty index, a rebuild after an insert, a re-layout that keeps the array (a checksum takes a sparse index back to the dense
    layout without an insert), drop, and the loaders and reset: see the child"""
    rc, out, err = _child("life")
    assert rc == 0 and "STAGE OK" in out, (rc, out, err)


def test_callers_stream(hip):
    """locate_dev after rb2_hip_use_stream on a torch stream, results read on that stream with no host synchronisation in between
    (in the child: torch opens the device first there)"""
    rc, out, err = _child("stream")
    assert rc == 0 and "STAGE OK" in out, (rc, out, err)
