"""GPU tests of the FM-index queries (include/rb2_hip.h: rb2_hip_backward_search[_dev], rb2_hip_extend, rb2_hip_extract): every
device result must equal the numpy reference (tests/query_ref.py) on the BWT downloaded from the same index."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import query_ref as Q

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Env:
    def __init__(self, **kw):
        self.kw = kw
    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update({k: str(v) for k, v in self.kw.items()})
    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _batches(seed, rev, n=(300, 200, 250)):
    out, strings = [], []
    for i, k in enumerate(n):
        reads = H.repetitive_reads(k, seed=seed + i, max_len=40)
        out.append(H.encode_batch(reads, True, rev))
        strings += Q.inserted_strings(reads, True, rev)
    return out, strings


def _patterns(strings, rng, k=400):
    pats = []
    for _ in range(k):                                              # substrings of the strings, lengths 1..40
        s = strings[rng.randint(len(strings))]
        if len(s) == 0:
            continue
        a = rng.randint(len(s))
        pats.append(s[a:a + rng.randint(1, 41)].copy())
    pats += [rng.randint(1, 6, size=rng.randint(1, 41)).astype(np.uint8) for _ in range(150)]     # random
    pats += [np.concatenate([p, [0]]).astype(np.uint8) for p in pats[:100]]                       # trailing $
    pats += [np.zeros(0, np.uint8), np.array([0], np.uint8), np.array([1, 0, 2], np.uint8), np.array([0, 0], np.uint8),
             np.array([7, 1], np.uint8), np.array([3, 6], np.uint8)]                               # empty, `$`, malformed
    return pats


def _check_search(g, fm, pats):
    lo, hi, m = g.backward_search(pats)
    want = np.array([fm.backward_search(p) for p in pats], np.int64).reshape(-1, 3)
    got = np.stack([lo, hi, m], 1)
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, [(pats[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    # the same through the device-pointer variant
    pat, off = __import__("ropebwt2_amd.hipbwt", fromlist=["pack_patterns"]).pack_patterns(pats)
    n = len(pats)
    dp, do, dq = g.dev_alloc(len(pat)), g.dev_alloc(8 * (n + 1)), g.dev_alloc(24 * n)
    try:
        g.L.rb2_hip_memcpy(g.h, dp, pat.ctypes.data, len(pat), 0)
        g.L.rb2_hip_memcpy(g.h, do, off.ctypes.data, 8 * (n + 1), 0)
        g.backward_search_dev(n, dp, do, dq)
        res = np.zeros((n, 3), np.int64)
        g.L.rb2_hip_memcpy(g.h, res.ctypes.data, dq, 24 * n, 1)
    finally:
        for p in (dp, do, dq):
            g.dev_free(p)
    assert np.array_equal(res, want)
    return want


def _chains(fm, strings, rng, k=120):
    """bi-intervals reached by chains of backward and forward extensions of substrings (both strands indexed)"""
    iks, qs = [], []
    for _ in range(k):
        s = strings[rng.randint(len(strings))]
        if len(s) < 2 or (s == 5).any():
            continue
        a = rng.randint(len(s)); b = a + 1
        ik = fm.sym_interval(int(s[a]))
        iks.append(list(ik)); qs.append(s[a:b].copy())
        for _ in range(30):
            if rng.rand() < 0.5 and a > 0:
                a -= 1; ik = fm.extend(ik, True)[int(s[a])].tolist()
            elif b < len(s):
                b += 1; ik = fm.extend(ik, False)[Q.COMP[int(s[b - 1])]].tolist()
            else:
                break
            iks.append(list(ik)); qs.append(s[a:b].copy())
    return np.array(iks, np.int64), qs


def _check_extend(g, fm, iks):
    for is_back in (0, 1):
        got = g.extend(iks, is_back)
        want = np.stack([fm.extend(ik, is_back) for ik in iks])
        bad = np.flatnonzero((got != want).reshape(len(iks), -1).any(1))
        assert len(bad) == 0, [(iks[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:3]]


def _check_extract(g, fm, so, strings):
    n = int(fm.C[1])
    assert n == len(strings)
    ml = max(len(s) for s in strings) if strings else 0
    got = g.extract(np.arange(n), max(ml, 1))
    for r in range(n):
        assert np.array_equal(got[r], fm.walk(r)), r
    if so == 0:
        for k, s in enumerate(strings):
            assert np.array_equal(got[k], s), k
    else:
        assert sorted(x.tobytes() for x in got) == sorted(np.asarray(s, np.uint8).tobytes() for s in strings)
    if so == 1:
        rk = [x[::-1].tobytes() for x in got]
        assert rk == sorted(rk)
    # truncation and bad rows
    cut = 10
    fit, out, ln = g.extract_raw(np.arange(n), cut)
    lens = np.array([len(fm.walk(r)) for r in range(n)])
    assert np.array_equal(ln, np.where(lens > cut, -1, lens)) and fit == int((lens <= cut).sum())
    for r in np.flatnonzero(lens <= cut)[:50]:
        assert np.array_equal(out[r, :lens[r]], fm.walk(r))
    fit, out, ln = g.extract_raw([-1, n, n + 5, fm.N + 3, 0] if n else [-1, 0, 5], 50)
    assert ln[:-1].tolist() == [-2] * (len(ln) - 1)
    with pytest.raises(ValueError):
        g.extract([n], 5)


def _check_all(g, fm, so, strings, rev, seed):
    rng = np.random.RandomState(seed)
    _check_search(g, fm, _patterns(strings, rng))
    if rev:
        iks, qs = _chains(fm, strings, rng)
        _check_extend(g, fm, iks)
        for ik, q in zip(iks, qs):                                  # x[0] = lo(Q), x[1] = lo(revcomp Q), x[2] = count(Q)
            lo, hi, m = fm.backward_search(q)
            rlo = fm.backward_search(Q.revcomp(q))[0]
            assert ik.tolist() == [lo, rlo, hi - lo]
    else:
        iks = np.array([[rng.randint(0, fm.N + 1), rng.randint(0, fm.N + 1), 0] for _ in range(200)], np.int64)
        iks[:, 2] = [rng.randint(0, fm.N - x + 1) for x in iks[:, 0]]
        _check_extend(g, fm, iks)
    _check_extract(g, fm, so, strings)


@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("rev", [False, True])
def test_queries_match_reference(hip, so, rev):
    batches, strings = _batches(20 + so, rev)
    o, g = H.Oracle(so), hip.HipBwt(so)
    for b in batches[:-1]:
        o.insert_multi(b); g.insert_multi(b)
    g.wait()
    k = len(strings) - len(Q.inserted_strings(H.repetitive_reads(250, seed=22 + so, max_len=40), True, rev))
    fm = Q.FM(g.bwt())
    assert np.array_equal(fm.bwt, o.bwt())
    before = g.rope_hashes()
    _check_all(g, fm, so, strings[:k], rev, seed=so)
    assert g.rope_hashes() == before, "a query changed the index"
    o.insert_multi(batches[-1]); g.insert_multi(batches[-1])          # an insert after queries still matches the oracle
    assert np.array_equal(g.bwt(), o.bwt())
    fm = Q.FM(g.bwt())
    _check_search(g, fm, _patterns(strings, np.random.RandomState(5)))
    g.close(); o.close()


def test_lazy_insert_queried_without_wait(hip):
    batches, strings = _batches(60, False)
    g = hip.HipBwt(0)
    g.set_lazy(1)
    o = H.Oracle(0)
    for b in batches:
        o.insert_multi(b)
        g.insert_multi(b)                                           # may return with the rounds still queued
    lo, hi, m = g.backward_search([strings[5]])                     # no explicit wait
    fm = Q.FM(o.bwt())
    assert (lo[0], hi[0], m[0]) == fm.backward_search(strings[5])
    got = g.extract(np.arange(len(strings)), 41)
    assert all(np.array_equal(a, s) for a, s in zip(got, strings))
    g.close()


def test_forced_sparse_layout(hip):
    """an index that stays in the sparse (in-place) layout: locate(), the directory prefix, two-plane leaves"""
    rng = np.random.RandomState(3)
    reads = []
    for i in range(120):
        r = list(rng.randint(1, 5, size=int(rng.randint(1500, 2600))))
        for _ in range(int(rng.randint(0, 3))):                     # 0-2 runs of N per read
            at, n = int(rng.randint(0, len(r) - 1)), int(rng.randint(1, 300))
            r[at:at + n] = [5] * len(r[at:at + n])
        reads.append(np.array(r, np.uint8))
    reads += H.repetitive_reads(100, seed=71, max_len=40)
    with _Env(RB2_SPARSE_LAMBDA="1e18", RB2_SPARSE_MAXPEN="0"):
        o, g = H.Oracle(1), hip.HipBwt(1)
        strings = []
        for part in (reads[:50], reads[50:100], reads[100:]):
            buf = H.encode_batch(part, True, True)
            o.insert_multi(buf); g.insert_multi(buf)
            strings += Q.inserted_strings(part, True, True)
        assert g.layout_stats()["sparse_now"]
        fm = Q.FM(o.bwt())
        _check_all(g, fm, 1, strings, True, seed=9)
        assert g.layout_stats()["sparse_now"], "a query changed the layout"
        assert np.array_equal(g.bwt(), o.bwt())
    g.close(); o.close()


def test_load_ropes_index(hip):
    batches, strings = _batches(80, True)
    o = H.Oracle(2)
    for b in batches:
        o.insert_multi(b)
    g = hip.HipBwt(2)
    g.load_ropes([hip.hipbwt.encode_runs(o.rope(b)) for b in range(6)])
    fm = Q.FM(o.bwt())
    _check_all(g, fm, 2, strings, True, seed=4)
    g.close(); o.close()


def test_empty_index(hip):
    g = hip.HipBwt(0)
    lo, hi, m = g.backward_search(["", "A", "ACG$", "$", np.array([0, 1], np.uint8)])
    assert lo.tolist() == [0, 0, 0, 0, -1] and hi.tolist() == [0, 0, 0, 0, -1] and m.tolist() == [0, 0, 0, 0, -1]
    assert g.count(["A", ""]).tolist() == [0, 0]
    ok = g.extend([[0, 0, 0]], 1)
    assert (ok == 0).all()
    fit, out, ln = g.extract_raw([0, 1], 4)
    assert fit == 0 and ln.tolist() == [-2, -2]
    g.close()


def test_piece_and_rope_boundaries(hip):
    """ranks exactly on the first row of every piece (b,x) and every rope, and one row either side"""
    batches, strings = _batches(90, True)
    g = hip.HipBwt(0)
    for b in batches:
        g.insert_multi(b)
    fm = Q.FM(g.bwt())
    cnt = g.counts()                                                # piece (b,x) holds the b's of rope x
    edges = set()
    for b in range(6):
        row = int(fm.C[b])
        for x in range(6 if b else 1):
            for d in (-1, 0, 1):
                edges.add(row + d)
            row += int(cnt[x, b]) if b else int(cnt[:, 0].sum())
    edges.add(fm.N)
    edges = sorted(e for e in edges if 0 <= e <= fm.N)
    iks = np.array([[e, 0, s] for e in edges for s in (0, 1, 2) if e + s <= fm.N], np.int64)
    _check_extend(g, fm, iks)
    iks[:, [0, 1]] = iks[:, [1, 0]]
    _check_extend(g, fm, iks)
    rows = [e for e in edges if e < fm.C[1]]
    got = g.extract(rows, 41)
    for r, s in zip(rows, got):
        assert np.array_equal(s, fm.walk(r))
    g.close()


def test_chunked_staging(hip):
    batches, strings = _batches(100, True)
    g = hip.HipBwt(1)
    for b in batches:
        g.insert_multi(b)
    fm = Q.FM(g.bwt())
    with _Env(RB2_QUERY_CHUNK=7):
        _check_all(g, fm, 1, strings, True, seed=12)
    g.close()


def test_sharded_handle_is_fatal(hip):
    """a query on one rank of a sharded index is fatal with a message (reported through the fatal handler, which leaves by _exit)"""
    code = ("import sys, os, ctypes as C; sys.path.insert(0, %r)\n"
            "from ropebwt2_amd import MultiBwt\n"
            "from ropebwt2_amd.hipbwt import load_hip_lib\n"
            "L = load_hip_lib()\n"
            "CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)\n"
            "def h(user, msg):\n"
            "    sys.stdout.write('fatal: ' + msg.decode()); sys.stdout.flush(); os._exit(7)\n"
            "cb = CB(h)\n"
            "L.rb2_hip_set_fatal_handler(cb, None)\n"
            "m = MultiBwt(0, [0, 0])\n"
            "m.engine(0).backward_search(['ACGT'])\n"
            "print('NOT FATAL')\n") % ROOT
    p = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 7, (p.returncode, p.stderr.decode()[-400:])
    assert b"fatal: [rb2_hip] backward_search" in p.stdout and b"sharded index" in p.stdout, p.stdout


def test_scale_io_4m_reads(hip):
    n, L = 4_000_000, 101
    g = hip.HipBwt(0)
    p = g.dev_alloc(n * (L + 1))
    g.synth_reads(p, 0, n, L, seed=42)
    g.insert_multi_dev(p, n * (L + 1))
    g.dev_free(p)
    rng = np.random.RandomState(1)
    rows = np.unique(np.concatenate([rng.randint(0, n, size=2000), [0, 1, n - 2, n - 1]]))
    got = g.extract(rows, L)
    for r, s in zip(rows, got):
        assert np.array_equal(s, H.splitmix_bases(1, L, seed=42, first=int(r))[0]), r
    reads = [np.concatenate([H.splitmix_bases(1, L, seed=42, first=int(r))[0], [0]]).astype(np.uint8) for r in rows[:500]]
    lo, hi, m = g.backward_search(reads)
    assert (m == L + 1).all()
    assert (lo >= g.counts()[:, 0].sum()).all()                     # a read's whole suffix lies behind the $ block
    assert (hi - lo == 1).all()                                     # multiplicity of a random 101-mer
    g.close()
