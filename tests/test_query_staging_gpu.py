"""GPU test of the staging the host variants of the FM-index queries share (csrc/rb2_query_host.h: stage_inputs, staged_results,
staged_records): every family in turn on ONE handle, so that qin / qout / qbytes are reused across families with sizes going up and down,
in chunks of 1, 3 and everything at once, in both layouts.  Ten items per call: at 3 the last chunk is partial.  Every result must equal
the Python references (query_ref, smem_ref, locate_ref, overlap_ref); what they are compared on is computed once, in `case`."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import locate_ref as LR
import overlap_ref as OR
import query_ref as Q
import smem_ref as SR
from ropebwt2_amd.hipbwt import pack_patterns
from test_locate_gpu import _locate_dev
from test_overlap_gpu import FILL, _from_dev, _to_dev, overlap_dev, string_ids_dev
from test_query_gpu import _Env

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FORCED = dict(RB2_SPARSE_LAMBDA="1e18", RB2_SPARSE_MAXPEN="0")       # the forced-sparse environment of test_query_gpu.py
N_ITEMS = 10
EMPTY, BAD = (3, 9), 4                                               # empty items: the first of a chunk of 3, and a last chunk with no byte at all; a malformed
                                                                     # one in the middle of a chunk of 3


def reads():
    rng = np.random.RandomState(2024)
    return [rng.randint(1, 5, size=int(rng.randint(5, 41))).astype(np.uint8) for _ in range(60)]


def _smem_raw(fm, qs, min_len, min_occ, cap):
    """(stored, mem (n, cap, 5), cnt (n,)) as HipBwt.smem_raw returns them, from smem_ref.smems"""
    mem = np.zeros((len(qs), cap, 5), np.int64)
    cnt = np.zeros(len(qs), np.int64)
    for i, q in enumerate(qs):
        w = SR.smems(fm, q, min_len, min_occ)
        cnt[i] = -1 if w is None else len(w)
        if w is not None:
            mem[i, :min(len(w), cap)] = w[:cap]
    return int(np.minimum(np.maximum(cnt, 0), cap).sum()), mem, cnt


class _Case:
    """the inputs of every family (ten items each) and what the references answer"""
    def __init__(self, bwt):
        self.fm = fm = Q.FM(bwt)
        self.n = n = int(fm.C[1])
        strings = Q.inserted_strings(reads(), True, True)
        assert n == len(strings) == 120
        rng = np.random.RandomState(5)
        qs = []
        for k in rng.choice(n, size=N_ITEMS, replace=False):        # strings of the index with a base changed: several SMEMs, several overlap lengths
            q = strings[k].copy()
            q[len(q) // 2] = 1 + q[len(q) // 2] % 4
            qs.append(q)
        for i in EMPTY:
            qs[i] = np.zeros(0, np.uint8)
        qs[BAD] = np.array([1, 0, 2], np.uint8)
        self.qs = qs
        self.smem = {cap: _smem_raw(fm, qs, 1, 1, cap) for cap in (8, 1)}
        c = self.smem[8][2]
        assert c[BAD] == -1 and all(c[i] == 0 for i in EMPTY) and (c > 1).sum() >= 5 and c.max() <= 8, c
        assert self.smem[1][0] == (c > 0).sum() and np.array_equal(self.smem[1][2], c)             # cap 1: the surplus is counted, one record kept
        self.overlap = {cap: OR.overlap_raw(fm, qs, 1, cap) for cap in (40, 1)}
        c = self.overlap[40][2]
        assert c[BAD] == -1 and all(c[i] == 0 for i in EMPTY) and (c > 1).sum() >= 5 and c.max() <= 40, c
        lo = rng.randint(0, fm.N - 20, size=N_ITEMS)
        self.iv = np.stack([lo, lo + rng.randint(2, 12, size=N_ITEMS)], 1)
        self.iv[EMPTY[0]], self.iv[EMPTY[1]], self.iv[BAD] = (7, 7), (fm.N, fm.N), (5, 4)
        self.locate = {cap: LR.locate_raw(fm, self.iv, cap) for cap in (16, 1)}
        c = self.locate[16][2]
        assert c[BAD] == -1 and (c > 1).sum() == 7 and c.max() <= 16, c
        zlo = rng.randint(0, n - 10, size=N_ITEMS)
        self.zv = np.stack([zlo, zlo + rng.randint(2, 9, size=N_ITEMS)], 1)
        self.zv[EMPTY[0]], self.zv[EMPTY[1]], self.zv[BAD] = (7, 7), (n, n), (0, n + 1)
        self.ids = {cap: OR.string_ids_raw(fm, self.zv, cap) for cap in (8, 1)}
        c = self.ids[8][2]
        assert c[BAD] == -1 and (c > 1).sum() == 7 and c.max() <= 8, c
        self.pats = [q[len(q) // 2:].copy() for q in qs]            # (from the changed base on: most stop short of their length)
        self.pats[0] = np.concatenate([strings[3], [0]]).astype(np.uint8)                           # a whole string and its end
        self.search = np.array([fm.backward_search(p) for p in self.pats], np.int64)
        assert self.search[BAD].tolist() == [-1, -1, -1] and self.search[EMPTY[0]].tolist() == [0, fm.N, 0] and self.search[0, 2] == len(self.pats[0])
        iks = []
        for k in rng.choice(n, size=N_ITEMS, replace=False):        # the bi-intervals of substrings of the strings
            s = strings[k]
            p = s[1:1 + rng.randint(1, 4)]
            lo_, hi_, m = fm.backward_search(p)
            assert m == len(p)
            iks.append([lo_, fm.backward_search(Q.revcomp(p))[0], hi_ - lo_])
        self.iks = np.array(iks, np.int64)
        self.extend = {b: np.stack([fm.extend(ik, b) for ik in self.iks]) for b in (0, 1)}
        assert all((self.extend[b][:, 1:5, 2] > 0).any() for b in (0, 1))
        self.rows = rng.choice(n, size=N_ITEMS, replace=False).astype(np.int64)
        self.rows[BAD] = n                                          # outside the $ block
        walks = [fm.walk(int(r)) if r < n else None for r in self.rows]
        self.max_len = 20
        self.ext_len = np.array([-2 if w is None else len(w) if len(w) <= self.max_len else -1 for w in walks], np.int64)
        assert (self.ext_len == -1).sum() >= 2 and (self.ext_len >= 0).sum() >= 3, self.ext_len
        self.walks = walks


def _build(hip, forced):
    """the 60 strings and their reverse complements in two batches, then a suffix array sampled every fourth row"""
    rs = reads()
    with _Env(**(FORCED if forced else {})):
        g = hip.HipBwt(0)
        for part in (rs[:30], rs[30:]):
            g.insert_multi(H.encode_batch(part, True, True))
        g.wait()
    g.build_ssa(2)
    return g


@pytest.fixture(scope="module")
def case(hip):
    g = _build(hip, False)
    bwt = g.bwt()
    g.close()
    return _Case(bwt)


@pytest.fixture(scope="module", params=["dense", "sparse"])
def idx(request, hip, case):
    g = _build(hip, request.param == "sparse")
    assert g.layout_stats()["sparse_now"] == (request.param == "sparse"), g.layout_stats()
    yield g
    g.close()


def _same(name, got, want):
    assert got[0] == want[0] and np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1]), (name, got[0], want[0], got[2].tolist(), want[2].tolist())


def _sequence(g, c):
    """smem, locate, overlap, string_ids, backward_search, extend, extract, smem: the staged records shrink and grow from call to call"""
    _same("smem 8", g.smem_raw(c.qs, 1, 1, 8), c.smem[8])
    _same("locate 1", g.locate_raw(c.iv, 1), c.locate[1])
    _same("overlap 40", g.overlap_raw(c.qs, 1, 40), c.overlap[40])
    _same("string_ids 1", g.string_ids_raw(c.zv, 1), c.ids[1])
    assert np.array_equal(np.stack(g.backward_search(c.pats), 1), c.search)
    for b in (0, 1):
        assert np.array_equal(g.extend(c.iks, b), c.extend[b]), b
    fit, out, ln = g.extract_raw(c.rows, c.max_len)
    assert np.array_equal(ln, c.ext_len) and fit == (c.ext_len >= 0).sum()
    assert all(np.array_equal(out[i, :ln[i]], c.walks[i]) for i in np.flatnonzero(ln >= 0))
    _same("smem 1", g.smem_raw(c.qs, 1, 1, 1), c.smem[1])             # cap 1: the slot is the first SMEM, the others are counted only
    _same("locate 16", g.locate_raw(c.iv, 16), c.locate[16])
    _same("overlap 1", g.overlap_raw(c.qs, 1, 1), c.overlap[1])
    _same("string_ids 8", g.string_ids_raw(c.zv, 8), c.ids[8])


@pytest.mark.parametrize("chunk", [1, 3, None])
def test_every_family_on_one_handle(idx, case, chunk):
    with _Env(**({} if chunk is None else {"RB2_QUERY_CHUNK": chunk})):
        _sequence(idx, case)


def _smem_dev(g, qs, min_len, min_occ, max_mems):
    qry, off = pack_patterns(qs)
    mem = np.full((len(qs), max_mems, 5), FILL, np.int64)
    cnt = np.full(len(qs), FILL, np.int64)
    ptrs = _to_dev(g, (qry, off, mem, cnt))
    try:
        g.smem_dev(len(qs), ptrs[0], ptrs[1], ptrs[2], ptrs[3], min_len, min_occ, max_mems)
        _from_dev(g, ptrs[2:], (mem, cnt))
    finally:
        for d in ptrs:
            g.dev_free(d)
    return mem, cnt


def _search_dev(g, pats):
    pat, off = pack_patterns(pats)
    out = np.full((len(pats), 3), FILL, np.int64)
    ptrs = _to_dev(g, (pat, off, out))
    try:
        g.backward_search_dev(len(pats), ptrs[0], ptrs[1], ptrs[2])
        _from_dev(g, ptrs[2:], (out,))
    finally:
        for d in ptrs:
            g.dev_free(d)
    return out


def _same_dev(name, dev, host):
    """the device variant's (records, counts) against the host variant's (stored, records, counts): equal where a record was stored,
    untouched elsewhere (the host variant returns zeros there)"""
    rec, cnt = dev
    _, h_rec, h_cnt = host
    live = np.arange(h_rec.shape[1])[None, :] < np.minimum(np.maximum(h_cnt, 0), h_rec.shape[1])[:, None]
    assert np.array_equal(cnt, h_cnt) and np.array_equal(rec[live], h_rec[live]) and (rec[~live] == FILL).all() and (h_rec[~live] == 0).all(), name


def test_device_variants_equal_host_variants(idx, case):
    g, c = idx, case
    with _Env(RB2_QUERY_CHUNK=3):
        for cap in (8, 1):
            _same_dev("smem", _smem_dev(g, c.qs, 1, 1, cap), g.smem_raw(c.qs, 1, 1, cap))
            _same_dev("string_ids", string_ids_dev(g, c.zv, cap), g.string_ids_raw(c.zv, cap))
        for cap in (16, 1):
            _same_dev("locate", _locate_dev(g, c.iv, cap), g.locate_raw(c.iv, cap))
        for cap in (40, 1):
            _same_dev("overlap", overlap_dev(g, c.qs, 1, cap), g.overlap_raw(c.qs, 1, cap))
        assert np.array_equal(_search_dev(g, c.pats), np.stack(g.backward_search(c.pats), 1))
    _same("smem 8", g.smem_raw(c.qs, 1, 1, 8), c.smem[8])             # (and the host variant still answers as the reference does)


def test_layout_and_index_unchanged(request, idx, case):
    """after the tests above: the queries left the layout alone, and both layouts hold the index the references read (the export
    re-lays a sparse index out, so this comes last)"""
    assert idx.layout_stats()["sparse_now"] == ("sparse" in request.node.name), idx.layout_stats()
    assert np.array_equal(idx.bwt(), case.fm.bwt)


def test_no_items_and_bad_parameters(hip):
    """smem returns for n = 0 before it looks at its parameters; locate checks max_hits first and is fatal (tests/query_staging_child.py)"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "query_staging_child.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out = p.stdout.decode()
    assert p.returncode == 7 and "NOT FATAL" not in out, (p.returncode, out, p.stderr.decode()[-1500:])
    assert "smem returned 0" in out and "handler: [rb2_hip] locate: max_hits must be at least 1 (got 0)" in out, out
