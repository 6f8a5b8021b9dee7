"""GPU tests of the SMEM query (include/rb2_hip.h: rb2_hip_smem[_dev], kernel k_smem): records and counts must equal the numpy model
(tests/smem_ref.py, computed from the definition) on the BWT downloaded from the same index."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import query_ref as Q
import smem_ref as S
from test_query_gpu import _Env, _batches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [(1, 1), (12, 1), (1, 2), (5, 5)]                           # (min_len, min_occ)
MALFORMED = [np.array([1, 0, 2], np.uint8), np.array([0], np.uint8), np.array([7, 1], np.uint8), np.array([3, 4, 6], np.uint8),
             np.array([2, 2, 0], np.uint8)]


def _queries(strings, rng, k=400, piece=25, rand_len=80):
    """queries built to have several SMEMs with ends inside them; the malformed ones go last"""
    strings = [s for s in strings if len(s)]
    pick = lambda: strings[rng.randint(len(strings))]

    def sub(lo=1):
        s = pick(); n = rng.randint(lo, piece + 1); a = rng.randint(max(len(s) - n, 0) + 1)
        return s[a:a + n].copy()

    def glued():
        return np.concatenate([sub(4) for _ in range(rng.randint(2, 4))]).astype(np.uint8)

    qs = []
    for _ in range(k // 10):
        qs.append(pick()[:200].copy())                              # whole strings ...
        qs.append(sub())                                            # ... and substrings
    for _ in range(k // 4):
        qs.append(glued())                                          # substrings of different strings glued together
    for _ in range(k // 5):
        q = glued()                                                 # the same with 1-3 substituted bases
        for at in rng.randint(len(q), size=rng.randint(1, 4)):
            q[at] = 1 + (q[at] + rng.randint(0, 3)) % 4 if q[at] < 5 else 1
        qs.append(q)
    for i in range(k // 8):
        q = glued()                                                 # with N at the first, the last or an inner position
        q[[0, len(q) - 1, rng.randint(1, len(q) - 1)][i % 3]] = 5
        if i % 7 == 0:
            q[[0, -1]] = 5
        qs.append(q)
    for _ in range(k // 5):
        qs.append(rng.randint(1, 5, size=rng.randint(1, rand_len + 1)).astype(np.uint8))     # random ACGT
    qs += [np.array([c], np.uint8) for c in (1, 2, 3, 4, 5)] + [np.zeros(0, np.uint8), np.full(9, 5, np.uint8), np.array([5, 5], np.uint8)]
    return qs + [m.copy() for m in MALFORMED]


class _Case:
    """an index (its batches, its strings), the model of it and the queries, with the model's answers computed once per parameter pair"""
    def __init__(self, batches, strings, so, seed, **kw):
        self.batches, self.strings, self.so = batches, strings, so
        o = H.Oracle(so)
        for b in batches:
            o.insert_multi(b)
        self.bwt = o.bwt()
        self.ropes = [o.rope(b) for b in range(6)]
        o.close()
        self.fm = Q.FM(self.bwt)
        self.qs = _queries(strings, np.random.RandomState(seed), **kw)
        self.tabs = [None if S.malformed(q) else S.occ_table(self.fm, q) for q in self.qs]
        self.memo = {}

    def want(self, min_len, min_occ):
        key = (min_len, min_occ)
        if key not in self.memo:
            self.memo[key] = [None if t is None else S.smems_from_table(self.fm, q, t, min_len, min_occ) for q, t in zip(self.qs, self.tabs)]
        return self.memo[key]

    def engine(self, hip, lazy=False):
        g = hip.HipBwt(self.so)
        if lazy:
            g.set_lazy(1)
        for b in self.batches:
            g.insert_multi(b)
        return g


_cases = {}


def _case(so):
    if so not in _cases:
        batches, strings = _batches(30 + so, True)
        _cases[so] = _Case(batches, strings, so, seed=so)
    return _cases[so]


@pytest.fixture(scope="module", params=[0, 1, 2])
def idx(request, hip):
    c = _case(request.param)
    g = c.engine(hip)
    assert np.array_equal(g.bwt(), c.bwt)                            # the model reads the BWT this index holds
    yield g, c
    g.close()


def _compare(c, want, stored, mem, cnt, max_mems, fill):
    """mem, cnt against the model; records no query wrote must still hold `fill`"""
    total = 0
    for i, w in enumerate(want):
        if w is None:
            assert cnt[i] == -1 and (mem[i] == fill).all(), (i, c.qs[i].tolist())
            continue
        k = min(len(w), max_mems)
        assert cnt[i] == len(w), (i, c.qs[i].tolist(), int(cnt[i]), w.tolist())
        assert np.array_equal(mem[i, :k], w[:k]), (i, c.qs[i].tolist(), mem[i, :k].tolist(), w[:k].tolist())
        assert (mem[i, k:] == fill).all(), i
        total += k
    assert stored == total == int(np.minimum(np.maximum(cnt, 0), max_mems).sum())


def _check(g, c, min_len, min_occ, max_mems=64):
    want = c.want(min_len, min_occ)
    stored, mem, cnt = g.smem_raw(c.qs, min_len, min_occ, max_mems)
    assert mem.shape == (len(c.qs), max_mems, 5)
    _compare(c, want, stored, mem, cnt, max_mems, 0)
    return want


def _check_dev(g, c, min_len, min_occ, max_mems):
    from ropebwt2_amd.hipbwt import pack_patterns
    qry, off = pack_patterns(c.qs)
    n = len(c.qs)
    mem = np.full((n, max_mems, 5), -7, np.int64)
    cnt = np.full(n, -7, np.int64)
    dq, do, dm, dc = g.dev_alloc(len(qry)), g.dev_alloc(8 * (n + 1)), g.dev_alloc(mem.nbytes), g.dev_alloc(8 * n)
    try:
        g.L.rb2_hip_memcpy(g.h, dq, qry.ctypes.data, len(qry), 0)
        g.L.rb2_hip_memcpy(g.h, do, off.ctypes.data, 8 * (n + 1), 0)
        g.L.rb2_hip_memcpy(g.h, dm, mem.ctypes.data, mem.nbytes, 0)
        g.L.rb2_hip_memcpy(g.h, dc, cnt.ctypes.data, 8 * n, 0)
        g.smem_dev(n, dq, do, dm, dc, min_len, min_occ, max_mems)
        g.L.rb2_hip_memcpy(g.h, mem.ctypes.data, dm, mem.nbytes, 1)
        g.L.rb2_hip_memcpy(g.h, cnt.ctypes.data, dc, 8 * n, 1)
    finally:
        for p in (dq, do, dm, dc):
            g.dev_free(p)
    stored = int(np.minimum(np.maximum(cnt, 0), max_mems).sum())
    _compare(c, c.want(min_len, min_occ), stored, mem, cnt, max_mems, -7)       # what the kernel does not write stays as it was


def _assert_not_vacuous(c):
    """the conditions on the model's answers that keep the comparisons from passing on nothing"""
    good = [i for i, t in enumerate(c.tabs) if t is not None]
    assert len(c.qs) >= 380 and len(c.qs) - len(good) == len(MALFORMED)
    w11, w55 = c.want(1, 1), c.want(5, 5)
    n11 = np.array([len(w11[i]) for i in good])
    assert (n11 >= 2).sum() * 4 >= len(good), (n11 >= 2).sum()
    assert (n11 >= 4).sum() >= 10
    assert sum(1 for i in good if len(w55[i])) >= 20
    lost = sum(1 for i in good if {tuple(r[:2]) for r in w11[i].tolist()} - {tuple(r[:2]) for r in w55[i].tolist()})
    assert lost >= 20, lost
    assert (n11 > 1).sum() >= 50                                    # truncated by max_mems = 1
    assert sum(1 for i in good if len(c.want(12, 1)[i]) < len(w11[i])) >= 20
    assert sum(1 for i in good if len(c.want(1, 2)[i])) >= 20
    for w in w11:
        if w is not None and len(w) > 1:
            assert (np.diff(w[:, 0]) > 0).all() and (np.diff(w[:, 1]) > 0).all()


@pytest.mark.parametrize("min_len,min_occ", PARAMS)
def test_smems_match_model(idx, min_len, min_occ):
    g, c = idx
    _assert_not_vacuous(c)
    before = g.rope_hashes()
    _check(g, c, min_len, min_occ)
    assert g.rope_hashes() == before, "a query changed the index"


@pytest.mark.parametrize("max_mems", [1, 2])
def test_truncated_by_max_mems(idx, max_mems):
    g, c = idx
    want = _check(g, c, 1, 1, max_mems)
    assert sum(1 for w in want if w is not None and len(w) > max_mems) >= (50 if max_mems == 1 else 10)


def test_python_lists(idx):
    g, c = idx
    n = len(c.qs) - len(MALFORMED)
    want = c.want(1, 1)
    got, cnt = g.smem(c.qs[:n], max_mems=3)
    assert cnt.tolist() == [len(w) for w in want[:n]]
    assert all(r.shape == (min(len(w), 3), 5) and np.array_equal(r, w[:3]) for r, w in zip(got, want))
    with pytest.raises(ValueError):
        g.smem(c.qs)
    got, cnt = g.smem([])
    assert got == [] and len(cnt) == 0
    txt = "".join("$ACGTN"[x] for x in c.qs[40])
    assert np.array_equal(g.smem([txt])[0][0], want[40])


@pytest.mark.parametrize("min_len,min_occ,max_mems", [(1, 1, 64), (5, 5, 64), (1, 1, 2)])
def test_device_pointer_variant(idx, min_len, min_occ, max_mems):
    g, c = idx
    _check_dev(g, c, min_len, min_occ, max_mems)


def test_chunked_staging(idx):
    g, c = idx
    with _Env(RB2_QUERY_CHUNK=7):
        _check(g, c, 1, 1)
        _check(g, c, 5, 5, 2)
        _check_dev(g, c, 1, 2, 64)


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
    parts = (reads[:50], reads[50:100], reads[100:])
    with _Env(RB2_SPARSE_LAMBDA="1e18", RB2_SPARSE_MAXPEN="0"):
        c = _Case([H.encode_batch(p, True, True) for p in parts], Q.inserted_strings(reads, True, True), 1, seed=8, k=150, rand_len=30)
        g = c.engine(hip)
        assert g.layout_stats()["sparse_now"]
        want = _check(g, c, 1, 1)
        assert sum(1 for w in want if w is not None and len(w) >= 2) >= 30
        _check(g, c, 5, 2, 2)
        _check_dev(g, c, 1, 1, 64)
        assert g.layout_stats()["sparse_now"], "a query changed the layout"
        assert np.array_equal(g.bwt(), c.bwt)                        # (the export re-lays the index out: last)
    g.close()


def test_lazy_insert_queried_without_wait(hip):
    c = _case(0)
    g = c.engine(hip, lazy=True)                                    # the rounds may still be queued
    _check(g, c, 1, 1)
    g.close()


def test_load_ropes_index(hip):
    c = _case(2)
    g = hip.HipBwt(2)
    g.load_ropes([hip.hipbwt.encode_runs(r) for r in c.ropes])
    _check(g, c, 1, 1)
    _check(g, c, 5, 5)
    g.close()


def test_empty_index(hip):
    g = hip.HipBwt(0)
    qs = ["", "A", "ACGTN", "NNN", np.array([1, 0], np.uint8)]
    stored, mem, cnt = g.smem_raw(qs)
    assert stored == 0 and cnt.tolist() == [0, 0, 0, 0, -1] and (mem == 0).all()
    g.close()


def test_min_occ_zero_is_fatal():
    """a parameter below 1 is fatal with a message (reported through the fatal handler, which leaves by _exit)"""
    code = ("import sys, os, ctypes as C; sys.path.insert(0, %r)\n"
            "from ropebwt2_amd import HipBwt\n"
            "from ropebwt2_amd.hipbwt import load_hip_lib\n"
            "L = load_hip_lib()\n"
            "CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)\n"
            "def h(user, msg):\n"
            "    sys.stdout.write('fatal: ' + msg.decode()); sys.stdout.flush(); os._exit(7)\n"
            "cb = CB(h)\n"
            "L.rb2_hip_set_fatal_handler(cb, None)\n"
            "g = HipBwt(0)\n"
            "print(g.smem_raw(['ACGT'], 1, 1, 4)[2].tolist())\n"
            "g.smem_raw(['ACGT'], 1, 0, 4)\n"
            "print('NOT FATAL')\n") % ROOT
    p = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 7, (p.returncode, p.stdout.decode()[-400:], p.stderr.decode()[-400:])
    assert b"[0]" in p.stdout and b"fatal: [rb2_hip] smem" in p.stdout and b"min_occ" in p.stdout and b"NOT FATAL" not in p.stdout, p.stdout


def test_single_strand_index_terminates_in_bounds(hip):
    """without the reverse strands the results are unspecified, but the call returns and every record lies inside its query"""
    batches, strings = _batches(50, False)
    g = hip.HipBwt(0)
    for b in batches:
        g.insert_multi(b)
    qs = [q for q in _queries(strings, np.random.RandomState(2)) if not S.malformed(q)]
    for min_len, min_occ, max_mems in ((1, 1, 64), (3, 2, 2)):
        stored, mem, cnt = g.smem_raw(qs, min_len, min_occ, max_mems)
        for i, q in enumerate(qs):
            assert 0 <= cnt[i] <= len(q), (i, int(cnt[i]))
            r = mem[i, :min(int(cnt[i]), max_mems)]
            assert ((r[:, 0] >= 0) & (r[:, 0] <= r[:, 1]) & (r[:, 1] <= len(q))).all(), (i, r.tolist())
        assert stored == int(np.minimum(cnt, max_mems).sum())
    g.close()
