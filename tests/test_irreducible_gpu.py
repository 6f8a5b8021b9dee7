"""GPU tests of the irreducible-overlap query (include/rb2_hip.h: rb2_hip_irreducible[_dev]; kernel k_irreducible in csrc/rb2_query.h): the
record sets and counts the device reports must equal the model on the BWT of the same index (tests/irreducible_ref.py, which
tests/test_irreducible_ref.py holds against brute force), and through HipBwt.irreducible and HipBwt.edges the brute force over string
slices itself.  What can go wrong is addressing -- the twin interval, the stacks in device memory, the record slots, the rows of a launch
-- not volume: on the small indexes every string is a query; on layouts D and S (900 000 and more symbols, strings of 100 to 1500) the
Python model is the limit, so the queries there are a sample of the strings and made-up ones that do have neighbours, and the step budget
is small enough for the model -- most of those queries end over budget, where the count and the records found by then must agree too."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import irreducible_ref as IR
import query_ref as Q
from ropebwt2_amd.hipbwt import StepBudgetExceeded, pack_patterns
from test_locate_ref import string_sets
from test_overlap_ref import queries as made_up
from test_query_layouts_gpu import _Models, _build_dense, _build_sparse

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILL = -7                                                            # what the device variant must leave in the slots it does not write
MALFORMED = [[1, 0], [0], [1, 0, 2], [7, 1], [3, 6], [1] * 8193]
PARAMS = [(1, 4), (3, 1000), (8, 1)]                                 # (min_ovlp, max_ext)
STEPS = 1 << 16                                                      # a budget no query of the small indexes uses up
BIG_STEPS = 1500                                                     # layouts D and S: what the model can follow


@pytest.fixture(scope="module")
def models():
    ms = _Models()
    yield ms
    ms.made.clear()


def small_index(hip, name, so):
    """a set of test_locate_ref.string_sets() in a fresh handle, in two batches"""
    reads, rev = string_sets()[name]
    g = hip.HipBwt(so)
    half = len(reads) // 2
    for part in (reads[:half], reads[half:]):
        g.insert_multi(H.encode_batch(part, True, rev))
    return g, Q.FM(g.bwt())


class _Ctx:
    """an index, its model, its strings by id (read back with extract), the queries, and the model's answers, computed once per
    (min_ovlp, max_ext, max_steps)"""
    def __init__(self, kind, g, fm, big):
        self.kind, self.g, self.fm, self.big = kind, g, fm, big
        self.n = n = int(fm.C[1])
        self.strings = [np.asarray(s, np.uint8) for s in g.extract(np.arange(n), 2048)]
        rng = np.random.RandomState(n)
        if big:
            clean = [s for s in self.strings if len(s) >= 50 and not (s == 5).any()]
            pick = [clean[k] for k in rng.choice(len(clean), size=12, replace=False)]
            qs = [s.copy() for s in pick[:6]]
            for k, s in enumerate(pick):                            # a neighbour that ends 1 .. 4 symbols behind the query: a record within max_ext = 4
                qs.append(np.concatenate([rng.randint(1, 5, size=5).astype(np.uint8), s[:len(s) - 1 - k % 4]]))
            qs += [np.array(q, np.uint8) for q in ([5], [1, 5], [])]
        else:
            plain, more = made_up(self.strings, rng)
            qs = [s for s in self.strings if len(s)] + more
        self.n_well = len(qs)
        self.queries = qs + [np.array(q, np.uint8) for q in MALFORMED]
        self.maxlen = max(len(q) for q in self.queries[:self.n_well])
        self.memo = {}

    def steps(self, max_ext):
        """the budget of a call: on layouts D and S a long extension is cut short for the model's sake"""
        return BIG_STEPS if self.big and max_ext >= 1000 else STEPS

    def want(self, min_ovlp, max_ext, max_steps=None):
        """([records as a list in the model's order, None for a malformed query], cnt) of all queries"""
        key = (min_ovlp, max_ext, max_steps or self.steps(max_ext))
        if key not in self.memo:
            res = [IR.irreducible(self.fm, q, min_ovlp, max_ext, key[2]) for q in self.queries]
            self.memo[key] = ([None if c == -1 else r for r, c, _ in res], np.array([c for _, c, _ in res], np.int64))
        return self.memo[key]


@pytest.fixture(scope="module", params=["dense-io", "dense-rclo", "D", "S", "tiny-io", "one-strand"])
def idx(request, hip, models):
    """repetitive-both in input order and in RCLO; layout D (every piece longer than two superblocks) and layout S (sparse, split leaves)
    of test_query_layouts_gpu.py; tiny-both; the repetitive set on one strand, where the records are whatever the arithmetic gives"""
    kind = request.param
    if kind == "D":
        ix = _build_dense(hip, models.get(0))
        g, fm = ix.g, ix.m.fm
    elif kind == "S":
        ix = _build_sparse(hip, models.get("S"))
        g, fm = ix.g, ix.m.fm
    else:
        name, so = {"dense-io": ("repetitive-both", 0), "dense-rclo": ("repetitive-both", 2), "tiny-io": ("tiny-both", 0), "one-strand": ("repetitive", 0)}[kind]
        g, fm = small_index(hip, name, so)
    cx = _Ctx(kind, g, fm, kind in "DS")
    yield cx
    g.close()


def _have(cnt, max_recs):
    return np.minimum(np.where(cnt <= -2, -2 - cnt, np.maximum(cnt, 0)), max_recs)


def _sets(rec, cnt, max_recs):
    """the records stored for every query as sorted lists of tuples (None for a malformed query)"""
    return [None if c == -1 else sorted(map(tuple, r[:k].tolist())) for r, k, c in zip(rec, _have(cnt, max_recs), cnt)]


def _to_dev(g, arrays):
    ptrs = [g.dev_alloc(max(a.nbytes, 8)) for a in arrays]
    for d, a in zip(ptrs, arrays):
        if a.nbytes:
            g.L.rb2_hip_memcpy(g.h, d, a.ctypes.data, a.nbytes, 0)
    return ptrs


def irreducible_dev(g, queries, max_len, min_ovlp, max_ext, max_steps, max_recs):
    """irreducible_dev on buffers filled with FILL, two records of room behind rec and two counts behind cnt, which must stay
    as they were: (rec, cnt) as the device left them"""
    qry, off = pack_patterns(queries)
    n = len(off) - 1
    rec = np.full((n * max_recs + 2, 4), FILL, np.int64)
    cnt = np.full(n + 2, FILL, np.int64)
    ptrs = _to_dev(g, (qry, off, rec, cnt))
    try:
        g.irreducible_dev(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], max_len, min_ovlp, max_ext, max_steps, max_recs)
        for d, a in zip(ptrs[2:], (rec, cnt)):
            g.L.rb2_hip_memcpy(g.h, a.ctypes.data, d, a.nbytes, 1)
    finally:
        for d in ptrs:
            g.dev_free(d)
    assert (rec[n * max_recs:] == FILL).all() and (cnt[n:] == FILL).all(), "something was written behind rec or cnt"
    return rec[:n * max_recs].reshape(n, max_recs, 4), cnt[:n]


def _check(cx, got, want, max_recs, what, fill=0):
    """stored, rec, cnt against the model's (records, cnt) with nothing cut; the slots behind the records hold fill"""
    stored, rec, cnt = got
    recs, wcnt = want
    assert np.array_equal(cnt, wcnt), (what, np.flatnonzero(cnt != wcnt)[:5].tolist(), cnt[cnt != wcnt][:5].tolist(), wcnt[cnt != wcnt][:5].tolist())
    have = _have(cnt, max_recs)
    assert have.max(initial=0) <= max_recs and (stored is None or stored == have.sum())
    for i, (a, b) in enumerate(zip(_sets(rec, cnt, max_recs), recs)):
        assert a == (None if b is None else sorted(b)), (what, i, cx.queries[i].tolist()[:40], a[:4] if a else a, b[:4] if b else b)
    assert (rec[~(np.arange(max_recs)[None, :] < have[:, None])] == fill).all(), what


@pytest.mark.parametrize("min_ovlp,max_ext", PARAMS)
def test_parity_with_the_model(idx, min_ovlp, max_ext):
    """every query of the set: the same records as sets and the same counts from the host variant and from the _dev variant, which leaves
    FILL where it stores nothing and writes nothing behind rec; the index stays as it was"""
    cx, g = idx, idx.g
    recs, wcnt = cx.want(min_ovlp, max_ext)
    found = np.where(wcnt <= -2, -2 - wcnt, np.maximum(wcnt, 0))
    max_recs = max(int(found.max()), 1)
    print("%s min_ovlp=%d max_ext=%d: %d queries, %d records, the most %d, %d over budget" % (cx.kind, min_ovlp, max_ext, len(cx.queries), found.sum(), max_recs, (wcnt <= -2).sum()))
    assert wcnt[cx.n_well:].tolist() == [-1] * len(MALFORMED) and (wcnt[:cx.n_well] != -1).all()
    steps = cx.steps(max_ext)
    if cx.big:
        assert (wcnt >= 0).sum() >= 3 and (wcnt <= -2).any() == (max_ext == 1000)
        assert max_ext != 4 or found.sum() >= 12                    # the made-up queries find their neighbours
    else:
        assert (wcnt >= -1).all() and (found.sum() > 0 or min_ovlp == 8 or cx.kind == "one-strand")
    before = g.layout_stats()
    _check(cx, g.irreducible_raw(cx.queries, min_ovlp, max_ext, steps, max_recs), (recs, wcnt), max_recs, (cx.kind, min_ovlp, max_ext))
    assert g.layout_stats() == before, "the query changed the layout"
    rec, cnt = irreducible_dev(g, cx.queries, min(max(cx.maxlen, 1), 8192), min_ovlp, max_ext, steps, max_recs)
    _check(cx, (None, rec, cnt), (recs, wcnt), max_recs, (cx.kind, min_ovlp, max_ext, "dev"), FILL)
    # a max_len below the longest query: that query is malformed for the _dev variant, the others are as they were
    short = cx.maxlen - 1
    if short >= 1:
        rec, cnt = irreducible_dev(g, cx.queries, short, min_ovlp, max_ext, steps, max_recs)
        lens = np.array([len(q) for q in cx.queries])
        assert (cnt[lens > short] == -1).all() and np.array_equal(cnt[lens <= short], wcnt[lens <= short])


@pytest.mark.parametrize("max_recs", [1, 2])
def test_truncated_records(idx, max_recs):
    """with fewer slots than records exactly max_recs distinct true records are stored and cnt is the whole number"""
    cx, g = idx, idx.g
    recs, wcnt = cx.want(1, 4)
    stored, rec, cnt = g.irreducible_raw(cx.queries, 1, 4, STEPS, max_recs)
    assert np.array_equal(cnt, wcnt) and stored == _have(cnt, max_recs).sum()
    cut = 0
    for i, have in enumerate(_sets(rec, cnt, max_recs)):
        if have is not None:
            assert len(set(have)) == len(have) == min(len(recs[i]), max_recs) and set(have) <= set(recs[i]), (cx.kind, i)
            assert (rec[i, len(have):] == 0).all()
            cut += len(recs[i]) > max_recs
    assert cut > 0 or not cx.kind.startswith("dense") or max_recs == 2, cx.kind
    qs = cx.queries[:40]
    rec, cnt = irreducible_dev(g, qs, min(max(cx.maxlen, 1), 8192), 1, 4, STEPS, max_recs)
    for i, have in enumerate(_sets(rec, cnt, max_recs)):
        if have is not None:
            assert len(set(have)) == len(have) == min(len(recs[i]), max_recs) and set(have) <= set(recs[i]) and (rec[i, len(have):] == FILL).all()


@pytest.mark.parametrize("max_steps", [1, 7, 40])
def test_step_budget(idx, max_steps):
    """cnt equals the model's at the same budget -- the steps are counted alike and the search runs in the same order --, and what is
    stored are records of the full answer"""
    cx, g = idx, idx.g
    full = None if cx.big else cx.want(2, 6, 1 << 40)[0]           # (D and S: the model at the same budget alone)
    recs, wcnt = cx.want(2, 6, max_steps)
    stored, rec, cnt = g.irreducible_raw(cx.queries, 2, 6, max_steps, 8)
    assert np.array_equal(cnt, wcnt), (cx.kind, np.flatnonzero(cnt != wcnt)[:5].tolist())
    assert ((cnt <= -2).any() or (cx.kind == "tiny-io" and max_steps == 40)) and stored == _have(cnt, 8).sum()
    for i, have in enumerate(_sets(rec, cnt, 8)):
        if have is not None:
            assert len(set(have)) == len(have) == min(len(recs[i]), 8) and set(have) <= set(recs[i]) and (full is None or set(recs[i]) <= set(full[i])), (cx.kind, i)
    assert max_steps < 40 or cx.big or any(c <= -3 for c in cnt.tolist()) or cx.kind == "tiny-io"   # out of steps with records in hand
    if max_steps == 7:
        over = np.flatnonzero(cnt <= -2).tolist()
        g.build_ssa(3)                                              # (the Python layer resolves the ranges: no query minds the array)
        with pytest.raises(StepBudgetExceeded) as e:
            g.irreducible(cx.queries, 2, 6, max_steps=7, max_recs=8)
        assert e.value.queries == over and len(e.value.results) == len(cx.queries)


def _brute(strings, q, min_ovlp, max_ext):
    b = IR.brute_irreducible(strings, q, min_ovlp, max_ext)
    return None if b is None else sorted(b)


@pytest.mark.parametrize("name", ["repetitive-both", "tiny-both"])
def test_python_layer_against_brute_force(hip, name):
    """HipBwt.irreducible(pairs=True) and HipBwt.edges(pairs=True) on the dense indexes in input order: the neighbours themselves, as the
    brute force over the strings names them; without pairs the ids are those of the reverse complements"""
    g, fm = small_index(hip, name, 0)
    n = int(fm.C[1])
    strings = [np.asarray(s, np.uint8) for s in g.extract(np.arange(n), 64)]
    assert all(np.array_equal(strings[k + 1], Q.revcomp(strings[k])) for k in range(0, n, 2))
    g.build_ssa(2)
    qs = strings + [np.array(q, np.uint8) for q in MALFORMED]
    edges = 0
    for min_ovlp, max_ext in PARAMS + [(2, None)]:
        me = max_ext or max(len(q) for q in qs if len(q) <= 8192)
        want = [_brute(strings, q, min_ovlp, me) for q in qs]
        got = g.irreducible(qs, min_ovlp, max_ext, max_recs=64, max_hits=64, pairs=True)
        assert got == want, (name, min_ovlp, max_ext, next(i for i in range(len(qs)) if got[i] != want[i]))
        twins = g.irreducible(qs, min_ovlp, max_ext, max_recs=64, max_hits=64)
        assert twins == [None if w is None else sorted((s ^ 1, l, e) for s, l, e in w) for w in want]
        rows = sorted((i, d, l, e) for i, w in enumerate(want[:n]) for d, l, e in w)
        ed = g.edges(min_ovlp=min_ovlp, max_ext=me, max_recs=64, max_hits=64, pairs=True)
        assert ed.dtype == np.int64 and ed.shape == (len(rows), 4) and ed.tolist() == [list(r) for r in rows]
        edges += len(rows)
    print(name, edges, "edges")
    assert edges > (300 if name == "repetitive-both" else 5)
    some = [3, 0, 17]
    ed = g.edges(some, min_ovlp=1, max_ext=4, max_recs=64, max_hits=64, pairs=True)
    assert ed.tolist() == sorted([i, d, l, e] for i in some for d, l, e in _brute(strings, strings[i], 1, 4))
    assert g.edges([], min_ovlp=1).shape == (0, 4) and g.irreducible([], 1) == []
    txt = "".join("$ACGTN"[c] for c in strings[4])
    assert g.irreducible([txt], 1, 4, max_recs=64, max_hits=64, pairs=True) == [_brute(strings, strings[4], 1, 4)]
    g.close()
    g = hip.HipBwt(1)                                               # another sorting order, an odd number of strings: no pairs
    g.insert_multi(H.encode_batch(string_sets()[name][0], True, True))
    g.build_ssa(2)
    with pytest.raises(ValueError):
        g.irreducible(qs[:3], 1, 4, pairs=True)
    g.close()
    g = hip.HipBwt(0)
    g.insert_multi(H.encode_batch(string_sets()[name][0][:3], True, False))
    g.build_ssa(2)
    with pytest.raises(ValueError):
        g.edges(min_ovlp=1, pairs=True)
    g.close()


def test_chain(hip):
    """reads of 20 symbols at every second position of a genome of 80, both strands: each overlaps five reads behind it at min_ovlp = 10
    and has one edge, to its successor; a suffix array built before stays valid, and an insert behind the call is seen by the next"""
    reads = IR.chain_reads(IR.CHAIN_SEED)
    g = hip.HipBwt(0)
    assert g.irreducible_raw([[1, 2], []], 1, 4)[2].tolist() == [0, 0]           # an empty index
    g.insert_multi(H.encode_batch(reads, True, True))
    g.build_ssa(1)
    inf, hashes = g.ssa_info(), g.rope_hashes()
    n = 2 * len(reads)
    want = sorted([2 * i, 2 * i + 2, 18, 2] for i in range(len(reads) - 1)) + sorted([2 * i + 1, 2 * i - 1, 18, 2] for i in range(1, len(reads)))
    ed = g.edges(min_ovlp=10, pairs=True)
    assert ed.tolist() == sorted(want) and len(ed) == n - 2
    assert g.ssa_info() == inf and inf["valid"] and g.rope_hashes() == hashes
    ov = g.overlaps(reads[:-5], 10)
    assert all(len([1 for s, l in o if l < 20]) == 5 for o in ov)                # five overlaps, one edge
    strings = Q.inserted_strings(reads, True, True)
    assert g.irreducible(reads, 10, pairs=True) == [_brute(strings, r, 10, 20) for r in reads]
    g.set_lazy(1)
    short = reads[2][:17]                                           # genome[4:21]: it leaves the first read by one symbol, and the second read lies behind it
    g.insert_multi(H.encode_batch([short], True, True))             # (lazy: the rounds may still be queued when the query begins)
    strings += Q.inserted_strings([short], True, True)
    g.build_ssa(1)
    got = g.irreducible(reads[:2], 8, pairs=True)
    assert got == [_brute(strings, r, 8, 20) for r in reads[:2]] and got[0] == [(n, 16, 1)]
    g.close()


def _child(stage):
    p = subprocess.run([sys.executable, os.path.join(HERE, "irreducible_child.py"), stage], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p.returncode, p.stdout.decode(), p.stderr.decode()[-1500:]


def test_chunks_and_rows(hip):
    """RB2_QUERY_CHUNK=7 and RB2_IRRED_SCRATCH of two rows' worth, in a process of their own: the same answers"""
    rc, out, err = _child("chunk")
    assert rc == 0 and "STAGE OK" in out, (rc, out, err)


@pytest.mark.parametrize("stage,what", [("ovlp0", "min_ovlp"), ("ext0", "max_ext"), ("ext8193", "max_ext"), ("steps0", "max_steps"), ("recs0", "max_recs"),
                                        ("dev-len0", "max_len"), ("dev-len8193", "max_len"), ("dev-ext0", "max_ext"), ("dev-recs0", "max_recs"),
                                        ("shard", "sharded index")])
def test_fatal_parameters(hip, stage, what):
    """each leaves through the fatal handler with the function's name and the parameter in the message; n = 0 with bad parameters returns"""
    rc, out, err = _child(stage)
    assert rc == 7 and "NOT FATAL" not in out, (rc, out, err)
    assert "irreducible ok" in out and "empty ok" in out and "handler: [rb2_hip] irreducible" in out and what in out, out
