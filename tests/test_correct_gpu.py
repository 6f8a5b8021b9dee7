"""GPU tests of the read correction (include/rb2_hip.h: rb2_hip_correct[_dev], rb2_hip_correct_into; kernels in csrc/rb2_correct.h).
Everything is compared EXACTLY with the model (tests/correct_ref.py, which tests/test_correct_ref.py holds against brute force) on the
BWT read back from the same handle: the text, cnt, weak and the return value.  The indexes are those of test_approx_gpu.py (dense and
forced sparse, one strand and both, the loaded cov3000.fmd) and the coverage fixture of test_correct_ref.py; the reads are the smallest
ones at which the kernel can go wrong: control flow, the read's own stores read back, the solid bits of a row, the rows of a launch."""
import os
import subprocess
import sys

import numpy as np
import pytest

import correct_ref as CR
import fmd_ref
import helpers as H
import merge_ref as M
import query_ref as Q
from ropebwt2_amd.hipbwt import StepBudgetExceeded, pack_patterns
from test_approx_gpu import MALFORMED, _forced_sparse, _to_dev
from test_locate_gpu import _small
from test_query_gpu import _Env, _batches

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PROBES = 1 << 20                                                     # a budget none of these reads uses up
FILL = 0xEE


def _sub(rng, s, *at):
    """s with another symbol out of A C G T at every position of at"""
    t = s.copy()
    for p in at:
        t[p] = 1 + (int(t[p]) + int(rng.randint(3))) % 4 if t[p] < 5 else rng.randint(1, 5)
    return t


def read_set(strings, k, seed):
    """the reads of the module docstring from the clean strings of an index: (reads, the number of well-formed ones)"""
    rng = np.random.RandomState(seed)
    clean = [s for s in strings if len(s) >= 2 * k + 6 and not (s == 5).any()]
    assert len(clean) >= 8
    w0 = clean[0]
    qs = [np.zeros(0, np.uint8), w0[:1].copy(), w0[:k - 1].copy(), w0[:k].copy(), _sub(rng, w0[:k], k // 2), w0[:k + 1].copy(), _sub(rng, w0[:k + 1], 0),
          _sub(rng, w0[:k + 1], k)]                                   # L = 0, 1, k - 1, k (a single window, ja == jb), k + 1
    for i in range(6):
        w = clean[rng.randint(len(clean))]
        L = len(w)
        qs.append(w.copy())
        for p in (0, k - 2, k - 1, L - k, L - 1, L // 2):            # one error
            qs.append(_sub(rng, w, p))
        qs.append(_sub(rng, w, L // 2, L // 2 + 3))                  # two errors less than k apart, and two more than k apart
        qs.append(_sub(rng, w, 2, k + 4))
        for p in (0, L - 1, L // 2):                                 # an N at either end and in the middle
            t = w.copy(); t[p] = 5; qs.append(t)
        t = _sub(rng, w, 3); t[L - 4] = 5; qs.append(t)
    qs.append(np.full(20, 5, np.uint8))                              # all N
    qs.append(np.full(30, 1, np.uint8))                              # a homopolymer
    long = np.tile(clean[1], 8192 // len(clean[1]) + 1)[:8193].astype(np.uint8)   # copies of one string: every position lies in a window inside a copy
    qs.append(_sub(rng, long[:8192], 5000))
    n_well = len(qs)
    qs.append(long)                                                  # 8193 symbols: malformed
    return qs + [np.array(q, np.uint8) for q in MALFORMED], n_well


class _Ctx:
    """an index, its model, its strings by id, the reads, and the model's answers, computed once per parameter set"""
    def __init__(self, kind, g, k, min_occ):
        self.kind, self.g, self.k, self.min_occ = kind, g, k, min_occ
        self.fm = Q.FM(g.bwt())
        self.occ = CR.fm_counter(self.fm)
        self.strings = g.unpack()
        self.reads, self.n_well = read_set(self.strings, k, len(self.strings))
        self.memo = {}

    def want(self, k=None, min_occ=None, max_fix=8, max_probes=PROBES, reads=None):
        k, min_occ = k or self.k, min_occ or self.min_occ
        if reads is not None:
            return CR._many(CR.correct_one, self.occ, reads, k, min_occ, max_fix, max_probes)
        key = (k, min_occ, max_fix, max_probes)
        if key not in self.memo:
            self.memo[key] = CR._many(CR.correct_one, self.occ, self.reads, k, min_occ, max_fix, max_probes)
        return self.memo[key]


def _cov_handle(hip, reads, so=0):
    g = hip.HipBwt(so)
    g.insert_multi(H.encode_batch(reads, True, True))
    return g


@pytest.fixture(scope="module", params=["dense-both", "dense-one", "sparse-both", "sparse-one", "fmd", "cov"])
def idx(request, hip):
    kind = request.param
    k, min_occ = 12, 3
    if kind == "dense-both":
        g = _small(hip, 0)[0]
    elif kind == "dense-one":
        g = hip.HipBwt(0)
        for b in _batches(230, False)[0]:
            g.insert_multi(b)
        assert not g.layout_stats()["sparse_now"]
    elif kind.startswith("sparse"):
        g = _forced_sparse(hip, kind.endswith("both"))
    elif kind == "fmd":
        img, bwt = fmd_ref.fixture("cov3000")
        g = hip.HipBwt(0)
        assert g.load_fmd(np.frombuffer(img, np.uint8)) == len(bwt)
        min_occ = 2
    else:
        g = _cov_handle(hip, CR.coverage_fixture()[1])
        k = CR.COV_K
    g.build_ssa(3)
    cx = _Ctx(kind, g, k, min_occ)
    yield cx
    g.close()


def _check(cx, reads, got, want, what):
    fixes, out, off, cnt, weak = got
    texts, wcnt, wweak, _ = want
    assert np.array_equal(cnt, wcnt), (what, np.flatnonzero(cnt != wcnt)[:5].tolist(), cnt[cnt != wcnt][:5].tolist(), wcnt[cnt != wcnt][:5].tolist())
    assert np.array_equal(weak, wweak), (what, np.flatnonzero(weak != wweak)[:5].tolist(), weak[weak != wweak][:5].tolist(), wweak[weak != wweak][:5].tolist())
    for i, t in enumerate(texts):
        assert np.array_equal(out[off[i]:off[i + 1]], t), (what, i, reads[i][:50].tolist(), np.flatnonzero(out[off[i]:off[i + 1]] != t)[:5].tolist())
    assert fixes == CR.total_fixes(wcnt), what


def test_parity_with_the_model(idx):
    """the whole set, none skipped; what the set must exercise is asserted on the model's answers; the index is what it was"""
    cx, g = idx, idx.g
    want = cx.want()
    texts, cnt, weak, probes = want
    assert cnt[cx.n_well:].tolist() == [-1] * (len(MALFORMED) + 1) and cnt[:3].tolist() == [0, 0, 0] and weak[:3].tolist() == [0, 1, cx.k - 1]
    assert (cnt[:cx.n_well] >= 0).all() and (cnt == 1).sum() >= 6 and (cnt == 2).sum() >= 2 and cnt[cx.n_well - 1] >= 1
    print("%s: %d reads, %d fixes, %d probes (the most %d), %d reads left weak" % (cx.kind, len(cx.reads), CR.total_fixes(cnt), probes.sum(), probes.max(), (weak > 0).sum()))
    hashes, lay, ssa = g.rope_hashes(), g.layout_stats(), g.ssa_info()
    _check(cx, cx.reads, g.correct_raw(cx.reads, cx.k, cx.min_occ, 8, PROBES), want, cx.kind)
    assert g.rope_hashes() == hashes and g.layout_stats() == lay and g.ssa_info() == ssa and ssa["valid"], "a correction changed the index"
    for n in (1, 15, 16, 17):                                        # rows of a block, a last partial block
        qs = cx.reads[8:8 + n]
        _check(cx, qs, g.correct_raw(qs, cx.k, cx.min_occ, 8, PROBES), tuple(w[8:8 + n] for w in want), (cx.kind, n))


@pytest.mark.parametrize("k,min_occ,max_fix", [(1, 3, 8), (1, 0, 8), (2, 3, 8), (5, 2, 8), (0, 1, 8), (0, 0, 1)], ids=["k1", "k1-rare", "k2", "k5", "occ1", "fix1"])
def test_parameters(idx, k, min_occ, max_fix):
    """k = 1 (with min_occ = 3, and one above the count of the rarest of A C G T, which makes that symbol weak everywhere), small k,
    min_occ = 1, and max_fix = 1 on reads with two errors (0 stands for the index's own k and min_occ)"""
    cx, g = idx, idx.g
    if k == 1 and min_occ == 0:
        min_occ = int(min(cx.fm.occ[cx.fm.N, 1:5])) + 1
    k, min_occ = k or cx.k, min_occ or cx.min_occ
    keep = np.array([len(q) < 8000 for q in cx.reads])               # (the reads of 8192 symbols once, in the parity test: the model is slow on them at small k)
    reads = [q for q in cx.reads if len(q) < 8000]
    want = cx.want(k, min_occ, max_fix, reads=reads)
    _check(cx, reads, g.correct_raw(reads, k, min_occ, max_fix, PROBES), want, (cx.kind, k, min_occ, max_fix))
    if max_fix == 1:
        two = cx.want()[1][keep] == 2
        assert two.sum() >= 2 and (want[1][two] == 1).all() and (want[2][two] > 0).any()


def test_budgets(idx):
    """max_probes at, just below and just above the model's probe count of a read, and at the number of its clean windows - 1, + 0, + 1"""
    cx, g = idx, idx.g
    texts, cnt, weak, probes = cx.want()
    m = cx.n_well - 1                                                # (without the read of 8192 symbols)
    pick = [int(i) for i in np.flatnonzero(cnt[:m] >= 1)[:4]] + [int(i) for i in np.flatnonzero((weak[:m] > 0) & (probes[:m] > 0))[:2]]
    assert len(pick) >= 5
    over = done = 0
    for i in pick:
        q = cx.reads[i]
        clean = sum(all(1 <= c <= 4 for c in q[j:j + cx.k]) for j in range(len(q) - cx.k + 1))
        for mp in sorted({clean - 1, clean, clean + 1, int(probes[i]) - 1, int(probes[i]), int(probes[i]) + 1} - {0, -1}):
            want = cx.want(max_probes=mp, reads=[q])
            _check(cx, [q], g.correct_raw([q], cx.k, cx.min_occ, 8, mp), want, (cx.kind, i, mp))
            assert (want[1][0] <= -2) == (mp < probes[i])
            over += want[1][0] <= -2
            done += want[1][0] >= 0
            if mp < clean:
                assert want[1][0] == -2 and np.array_equal(want[0][0], q)
    assert over >= 2 * len(pick) and done >= 2 * len(pick)
    i = pick[0]
    with pytest.raises(StepBudgetExceeded) as e:
        g.correct([cx.reads[i], cx.reads[0]], cx.k, cx.min_occ, max_probes=int(probes[i]) - 1)
    want = cx.want(max_probes=int(probes[i]) - 1, reads=[cx.reads[i], cx.reads[0]])
    assert e.value.queries == [0] and np.array_equal(e.value.results[0][0], want[0][0]) and e.value.results[1].tolist() == want[1].tolist()
    res = g.correct([cx.reads[i]], cx.k, cx.min_occ)                 # the default budget is enough for a read of this set
    assert np.array_equal(res[0][0], texts[i]) and res[1].tolist() == [cnt[i]] and res[2].tolist() == [weak[i]]


def test_rows_and_chunks(idx):
    """four rows per launch with many more reads than rows; RB2_QUERY_CHUNK = 3"""
    cx, g = idx, idx.g
    want = cx.want()
    with _Env(RB2_CORRECT_ROWS=4):
        _check(cx, cx.reads, g.correct_raw(cx.reads, cx.k, cx.min_occ, 8, PROBES), want, (cx.kind, "4 rows"))
    with _Env(RB2_QUERY_CHUNK=3):
        _check(cx, cx.reads, g.correct_raw(cx.reads, cx.k, cx.min_occ, 8, PROBES), want, (cx.kind, "chunks of 3"))
    with _Env(RB2_QUERY_CHUNK=3, RB2_CORRECT_ROWS=2):
        _check(cx, cx.reads, g.correct_raw(cx.reads, cx.k, cx.min_occ, 8, PROBES), want, (cx.kind, "chunks of 3, 2 rows"))


@pytest.mark.parametrize("inplace", [True, False], ids=["out-is-qry", "out-apart"])
def test_device_variant(idx, inplace):
    """correct_dev with the reads between junk: off[0] = 37, a fill behind the data, in cnt and weak too, all of which must survive"""
    cx, g = idx, idx.g
    texts, wcnt, wweak, _ = cx.want()
    qry, off = pack_patterns(cx.reads)
    n, total = len(off) - 1, int(off[-1])
    buf = np.concatenate([np.full(37, FILL, np.uint8), qry[:total], np.full(64, FILL, np.uint8)])
    off = off + 37
    out = np.full(len(buf), FILL, np.uint8)
    cnt, weak = np.full(n + 2, -7, np.int64), np.full(n + 2, -7, np.int64)
    ptrs = _to_dev(g, (buf, off, out, cnt, weak))
    try:
        d_out = ptrs[0] if inplace else ptrs[2]
        with _Env(RB2_CORRECT_ROWS=16 if inplace else 1 << 20):
            g.correct_dev(n, ptrs[0], ptrs[1], total, d_out, ptrs[3], ptrs[4], cx.k, cx.min_occ, 8, PROBES)
        g.sync()
        got = np.zeros(len(buf), np.uint8)
        for d, a in ((d_out, got), (ptrs[3], cnt), (ptrs[4], weak), (ptrs[0], buf)):
            g.L.rb2_hip_memcpy(g.h, a.ctypes.data, d, a.nbytes, 1)
    finally:
        for d in ptrs:
            g.dev_free(d)
    assert (got[:37] == FILL).all() and (got[37 + total:] == FILL).all() and (cnt[n:] == -7).all() and (weak[n:] == -7).all()
    assert np.array_equal(cnt[:n], wcnt) and np.array_equal(weak[:n], wweak)
    assert np.array_equal(got[37:37 + total], np.concatenate(texts))
    if not inplace:
        assert np.array_equal(buf[37:37 + total], qry[:total]), "the reads were changed"


def test_empty_calls(hip):
    g = hip.HipBwt(0)
    assert g.correct([], 5)[0] == []
    fixes, out, off, cnt, weak = g.correct_raw([[1, 2, 3], [], [5], [0]], 2, 1)      # an empty index: nothing is solid, nothing can be fixed
    assert fixes == 0 and cnt.tolist() == [0, 0, 0, -1] and weak.tolist() == [3, 0, 1, -1] and out[:5].tolist() == [1, 2, 3, 5, 0]
    assert g.L.rb2_hip_correct(g.h, 0, None, None, 0, 0, 0, 0, None, None, None) == 0         # n = 0 returns before the parameters are checked
    g.L.rb2_hip_correct_dev(g.h, 0, None, None, -1, 0, 0, 0, 0, None, None, None)
    d = hip.HipBwt(0)
    assert g.correct_into(d, 3)["symbols"] == 0 and d.counts().sum() == 0
    g.close(); d.close()


# ---- correct_into ---------------------------------------------------------------------------------------------------------------------

def _into_reads(long):
    """a small coverage set (200 reads of 30 symbols, half of them damaged), an empty read, one shorter than k, one with an N, and, when
    asked for, one of 8200 symbols, which is malformed and copied as it is"""
    reads = CR.coverage_fixture(seed=11, G=200, L=30, cov=30, k=11)[1]
    rng = np.random.RandomState(4)
    n = reads[5].copy(); n[9] = 5
    return reads[:100] + [np.zeros(0, np.uint8), reads[3][:6].copy(), n] + reads[100:] + ([rng.randint(1, 5, size=8200).astype(np.uint8)] if long else [])


@pytest.mark.parametrize("so,pairs", [(0, True), (0, False), (1, False), (2, False)], ids=["io-pairs", "io", "rlo", "rclo"])
def test_correct_into(hip, so, pairs):
    """with RB2_MERGE_BATCH small enough for many batches (whole pairs when asked) and with the default: dst's BWT is the oracle's of dst's
    strings followed by the model's corrected strings, info is the model's, src is what it was"""
    long = so == 0                                                   # (a string of 8200 symbols is 8200 rounds of every insert: in one order only)
    src, k = _cov_handle(hip, _into_reads(long), so), 11
    base = H.encode_batch(M.mixed_reads(30, 7))
    try:
        src.build_ssa(2)
        strings = src.unpack()
        fm = Q.FM(src.bwt())
        hashes, ssa = src.rope_hashes(), src.ssa_info()
        if pairs:
            assert all(np.array_equal(strings[i + 1], Q.revcomp(strings[i])) for i in range(0, len(strings), 2))
        want_bwt = {}
        for budget in (150, 0):
            texts, winfo, added = CR.correct_into(strings, k, 3, pairs=pairs, fm=fm, budget=budget or 1 << 62)
            key = b"".join(t.tobytes() + b"\0" for t in texts)
            if key not in want_bwt:
                want_bwt[key] = M.oracle_bwt(so, [base, H.encode_batch(texts)])
            # (a floor, not the figure: 100 of the 200 reads carry a substitution, and the model's info is what is compared exactly below)
            assert winfo[1] >= 40 and winfo[2] >= winfo[1] and winfo[5] == (0 if not long else 1 if pairs else 2) and (winfo[6] > 50 if budget else winfo[6] == 1)
            dst = hip.HipBwt(so)
            dst.insert_multi(base)
            dst.build_ssa(2)
            with _Env(**({"RB2_MERGE_BATCH": budget} if budget else {})):
                info = src.correct_into(dst, k, 3, pairs=pairs)
            assert [info[f] for f in hip.HipBwt.CORRECT_INFO] == winfo.tolist() and info["symbols"] == added, (info, winfo.tolist())
            assert np.array_equal(dst.bwt(), want_bwt[key]), (so, pairs, budget)
            assert not dst.ssa_info()["valid"]
            dst.close()
        assert len(want_bwt) == 1                                    # (the batches do not change what is inserted)
        assert src.rope_hashes() == hashes and src.ssa_info() == ssa and ssa["valid"]
        if not long:                                                 # batch_bytes as an argument cuts like the environment does; an empty dst
            dst = hip.HipBwt(so)
            info = src.correct_into(dst, k, 3, pairs=pairs, batch_bytes=150)
            assert info["batches"] == CR.correct_into(strings, k, 3, pairs=pairs, fm=fm, budget=150)[1][6] > 50
            assert np.array_equal(dst.bwt(), M.oracle_bwt(so, [H.encode_batch(texts)]))
            dst.close()
    finally:
        src.close()


def test_corrected_then_assembled(hip):
    """the coverage fixture corrected on the device is the index of the error-free reads, byte for byte (the model restores every read:
    test_correct_ref.py), and so are its unitigs"""
    truth, reads, pos = CR.coverage_fixture()
    src, ref = _cov_handle(hip, reads), _cov_handle(hip, truth)
    try:
        for pairs in (True, False):
            g, info = src.corrected(CR.COV_K, CR.COV_MIN_OCC, pairs=pairs)
            assert info["strings"] == 1200 and info["changed"] == info["fixes"] == (300 if pairs else 600) and info["weak"] == info["over_budget"] == info["malformed"] == 0
            assert g.so == src.so and g.rope_hashes() == ref.rope_hashes() and np.array_equal(g.bwt(), ref.bwt())
            if pairs:
                g.build_ssa(2); ref.build_ssa(2)
                a, ia = g.assemble(20)
                b, ib = ref.assemble(20)
                assert ia.tolist() == ib.tolist() and len(a) == len(b) >= 1
                assert [(t.tobytes(), p.tolist(), c) for t, p, c in a] == [(t.tobytes(), p.tolist(), c) for t, p, c in b]
            g.close()
    finally:
        src.close(); ref.close()


@pytest.mark.parametrize("case,what", [("k0", "correct: k must"), ("minocc0", "correct: min_occ must"), ("maxfix0", "correct: max_fix must"), ("maxprobes0", "correct: max_probes must"),
                                       ("dev_k0", "correct_dev: k must"), ("dev_total", "correct_dev: total must"), ("rank", "correct: this handle holds only"),
                                       ("into_k0", "correct_into: k must"), ("into_maxprobes0", "correct_into: max_probes must"), ("dst_is_src", "correct_into: dst and src must be two different"),
                                       ("negative_batch", "correct_into: batch_bytes must not be negative"), ("rank_dst", "correct_into: dst holds only"),
                                       ("rank_src", "correct_into: src holds only"), ("odd_pairs", "correct_into: pairs needs")])
def test_fatal_cases(hip, case, what):
    """each leaves through the fatal handler with a message of its own, and dst and src are what they were"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "correct_fatal_child.py"), case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 7 and "the call returned" not in out, (p.returncode, out, p.stderr.decode()[-1500:])
    assert "handler: [rb2_hip] " + what in out and "unchanged ok" in out, out
