"""Model of rb2_hip_correct[_dev] and rb2_hip_correct_into (include/rb2_hip.h, "correcting reads by the k-mer spectrum"): the rule over
any function that counts a word, with the probe count the header fixes, so that budget cases compare exactly.

occ(w) = the occurrences of the word w in the indexed strings: query_ref.FM.count over a BWT (correct_raw), or a table of the windows
of the strings themselves, which never looks at a BWT (window_counts).  brute_one restates the rule naively -- every window counted
again after every fix, the weak set recomputed from all of them -- and counts only what the header says a probe is."""
import collections

import numpy as np

import query_ref as Q

MAX_LEN = 8192


def _acgt(c):
    return 1 <= c <= 4


def malformed(q):
    q = np.asarray(q)
    return len(q) > MAX_LEN or bool(((q < 1) | (q > 5)).any())


def fm_counter(fm):
    """occ(w) by backward search on the model index, memoised"""
    memo = {}

    def occ(w):
        key = bytes(bytearray(w))
        if key not in memo:
            memo[key] = fm.count(np.array(w, np.uint8)) if len(w) else fm.N
        return memo[key]
    return occ


def window_counts(strings, k):
    """occ(w) for words of k symbols by a table of every window of the strings (no BWT)"""
    tab = collections.Counter()
    for s in strings:
        b = bytes(bytearray(np.asarray(s, np.uint8)))
        for i in range(len(b) - k + 1):
            tab[b[i:i + k]] += 1
    return lambda w: tab.get(bytes(bytearray(w)), 0)


class _Over(Exception):
    pass


def correct_one(occ, q, k, min_occ, max_fix, max_probes, where=None):
    """(text, cnt, weak, probes) of one well-formed read, incrementally as the rule is stated; where (a list) is told in which part a
    read ran out of probes: profile, alternatives or re-evaluation"""
    where = [] if where is None else where
    q = [int(c) for c in q]
    L = len(q)
    if L < k:
        return np.array(q, np.uint8), 0, L, 0
    nw = L - k + 1
    solid = [False] * nw
    st = {"probes": 0, "part": "profile"}

    def probe(w):
        if st["probes"] >= max_probes:
            where.append(st["part"])
            raise _Over()
        st["probes"] += 1
        return occ(w) >= min_occ

    def evaluate(j0, j1):
        for j in range(j0, j1 + 1):
            w = q[j:j + k]
            solid[j] = all(_acgt(c) for c in w) and probe(w)

    def weak_positions():
        return [p for p in range(L) if not any(solid[j] for j in range(max(0, p - k + 1), min(p, L - k) + 1))]

    fixes = 0
    try:
        evaluate(0, nw - 1)
        while fixes < max_fix:
            fixed = False
            for p in weak_positions():
                ja = p - k + 1 if p >= k - 1 else 0
                jb = p if p + k <= L else L - k
                for j in ([ja] if ja == jb else [ja, jb]):
                    if not all(_acgt(q[x]) for x in range(j, j + k) if x != p):
                        continue
                    good = []
                    st["part"] = "alternatives"
                    for b in (1, 2, 3, 4):
                        if b != q[p] and probe(q[j:p] + [b] + q[p + 1:j + k]):
                            good.append(b)
                    if len(good) == 1:
                        q[p] = good[0]
                        fixes += 1
                        fixed = True
                        st["part"] = "re-evaluation"
                        evaluate(max(0, p - k + 1), min(p, L - k))
                        break
                if fixed:
                    break
            if not fixed:
                break
    except _Over:
        return np.array(q, np.uint8), -2 - fixes, -1, st["probes"]
    return np.array(q, np.uint8), fixes, len(weak_positions()), st["probes"]


def brute_one(occ, q, k, min_occ, max_fix, max_probes):
    """the same four values with a full recomputation after every fix: all windows are counted again (that costs nothing here), and the
    probes are only counted -- the clean windows of the profile, three or four per tried window, the clean windows around a fix"""
    q = [int(c) for c in q]
    L = len(q)
    if L < k:
        return np.array(q, np.uint8), 0, L, 0
    wins = range(L - k + 1)
    clean = lambda j: all(_acgt(c) for c in q[j:j + k])
    weak = lambda: [p for p in range(L) if not any(clean(j) and occ(q[j:j + k]) >= min_occ for j in wins if j <= p < j + k)]
    probes, fixes = sum(clean(j) for j in wins), 0
    if probes > max_probes:
        return np.array(q, np.uint8), -2, -1, max_probes
    while fixes < max_fix:
        fixed = False
        for p in weak():
            tried = []
            for j in (max(p - k + 1, 0), min(p, L - k)):
                if j in tried or any(not _acgt(q[x]) for x in range(j, j + k) if x != p):
                    continue
                tried.append(j)
                alts = [b for b in (1, 2, 3, 4) if b != q[p]]
                if probes + len(alts) > max_probes:
                    return np.array(q, np.uint8), -2 - fixes, -1, max_probes
                probes += len(alts)
                good = [b for b in alts if occ(q[j:p] + [b] + q[p + 1:j + k]) >= min_occ]
                if len(good) == 1:
                    q[p] = good[0]
                    fixes += 1
                    fixed = True
                    probes += sum(clean(w) for w in wins if w <= p < w + k)
                    if probes > max_probes:
                        return np.array(q, np.uint8), -2 - fixes, -1, max_probes
                    break
            if fixed:
                break
        if not fixed:
            break
    return np.array(q, np.uint8), fixes, len(weak()), probes


def _many(one, occ, reads, k, min_occ, max_fix, max_probes):
    texts, cnt, weak, probes = [], [], [], []
    for r in reads:
        r = np.asarray(r, np.uint8).reshape(-1)
        t, c, w, p = (r.copy(), -1, -1, 0) if malformed(r) else one(occ, r, k, min_occ, max_fix, max_probes)
        texts.append(t); cnt.append(c); weak.append(w); probes.append(p)
    return texts, np.array(cnt, np.int64), np.array(weak, np.int64), np.array(probes, np.int64)


def correct_raw(fm, reads, k, min_occ=3, max_fix=8, max_probes=1 << 20):
    """rb2_hip_correct on the index of fm: (texts, cnt, weak, probes); probes is what the model counted, the device does not report it"""
    return _many(correct_one, fm_counter(fm), reads, k, min_occ, max_fix, max_probes)


def brute_raw(strings, reads, k, min_occ=3, max_fix=8, max_probes=1 << 20):
    """the same from the windows of the strings, by the naive restatement"""
    return _many(brute_one, window_counts(strings, k), reads, k, min_occ, max_fix, max_probes)


def total_fixes(cnt):
    cnt = np.asarray(cnt, np.int64)
    return int(np.where(cnt <= -2, -2 - cnt, np.maximum(cnt, 0)).sum())


def batches(lens, budget, pairs):
    """how rb2_hip_correct_into cuts strings of these lengths (sentinel included) into batches: the most strings within the budget, one at
    the least; with pairs a batch holds whole pairs (one string less, or the pair when it alone is too long): [(i0, i1), ...]"""
    out, i0, n = [], 0, len(lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    while i0 < n:
        e = i0 + 1
        while e < n and off[e + 1] - off[i0] <= budget:
            e += 1
        if pairs and (e - i0) % 2:
            e = e + 1 if e - i0 == 1 else e - 1
        out.append((i0, e))
        i0 = e
    return out


def correct_into(strings, k, min_occ=3, max_fix=8, max_probes=1 << 20, pairs=False, fm=None, budget=1 << 62):
    """rb2_hip_correct_into: (the strings appended to dst, in order; info (8,) int64; the symbols added, sentinels included).  The counts
    are those of fm's index when one is given, of the strings' own windows otherwise"""
    strings = [np.asarray(s, np.uint8) for s in strings]
    occ = fm_counter(fm) if fm is not None else window_counts(strings, k)
    assert not pairs or len(strings) % 2 == 0
    todo = strings[::2] if pairs else strings
    texts, cnt, weak, _ = _many(correct_one, occ, todo, k, min_occ, max_fix, max_probes)
    out = [t for c in texts for t in (c, Q.revcomp(c))] if pairs else texts
    changed = sum(not np.array_equal(a, b) for a, b in zip(todo, texts))
    cuts = batches([len(s) + 1 for s in strings], budget, pairs)
    size = lambda a, b: sum(len(s) + 1 for s in strings[a:b])
    info = np.array([len(strings), changed, total_fixes(cnt), int((weak > 0).sum()), int((cnt <= -2).sum()), int((cnt == -1).sum()),
                     len(cuts), max((size(a, b) for a, b in cuts), default=0)], np.int64)
    return out, info, sum(len(s) + 1 for s in strings)


# ---- the coverage fixture of tests/test_correct_ref.py and tests/test_correct_gpu.py ---------------------------------------------------
COV_SEED, COV_K, COV_MIN_OCC, COV_LEN = 7, 15, 3, 40


def coverage_fixture(seed=COV_SEED, G=600, L=COV_LEN, cov=40, k=COV_K):
    """reads of L symbols at cov x from both strands of one random circular genome of G symbols (circular, so that no read lies at a thin
    end), half of them with one substitution -- the first thirty of those at position 0, L - 1 and k - 1 in turn, the others anywhere.
    Returns (truth, reads, pos): the error-free reads, the reads as sequenced, the damaged position of each (-1: none)"""
    rng = np.random.RandomState(seed)
    genome = rng.randint(1, 5, size=G).astype(np.uint8)
    n = G * cov // L
    truth = []
    for a, rev in zip(rng.randint(G, size=n), rng.randint(2, size=n)):
        r = genome[(a + np.arange(L)) % G]
        truth.append(Q.revcomp(r) if rev else r.copy())
    pos = np.full(n, -1, np.int64)
    reads = [r.copy() for r in truth]
    for i, x in enumerate(rng.permutation(n)[:n // 2]):
        p = (0, L - 1, k - 1)[i % 3] if i < 30 else int(rng.randint(L))
        reads[x][p] = 1 + (int(reads[x][p]) + int(rng.randint(3))) % 4
        pos[x] = p
    return truth, reads, pos
