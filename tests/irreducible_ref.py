"""References of the irreducible-overlap query of include/rb2_hip.h (rb2_hip_irreducible; kernel k_irreducible in csrc/rb2_query.h; DESIGN.md
section 19), two that share nothing but the definition:

  A candidate of the query q (L symbols) is (T, l, X): T a string of the index, min_ovlp <= l < L, T[:l] == q[L-l:] with no N in it (the
  search stops at the first N from the end), X = T[l:] with 1 <= |X| <= max_ext over A C G T only.  A candidate is reducible when another
  candidate (U, l', X') has X' a proper prefix of X, or X' == X and l' > l.  One record (l, |X|, zlo, zhi) per distinct (l, X) of the
  others; [zlo, zhi) are the `$` ranks (rb2_hip_string_ids) of the strings revcomp(T).

  brute_irreducible(strings, q, ...)  slices of the strings only; never looks at a BWT
  irreducible(fm, q, ...)             the arithmetic of the kernel over query_ref.FM, step for step and in its order

and the composition the fused call replaces (edges_by_composition: overlaps, then the text of every neighbour, then the pruning on the host).
Small indexes only.
"""
import numpy as np

from overlap_ref import head

MAX_LEN = 8192                                                       # a longer query is malformed


def malformed(q):
    q = np.asarray(q, dtype=np.int64)
    return len(q) > MAX_LEN or bool(((q < 1) | (q > 5)).any())


def irreducible(fm, q, min_ovlp, max_ext, max_steps=1 << 62):
    """(records, cnt, steps) of one query: records = [(l, ext, zlo, zhi), ...] in the order the depth-first search finds them, cnt as
    rb2_hip_irreducible reports it (-1 malformed, <= -2 out of steps with -2 - cnt records found), steps = the rank pairs taken"""
    q = np.asarray(q, dtype=np.uint8).reshape(-1)
    if malformed(q):
        return [], -1, 0
    L, N, C, occ = len(q), fm.N, fm.C, fm.occ
    recs, steps = [], 0
    if L == 0:
        return recs, 0, 0
    rank = lambda x: occ[min(max(int(x), 0), N)]                     # (an index of one strand: the twin interval may leave the index)
    # 1. the backward search of q from its end, carrying the twin interval: every suffix some string begins with becomes an entry
    root = []
    c0 = int(q[L - 1])
    if c0 < 5:
        x0, x1, size, m = int(C[c0]), int(C[5 - c0]), int(occ[N, c0]), 1
        while size > 0:
            if steps >= max_steps:
                return recs, -2, steps
            steps += 1
            cl, ch = rank(x0), rank(x0 + size)
            nd = int(ch[0] - cl[0])
            if min_ovlp <= m < L and nd > 0:
                root.append((m, x1, x1 + nd))                       # the interval of revcomp(q[L-m:]) followed by `$`
            if m == L:
                break
            c = int(q[L - 1 - m])
            if c == 5:
                break
            x1 += nd + sum(int(ch[b] - cl[b]) for b in range(c + 1, 5))   # the other end in the complement order $ T G C A N
            x0, size, m = int(C[c] + cl[c]), int(ch[c] - cl[c]), m + 1
    # 2. depth first over the extensions; a node is (d, entries), its children are made when it is visited
    stack = [(0, root)]
    while stack:
        d, ents = stack.pop()
        kids = [[], [], [], []]
        best = None
        for l, lo, hi in ents:
            if steps >= max_steps:
                return recs, -2 - len(recs), steps
            steps += 1
            cl, ch = rank(lo), rank(hi)
            if ch[0] > cl[0] and (best is None or l > best[0]):
                best = (l, d, int(cl[0]), int(ch[0]))
            for a in (1, 2, 3, 4):
                nlo, nhi = int(C[a] + cl[a]), int(C[a] + ch[a])
                if nlo < nhi:
                    kids[a - 1].append((l, nlo, nhi))
        if d >= 1 and best is not None:
            recs.append(best)
            continue
        if d < max_ext:
            for a in (4, 3, 2, 1):                                  # (a stack: child 1 is visited first)
                if kids[a - 1]:
                    stack.append((d + 1, kids[a - 1]))
    return recs, len(recs), steps


def irreducible_raw(fm, queries, min_ovlp, max_ext, max_steps=1 << 16, max_recs=16):
    """(stored, rec (n, max_recs, 4), cnt (n,)) in the shape of HipBwt.irreducible_raw: the first min(found, max_recs) records in the
    model's order (the device's order is unspecified: compare as sets), zeros behind them"""
    n = len(queries)
    rec = np.zeros((n, max_recs, 4), np.int64)
    cnt = np.zeros(n, np.int64)
    stored = 0
    for i, q in enumerate(queries):
        r, cnt[i], _ = irreducible(fm, q, min_ovlp, max_ext, max_steps)
        r = r[:max_recs]
        rec[i, :len(r)] = np.array(r, np.int64).reshape(-1, 4)
        stored += len(r)
    return stored, rec, cnt


def edges_of(fm, recs):
    """the records of one query resolved through head[]: the set of (id of revcomp(T), l, ext)"""
    hd = head(fm)
    return {(int(s), l, e) for l, e, zlo, zhi in recs for s in hd[zlo:zhi]}


def _candidates(strings, q, min_ovlp, max_ext):
    q = np.asarray(q, dtype=np.uint8).reshape(-1)
    L = len(q)
    out = []
    for l in range(max(int(min_ovlp), 1), L):
        suf = q[L - l:]
        if (suf == 5).any():
            break
        for k, s in enumerate(strings):
            s = np.asarray(s, np.uint8)
            X = s[l:]
            if len(s) > l and len(X) <= max_ext and np.array_equal(s[:l], suf) and ((X >= 1) & (X <= 4)).all():
                out.append((k, l, X.tobytes()))
    return out


def _prune(cand):
    """the (k, l, |X|) of the candidates (k, l, X) that no other candidate makes reducible"""
    return {(k, l, len(X)) for k, l, X in cand
            if not any((len(X2) < len(X) and X[:len(X2)] == X2) or (X2 == X and l2 > l) for _, l2, X2 in cand)}


def brute_irreducible(strings, q, min_ovlp, max_ext):
    """the set of (k, l, ext): string k is an irreducible neighbour of q by the definition at the top; None for a malformed query"""
    return None if malformed(q) else _prune(_candidates(strings, q, min_ovlp, max_ext))


def edges_by_composition(texts, ovl, max_ext):
    """the host pruning the fused call replaces.  ovl: the (string id, l) pairs of one query as the overlaps of its proper suffixes give
    them (l below the length of the query), texts[id] = that string; the set of (id, l, ext) that survive"""
    cand = []
    for k, l in ovl:
        X = np.asarray(texts[k], np.uint8)[l:]
        if 1 <= len(X) <= max_ext and ((X >= 1) & (X <= 4)).all():
            cand.append((k, l, X.tobytes()))
    return _prune(cand)


def chain_reads(seed, glen=80, rlen=20, stride=2):
    """reads of rlen symbols at every stride-th position of a random genome of glen symbols"""
    g = np.random.RandomState(seed).randint(1, 5, size=glen).astype(np.uint8)
    return [g[p:p + rlen].copy() for p in range(0, glen - rlen + 1, stride)]


CHAIN_SEED = 1                                                       # (test_irreducible_ref.py asserts that this seed gives the plain chain)
