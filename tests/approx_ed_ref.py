"""References of the approximate search with insertions and deletions of include/rb2_hip.h (rb2_hip_approx_ed; kernel k_approx_ed in
csrc/rb2_edit.h), two that share nothing but the definition of a match:

  sub(a, c) = 0 if a == c and c is one of A C G T, else 1; lev = the unit-cost Levenshtein distance with sub as the cost of a column;
  ed(S, q) = sub(S[0], q[0]) + lev(S[1:-1], q[1:-1]) + sub(S[-1], q[-1]) for L >= 2 and |S| >= 2, sub(S[0], q[0]) for L == |S| == 1,
  infinite otherwise; a match is a word S over A C G T with ed(S, q) <= max_ed and at least min_occ occurrences

  brute(strings, q, ...)   every window of L - max_ed .. L + max_ed symbols of the strings that holds only A C G T, counted, with the full
                           dynamic programme of each distinct one; never looks at a BWT
  model(fm, q, ...)        the trie of words over query_ref.FM, from the last symbol, with the whole column lev(W', t[j:]) per node; its
                           only pruning is "some cell of the column <= max_ed - c0" (and min_occ)

A record is (lo, hi, ed, len).  Small indexes only.
"""
import numpy as np

from approx_ref import malformed, windows

INF = 1 << 20


def sub(a, c):
    return 0 if a == c and 1 <= c <= 4 else 1


def lev(X, Y):
    """unit-cost Levenshtein distance of the word X (A C G T) and the part Y of a query, a column costing sub; plain Python, the definition"""
    prev = list(range(len(Y) + 1))
    for i, x in enumerate(X):
        cur = [i + 1]
        for j, y in enumerate(Y):
            cur.append(min(prev[j + 1] + 1, cur[j] + 1, prev[j] + sub(int(x), int(y))))
        prev = cur
    return prev[len(Y)]


def ed(S, q):
    """the distance of the definition; INF when the ends cannot be aligned"""
    if len(q) >= 2 and len(S) >= 2:
        return sub(int(S[0]), int(q[0])) + lev(S[1:-1], q[1:-1]) + sub(int(S[-1]), int(q[-1]))
    if len(q) == 1 and len(S) == 1:
        return sub(int(S[0]), int(q[0]))
    return INF


def _lev_many(W, Y):
    """lev(w, Y) for every row w of W (n words of one length): the same recurrence, the rows of the table as vectors over the words"""
    n, m = W.shape[0], len(Y)
    Y = np.asarray(Y, np.int64)
    ok = (Y >= 1) & (Y <= 4)
    ar = np.arange(m + 1)
    prev = np.broadcast_to(ar, (n, m + 1)).copy()
    for i in range(W.shape[1]):
        x = W[:, i].astype(np.int64)
        tmp = np.empty((n, m + 1), np.int64)
        tmp[:, 0] = i + 1
        cost = 1 - ((x[:, None] == Y[None, :]) & ok[None, :])
        tmp[:, 1:] = np.minimum(prev[:, 1:] + 1, prev[:, :-1] + cost)
        prev = np.minimum.accumulate(tmp - ar, axis=1) + ar         # cur[j] = min over k <= j of tmp[k] + (j - k)
    return prev[:, m]


def brute(strings, q, max_ed, min_occ=1, fm=None, memo=None):
    """the matches of q among the windows of the strings: None for a malformed query, else a sorted list of (S as bytes, count, ed), or of
    the records (lo, hi, ed, len) when an FM model of the same strings is given.  memo: a dict that keeps the windows of a length"""
    q = np.asarray(q, dtype=np.uint8)
    if malformed(q):
        return None
    L = len(q)
    if L == 0:
        return []
    if memo is None:
        memo = {}
    out = []
    for n in ([1] if L == 1 else range(max(2, L - max_ed), L + max_ed + 1)):
        if n not in memo:
            memo[n] = windows(strings, n)
        cnt = memo[n]
        if not cnt:
            continue
        keys = list(cnt)
        W = np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), n)
        if L == 1:
            d = 1 - ((W[:, 0] == q[0]) & (q[0] <= 4))
        else:
            d = (1 - ((W[:, 0] == q[0]) & (q[0] <= 4))) + _lev_many(W[:, 1:-1], q[1:-1]) + (1 - ((W[:, -1] == q[-1]) & (q[-1] <= 4)))
        for k in np.flatnonzero(d <= max_ed):
            w, c = keys[k], cnt[keys[k]]
            if c < min_occ:
                continue
            if fm is None:
                out.append((w, c, int(d[k])))
            else:
                lo, hi, m = fm.backward_search(np.frombuffer(w, np.uint8))
                assert m == n and hi - lo == c, "the interval of a window is not as large as its count"
                out.append((int(lo), int(hi), int(d[k]), n))
    return sorted(out)


def model(fm, q, max_ed, min_occ=1):
    """the matches of q by a search over the trie of words of fm: None for a malformed query, else the sorted records (lo, hi, ed, len)"""
    q = np.asarray(q, dtype=np.uint8)
    if malformed(q):
        return None
    L = len(q)
    out = []
    if L == 0:
        return out
    C, occ = np.asarray(fm.C, np.int64), fm.occ
    kids = lambda lo, hi: [(int(C[a] + occ[lo, a]), int(C[a] + occ[hi, a])) for a in (1, 2, 3, 4)]
    if L == 1:
        return sorted((lo, hi, sub(a, int(q[0])), 1) for a, (lo, hi) in zip((1, 2, 3, 4), kids(0, fm.N)) if hi - lo >= min_occ and sub(a, int(q[0])) <= max_ed)
    t = q[1:-1].astype(np.int64)
    M = len(t)
    ar = np.arange(M + 1)
    tcost = [1 - ((t == a) & (t <= 4)) for a in (1, 2, 3, 4)]      # sub(a, t[j]) for the four a
    stack = []
    for z, (lo, hi) in zip((1, 2, 3, 4), kids(0, fm.N)):
        c0 = sub(z, int(q[-1]))
        if hi - lo >= min_occ and c0 <= max_ed:                      # (the column of the empty W' has the cell D[M] = 0)
            stack.append((lo, hi, c0, 0, (M - ar).astype(np.int64)))
    while stack:
        lo, hi, c0, d, D = stack.pop()                               # the node W'z, |W'| = d, D[j] = lev(W', t[j:])
        for a, (nlo, nhi) in zip((1, 2, 3, 4), kids(lo, hi)):
            if nhi - nlo < min_occ:
                continue
            e = c0 + int(D[0]) + sub(a, int(q[0]))                   # a as the first symbol
            if e <= max_ed:
                out.append((nlo, nhi, e, d + 2))
            tmp = D + 1                                              # a as one more inner symbol: ND[j] = min(D[j] + 1, D[j+1] + sub, ND[j+1] + 1)
            tmp[:M] = np.minimum(tmp[:M], D[1:] + tcost[a - 1])
            ND = (np.minimum.accumulate((tmp + ar)[::-1])[::-1]) - ar
            if int(ND.min()) <= max_ed - c0:
                stack.append((nlo, nhi, c0, d + 1, ND))
    return sorted(out)


def approx_ed_raw(fm, queries, max_ed, min_occ=1):
    """model() for every query: (the sorted records of each query, None for a malformed one; cnt as rb2_hip_approx_ed reports it, nothing cut)"""
    recs = [model(fm, q, max_ed, min_occ) for q in queries]
    return recs, np.array([-1 if r is None else len(r) for r in recs], np.int64)
