"""References of the approximate search of include/rb2_hip.h (rb2_hip_approx; kernel k_approx in csrc/rb2_query.h), two that share nothing
but the definition of a match -- a word S over A C G T as long as the query, at most max_mm positions where S differs from it (an N of the
query always differs), at least min_occ occurrences -- and take the interval of a match from query_ref.FM.backward_search:

  brute(strings, q, ...)   every window of the indexed strings that holds only A C G T, counted; never looks at a BWT
  model(fm, q, ...)        backtracking over an FM-index with no bound at all: every child with min_occ rows is followed

and a plain statement of the piece bound D (csrc/rb2_query_plan.h: approx_bound).  Small indexes only.
"""
from collections import Counter

import numpy as np

MAX_LEN = 8192                                                       # a longer query is malformed


def pack_subs(subs):
    """[(pos, sym), ...] -> the subs word of a record: 16 bits each as pos << 3 | sym, in decreasing pos, the first in bits 0..15"""
    v = 0
    for k, (p, c) in enumerate(sorted(subs, reverse=True)):
        assert 0 <= p < MAX_LEN and 1 <= c <= 4 and k < 4
        v |= (p << 3 | c) << (16 * k)
    return v


def unpack_subs(v):
    out = []
    while v & 0xFFFF:
        out.append(((v & 0xFFFF) >> 3, v & 7))
        v >>= 16
    return out


def malformed(q):
    q = np.asarray(q, dtype=np.int64)
    return len(q) > MAX_LEN or bool(((q < 1) | (q > 5)).any())


def _record(fm, q, S):
    """the record of the match S of q: (lo, hi, n_mm, subs)"""
    lo, hi, m = fm.backward_search(np.array(S, np.uint8))
    assert m == len(S)
    subs = [(p, int(S[p])) for p in range(len(q)) if S[p] != q[p]]
    return int(lo), int(hi), len(subs), pack_subs(subs)


def windows(strings, L):
    """Counter of the windows of L symbols of the strings that hold only A C G T, as bytes"""
    cnt = Counter()
    for s in strings:
        s = np.asarray(s, dtype=np.uint8)
        if len(s) < L:
            continue
        w = np.lib.stride_tricks.sliding_window_view(s, L)
        w = w[((w >= 1) & (w <= 4)).all(1)]
        cnt.update(map(bytes, w))
    return cnt


def brute(strings, q, max_mm, min_occ=1, fm=None, memo=None):
    """the matches of q among the windows of the strings: None for a malformed query, else a sorted list of (S as bytes, count), or of the
    records (lo, hi, n_mm, subs) when an FM model of the same strings is given.  memo: a dict that keeps the windows of a length"""
    q = np.asarray(q, dtype=np.uint8)
    if malformed(q):
        return None
    L = len(q)
    if L == 0:
        return []
    if memo is None:
        memo = {}
    if L not in memo:
        memo[L] = windows(strings, L)
    out = []
    for w, c in memo[L].items():
        S = np.frombuffer(w, np.uint8)
        if c < min_occ or int((S != q).sum()) > max_mm:
            continue
        if fm is None:
            out.append((w, c))
        else:
            r = _record(fm, q, S)
            assert r[1] - r[0] == c, "the interval of a window is not as large as its count"
            out.append(r)
    return sorted(out)


def model(fm, q, max_mm, min_occ=1):
    """the matches of q by backtracking over fm: None for a malformed query, else the sorted records (lo, hi, n_mm, subs)"""
    q = np.asarray(q, dtype=np.uint8)
    if malformed(q):
        return None
    L = len(q)
    out = []
    if L == 0:
        return out
    stack = [(L - 1, 0, fm.N, 0, ())]
    while stack:
        p, lo, hi, m, subs = stack.pop()
        for a in (1, 2, 3, 4):
            cost = int(a != q[p])
            if m + cost > max_mm:
                continue
            nlo, nhi = int(fm.C[a] + fm.occ[lo, a]), int(fm.C[a] + fm.occ[hi, a])
            if nhi - nlo < min_occ:
                continue
            ns = subs + ((p, a),) if cost else subs
            if p == 0:
                out.append((nlo, nhi, m + cost, pack_subs(ns)))
            else:
                stack.append((p - 1, nlo, nhi, m + cost, ns))
    return sorted(out)


def bound(count, q, min_occ=1):
    """D[p], p < len(q): the pieces that lie wholly in [0, p].  count(w) = occurrences of the word w.  From the last symbol: the longest
    q[s .. e] is extended to the left while it has min_occ occurrences; the first q[s .. e] that has fewer is a piece, and the search goes
    on at e = s - 1; an N is a piece by itself (the symbols behind it that still matched are none)"""
    q = [int(c) for c in q]
    L = len(q)
    pieces = []
    e = L - 1
    j = L - 1
    while j >= 0:
        if q[j] == 5:
            pieces.append((j, j)); e = j - 1
        elif count(q[j:e + 1]) < min_occ:
            pieces.append((j, e)); e = j - 1
        j -= 1
    return [sum(1 for s, t in pieces if t <= p) for p in range(L)], pieces


def approx_raw(fm, queries, max_mm, min_occ=1):
    """model() for every query: (the sorted records of each query, None for a malformed one; cnt as rb2_hip_approx reports it, nothing cut)"""
    recs = [model(fm, q, max_mm, min_occ) for q in queries]
    return recs, np.array([-1 if r is None else len(r) for r in recs], np.int64)
