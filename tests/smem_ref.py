"""numpy reference of rb2_hip_smem (include/rb2_hip.h): the super-maximal exact matches of a query, straight from the definition.

For every start s the longest match q[s:e(s)) with at least min_occ occurrences is found by counting q[s:e) with
query_ref.FM.backward_search for growing e; [s, e(s)) is an SMEM when e(s) > s, no earlier start reaches as far (s == 0 or
e(s-1) < e(s)) and it is at least min_len long.  Quadratic in the query length and deliberately not the kernel's algorithm (which walks
one bi-interval backward and forward from the end of the previous SMEM).  The index must hold both strands of every string.

smems() asks backward_search for every pair (s, e) it looks at; for hundreds of queries occ_table() gets the same counts for all pairs of
a query from one backward walk per end e (the intervals a backward search of q[0:e) passes through are those of q[s:e), s = e-1 .. 0),
and smems_from_table() reads the SMEMs of any (min_len, min_occ) off that table.  tests/test_smem_ref.py holds the two against each other.
"""
import numpy as np

import query_ref as Q


def malformed(q):
    q = np.asarray(q, dtype=np.int64)
    return bool(((q < 1) | (q > 5)).any())


def occ(fm, q, s, e):
    """occurrences of q[s:e) (s < e); 0 when it holds an N"""
    p = np.asarray(q[s:e], dtype=np.uint8)
    if (p == 5).any():
        return 0
    lo, hi, m = fm.backward_search(p)
    return hi - lo if m == len(p) else 0


def ends(fm, q, min_occ):
    """e(s) for every s: the largest e with occ(s, e) >= min_occ, s if there is none (occ falls as e grows, so the first miss ends it)"""
    L = len(q)
    out = []
    for s in range(L):
        e = s
        while e < L and occ(fm, q, s, e + 1) >= min_occ:
            e += 1
        out.append(e)
    return out


def smems(fm, q, min_len=1, min_occ=1):
    """(k, 5) int64 array of start, end, x0, x1, size in increasing start; None for a malformed query"""
    q = np.asarray(q, dtype=np.uint8).reshape(-1)
    if malformed(q):
        return None
    es = ends(fm, q, min_occ)
    out = []
    for s, e in enumerate(es):
        if e > s and (s == 0 or es[s - 1] < e) and e - s >= min_len:
            lo, hi, m = fm.backward_search(q[s:e])
            rlo = fm.backward_search(Q.revcomp(q[s:e]))[0]
            out.append([s, e, lo, rlo, hi - lo])
    return np.array(out, np.int64).reshape(-1, 5)


def occ_table(fm, q):
    """tab[s, e] = occ(s, e) for all 0 <= s < e <= L ((L + 1) x (L + 1), zero elsewhere)"""
    q = np.asarray(q, dtype=np.uint8).reshape(-1)
    L = len(q)
    tab = np.zeros((L + 1, L + 1), np.int64)
    C = fm.C.tolist()
    for e in range(1, L + 1):
        lo, hi = 0, fm.N
        for s in range(e - 1, -1, -1):
            c = int(q[s])
            if c == 5:
                break
            lo, hi = C[c] + int(fm.occ[lo, c]), C[c] + int(fm.occ[hi, c])
            if lo >= hi:
                break
            tab[s, e] = hi - lo
    return tab


def smems_from_table(fm, q, tab, min_len=1, min_occ=1):
    """smems() with the counts taken from tab = occ_table(fm, q)"""
    q = np.asarray(q, dtype=np.uint8).reshape(-1)
    es = []
    for s in range(len(q)):
        ok = np.flatnonzero(tab[s, s + 1:] >= min_occ)
        es.append(s + 1 + int(ok[-1]) if len(ok) else s)
    out = []
    for s, e in enumerate(es):
        if e > s and (s == 0 or es[s - 1] < e) and e - s >= min_len:
            lo, hi, m = fm.backward_search(q[s:e])
            out.append([s, e, lo, fm.backward_search(Q.revcomp(q[s:e]))[0], hi - lo])
    return np.array(out, np.int64).reshape(-1, 5)
