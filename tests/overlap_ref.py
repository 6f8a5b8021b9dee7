"""numpy reference of the suffix-prefix overlap queries of the device index (include/rb2_hip.h: rb2_hip_overlap, rb2_hip_string_ids) over
query_ref.FM.

A row of the interval [lo, hi) of a non-empty pattern P whose BWT symbol is `$` is the row of a whole string that starts with P, so the
strings with the prefix P are head[q] for q in [occ($, lo), occ($, hi)), head[q] = the string behind the q-th `$` of the BWT.  Small
indexes only.
"""
import numpy as np

from locate_ref import suffix_array


def head(fm):
    """head[q] = the string (row of the `$` block) whose whole-string row holds the q-th `$` of the BWT"""
    if getattr(fm, "_head", None) is None:
        fm._head = suffix_array(fm)[0][fm.bwt == 0]
    return fm._head


def malformed(q):
    q = np.asarray(q, dtype=np.int64)
    return bool(((q < 1) | (q > 5)).any())


def overlap(fm, q, min_ovlp, max_recs=1 << 40):
    """(records, cnt) of one query by the definition, every suffix searched on its own: records (min(cnt, max_recs), 3) = l, zlo, zhi in
    increasing l; cnt = -1 (and no records) for a malformed query"""
    q = np.asarray(q, dtype=np.uint8).reshape(-1)
    if malformed(q):
        return np.zeros((0, 3), np.int64), -1
    recs = []
    for l in range(max(min_ovlp, 1), len(q) + 1):
        suf = q[len(q) - l:]
        if (suf == 5).any():                                        # an N belongs to no overlap, nor does anything that reaches across it
            break
        lo, hi, m = fm.backward_search(suf)
        if m != l:
            continue
        zlo, zhi = int(fm.occ[lo, 0]), int(fm.occ[hi, 0])
        if zhi > zlo:
            recs.append((l, zlo, zhi))
    return np.array(recs[:max_recs], np.int64).reshape(-1, 3), len(recs)


def overlap_raw(fm, queries, min_ovlp, max_recs):
    """(stored, rec (n, max_recs, 3), cnt (n,)) as HipBwt.overlap_raw returns them: zeros beyond min(cnt, max_recs).  All queries search
    in step, one symbol per turn, the way the kernel does: one pair of ranks gives the record of this length and the next interval"""
    qs = [np.asarray(q, dtype=np.int64).reshape(-1) for q in queries]
    n = len(qs)
    rec = np.zeros((n, max_recs, 3), np.int64)
    cnt = np.zeros(n, np.int64)
    lens = np.array([len(q) for q in qs], np.int64)
    bad = np.array([malformed(q) for q in qs], bool)
    cnt[bad] = -1
    R = np.full((n, int(lens.max()) + 1 if n else 1), 5, np.int64)  # the queries from their last symbol, an N behind each: it stops the search
    for i, q in enumerate(qs):
        if not bad[i]:
            R[i, :len(q)] = q[::-1]
    act = np.flatnonzero(R[:, 0] < 5)
    c = R[act, 0]
    lo, hi, m = fm.C[c], fm.C[c] + fm.occ[fm.N, c], 1
    while True:
        keep = lo < hi
        act, lo, hi = act[keep], lo[keep], hi[keep]
        if len(act) == 0:
            break
        zlo, zhi = fm.occ[lo, 0], fm.occ[hi, 0]
        if m >= min_ovlp:
            r = zhi > zlo
            who, k = act[r], cnt[act[r]]
            st = k < max_recs
            rec[who[st], k[st]] = np.stack([np.full(int(st.sum()), m), zlo[r][st], zhi[r][st]], 1)
            cnt[who] += 1
        c = R[act, m]
        go = c < 5
        act, lo, hi, c = act[go], lo[go], hi[go], c[go]
        lo, hi, m = fm.C[c] + fm.occ[lo, c], fm.C[c] + fm.occ[hi, c], m + 1
    return int(np.minimum(np.maximum(cnt, 0), max_recs).sum()), rec, cnt


def string_ids(fm, zlo, zhi, max_hits):
    """(ids, cnt) exactly as rb2_hip_string_ids answers one range: ids = head[zlo .. zlo + min(cnt, max_hits)); cnt = zhi - zlo, or -1
    (and no ids) for zlo < 0, zhi > the number of strings or zlo > zhi"""
    if zlo < 0 or zhi > int(fm.C[1]) or zlo > zhi:
        return np.zeros(0, np.int64), -1
    return head(fm)[zlo:zlo + min(zhi - zlo, max_hits)].astype(np.int64), zhi - zlo


def string_ids_raw(fm, ranges, max_hits):
    """(stored, ids (n, max_hits), cnt (n,)) as HipBwt.string_ids_raw returns them: zeros beyond min(cnt, max_hits)"""
    zv = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    ids = np.zeros((len(zv), max_hits), np.int64)
    cnt = np.zeros(len(zv), np.int64)
    for i, (zlo, zhi) in enumerate(zv.tolist()):
        h, cnt[i] = string_ids(fm, zlo, zhi, max_hits)
        ids[i, :len(h)] = h
    return int(np.minimum(np.maximum(cnt, 0), max_hits).sum()), ids, cnt


def overlaps(fm, q, min_ovlp):
    """the set of (string id, l) the model finds for one well-formed query"""
    hd = head(fm)
    recs, cnt = overlap(fm, q, min_ovlp)
    assert cnt == len(recs)
    return {(int(s), l) for l, zlo, zhi in recs.tolist() for s in hd[zlo:zhi]}


def brute_overlaps(strings, q, min_ovlp):
    """the set of (k, l): string k begins with the last l symbols of q, min_ovlp <= l <= len(q), no N among them.  Slices of the strings
    are compared; the BWT is never looked at"""
    q = np.asarray(q, dtype=np.uint8).reshape(-1)
    out = set()
    for l in range(max(min_ovlp, 1), len(q) + 1):
        suf = q[len(q) - l:]
        if (suf == 5).any():
            break
        for k, s in enumerate(strings):
            if len(s) >= l and np.array_equal(np.asarray(s, np.uint8)[:l], suf):
                out.add((k, l))
    return out
