"""numpy reference of the suffix array of the device index (include/rb2_hip.h: rb2_hip_ssa_build, rb2_hip_locate) over query_ref.FM.

String k is row k of the `$` block.  Its walk starts at row k and takes LF steps until the BWT symbol is `$`; the row after j steps is
the suffix of string k that starts j symbols before its end, so SA(row) = (k, len[k] - j): the string and the 0-based position in text
order where the row's suffix starts ((k, len[k]), the place of the sentinel, for the rows of the `$` block).  Small indexes only.
"""
import numpy as np


def suffix_array(fm):
    """(sid[N], pos[N], lens[n]) by the walk definition, all strings walking in step; every row is visited exactly once"""
    if getattr(fm, "_sa", None) is not None:
        return fm._sa
    n, N = int(fm.C[1]), fm.N
    sid = np.full(N, -1, np.int64)
    step = np.zeros(N, np.int64)
    lens = np.zeros(n, np.int64)
    x = np.arange(n, dtype=np.int64)
    who = np.arange(n, dtype=np.int64)
    j = 0
    while len(x):
        assert (sid[x] == -1).all() and len(np.unique(x)) == len(x), "a row lies on two walks"
        sid[x], step[x] = who, j
        c = fm.bwt[x].astype(np.int64)
        done = c == 0
        lens[who[done]] = j
        x, who, c = x[~done], who[~done], c[~done]
        x = fm.C[c] + fm.occ[x, c]
        j += 1
    assert (sid >= 0).all(), "a row lies on no walk"
    pos = lens[sid] - step if N else np.zeros(0, np.int64)
    fm._sa = (sid, pos, lens)
    return fm._sa


def locate(fm, lo, hi, max_hits):
    """(hits, cnt) exactly as rb2_hip_locate answers one interval: hits (min(cnt, max_hits), 2) = string id, position of the rows
    lo, lo + 1, ..; cnt = hi - lo, or -1 (and no hits) for lo < 0, hi > N or lo > hi"""
    if lo < 0 or hi > fm.N or lo > hi:
        return np.zeros((0, 2), np.int64), -1
    sid, pos, _ = suffix_array(fm)
    m = min(hi - lo, max_hits)
    return np.stack([sid[lo:lo + m], pos[lo:lo + m]], 1).astype(np.int64), hi - lo


def locate_raw(fm, intervals, max_hits):
    """(stored, hit (n, max_hits, 2), cnt (n,)) as HipBwt.locate_raw returns them: zeros beyond min(cnt, max_hits)"""
    iv = np.asarray(intervals, dtype=np.int64).reshape(-1, 2)
    hit = np.zeros((len(iv), max_hits, 2), np.int64)
    cnt = np.zeros(len(iv), np.int64)
    for i, (lo, hi) in enumerate(iv.tolist()):
        h, cnt[i] = locate(fm, lo, hi, max_hits)
        hit[i, :len(h)] = h
    return int(np.minimum(np.maximum(cnt, 0), max_hits).sum()), hit, cnt


def brute_places(strings, pat):
    """the set of (k, i): pat (text order; a trailing 0 = the string end) starts at position i of string k + its sentinel.  Slices of
    the strings are compared; the BWT is never looked at (query_ref.brute_count returning the places instead of their number)"""
    pat = np.asarray(pat, dtype=np.uint8)
    L = len(pat)
    out = set()
    for k, s in enumerate(strings):
        t = np.concatenate([np.asarray(s, np.uint8), [0]]).astype(np.uint8)
        if L == 0:                                                  # the empty pattern starts at every symbol, the sentinel included
            out.update((k, i) for i in range(len(t)))
            continue
        for i in range(len(t) - L + 1):
            if t[i] == pat[0] and np.array_equal(t[i:i + L], pat):
                out.add((k, i))
    return out
