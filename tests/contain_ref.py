"""numpy model of rb2_hip_contained (include/rb2_hip.h) over query_ref.FM, and a brute force over string slices
that never looks at a BWT.

The model is the walk of the header, all strings in step as FM.walk_all does: row = k, [lo, hi) = [0, N), ahi = C[1]; a step reads the
symbol c of the row, stops at `$` and otherwise moves row, lo, hi and ahi to C[c] + occ(c, .).  Records are flag, occ, n_equal, rank,
walked."""
import numpy as np

import helpers as H
import query_ref as Q


def contained(fm, ids=None, early=True, check=None, info=None):
    """the (n, 5) records of the strings ids (None: all of them); check(row, lo, ahi, hi), if given, is called with the state of the
    strings still walking after every step; info, a dict, gets "early" = the walks the early exit ended (some of them in front of
    their `$`, with all their symbols read)"""
    N, n = fm.N, int(fm.C[1])
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64).reshape(-1)
    rec = np.zeros((len(ids), 5), np.int64)
    ok = (ids >= 0) & (ids < n)
    rec[~ok, 0] = -1
    who = np.flatnonzero(ok)
    row = ids[who].copy()
    lo, hi, ahi = np.zeros(len(who), np.int64), np.full(len(who), N, np.int64), np.full(len(who), n, np.int64)
    z = fm.occ[:, 0]
    j = n_early = 0
    while len(who):
        c = fm.bwt[row].astype(np.int64)
        end = c == 0
        if end.any():
            e = who[end]
            if j == 0:
                rec[e, 0] = 4
            else:
                one = (ahi - lo == 1)[end]                          # [lo, ahi) is the row itself
                occ, neq, rank = (hi - lo)[end], np.where(one, 1, (z[ahi] - z[lo])[end]), np.where(one, 0, (z[row] - z[lo])[end])
                rec[e] = np.stack([(rank != 0) * 1 + (occ > neq) * 2, occ, neq, rank, np.full(len(e), j)], 1)
        go = ~end
        who, row, lo, hi, ahi, c = who[go], row[go], lo[go], hi[go], ahi[go], c[go]
        if j >= N:
            rec[who, 0] = -2
            break
        one = ahi - lo == 1
        row = fm.C[c] + fm.occ[row, c]
        lo = fm.C[c] + fm.occ[lo, c]
        hi = fm.C[c] + fm.occ[hi, c]
        ahi = np.where(one, np.minimum(lo + 1, N), fm.C[c] + fm.occ[np.minimum(ahi, N), c])
        j += 1
        out = row >= N
        rec[who[out], 0] = -2
        stop = out
        if early:
            uniq = ~out & (hi - lo == 1)
            rec[who[uniq]] = [0, 1, 1, 0, j]
            n_early += int(uniq.sum())
            stop = out | uniq
        go = ~stop
        who, row, lo, hi, ahi = who[go], row[go], lo[go], hi[go], ahi[go]
        if check is not None:
            check(row, lo, ahi, hi)
    if info is not None:
        info["early"] = n_early
    return rec


def brute(strings):
    """(occ, n_equal) of every string by bytes.find over the strings themselves: occ = the places where it occurs in any string
    (overlapping ones too, itself included), n_equal = the strings equal to it; (0, 0) for an empty string"""
    bs = [np.asarray(s, np.uint8).tobytes() for s in strings]
    text = b"\0".join(bs)                                            # no string holds a 0, so no match crosses a border
    same = {}
    for b in bs:
        same[b] = same.get(b, 0) + 1
    memo = {}
    out = np.zeros((len(bs), 2), np.int64)
    for k, b in enumerate(bs):
        if not b:
            continue
        if b not in memo:
            cnt, at = 0, text.find(b)
            while at >= 0:
                cnt += 1
                at = text.find(b, at + 1)
            memo[b] = cnt
        out[k] = memo[b], same[b]
    return out


def mixed_reads():
    """the fixture *mixed*: repetitive reads of a short genome, random reads, copies of some of those, substrings of others, empty
    reads and two tiny reads, shuffled; every flag 0 .. 4 occurs"""
    A = H.repetitive_reads(120, seed=21, genome_len=600, max_len=60)
    B = list(H.splitmix_bases(80, 48, seed=9))
    reads = A + B + B[:20] + B[:5] + [b[5:40] for b in B[20:40]] + [np.zeros(0, np.uint8), np.zeros(0, np.uint8)]
    reads += [np.array([1, 2, 3, 4], np.uint8), np.array([1, 1, 2, 4, 3, 4, 4], np.uint8)]
    return [reads[i] for i in np.random.RandomState(1).permutation(len(reads))]


def mixed(so, rev, extra=()):
    """(the two batches, the oracle's BWT) of *mixed* (and the reads extra behind it), one strand or both"""
    reads = mixed_reads() + list(extra)
    half = len(reads) // 2
    bufs = [H.encode_batch(reads[:half], True, rev), H.encode_batch(reads[half:], True, rev)]
    o = H.Oracle(so)
    for b in bufs:
        o.insert_multi(b)
    bwt = o.bwt()
    o.close()
    return bufs, bwt


def survivors_bwt(so, strings):
    """the oracle's BWT of these strings (text order) inserted in order as one batch"""
    o = H.Oracle(so)
    o.insert_multi(H.encode_batch(strings, True, False))
    bwt = o.bwt()
    o.close()
    return bwt


def shuffled_ropes(bwt, seed):
    """the symbols of every rope (rope a has as many rows as the BWT has a's) in a random order: consistent totals, no BWT of strings"""
    cut = np.concatenate([[0], np.cumsum(np.bincount(bwt, minlength=6))])
    rng = np.random.RandomState(seed)
    out = np.array(bwt, np.uint8)
    for a in range(6):
        out[cut[a]:cut[a + 1]] = out[cut[a]:cut[a + 1]][rng.permutation(cut[a + 1] - cut[a])]
    return out
