"""Models of rb2_hip_unpack and rb2_hip_merge (include/rb2_hip.h) on the CPU, over the oracle's BWT.

unpack = the inverse BWT of query_ref.FM.walk_all (string k = row k of the `$` block), formatted as the (txt, off) the call returns.
merge  = the oracle given src's strings again, in the row order of src's `$` block, cut into batches anywhere."""
import numpy as np

import helpers as H
import query_ref as Q


def strings(bwt):
    """the strings of a BWT in the row order of its `$` block, in text order"""
    return Q.FM(bwt).walk_all()[0] if len(bwt) else []


def pack(strs, reversed=False):
    """(txt, off) of rb2_hip_unpack for these strings: each followed by one 0, last symbol first when reversed"""
    off = np.zeros(len(strs) + 1, np.int64)
    parts = []
    for i, s in enumerate(strs):
        s = np.asarray(s, np.uint8)
        parts += [s[::-1] if reversed else s, np.zeros(1, np.uint8)]
        off[i + 1] = off[i] + len(s) + 1
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), off


def unpack(bwt, first=0, n=None, reversed=False):
    s = strings(bwt)
    return pack(s[first:] if n is None else s[first:first + n], reversed)


def cut(strs, sizes):
    """the strings in consecutive groups of these sizes (the last group takes the rest; None: one group)"""
    if sizes is None:
        return [strs] if strs else []
    out, i = [], 0
    for k in sizes:
        if strs[i:i + k]:
            out.append(strs[i:i + k])
        i += k
    if strs[i:]:
        out.append(strs[i:])
    return out


def merge(so, dst_batches, src_bwt, sizes=None):
    """the BWT after the batches of dst and then the strings of src, in src's row order, in groups of `sizes`"""
    o = H.Oracle(so)
    for b in dst_batches:
        o.insert_multi(b)
    for grp in cut(strings(src_bwt), sizes):
        o.insert_multi(pack(grp, True)[0])
    bwt, cnt = o.bwt(), o.counts()
    o.close()
    return bwt, cnt


def oracle_bwt(so, batches):
    o = H.Oracle(so)
    for b in batches:
        if len(b):
            o.insert_multi(b)
    bwt = o.bwt()
    o.close()
    return bwt


def mixed_reads(n, seed):
    """repetitive_reads (duplicates, N, empty strings among them) plus explicit empty, one-symbol and duplicated strings"""
    r = H.repetitive_reads(n, seed=seed, max_len=40)
    r += [np.zeros(0, np.uint8), np.array([3], np.uint8), np.zeros(0, np.uint8), np.array([5], np.uint8)]
    r += [x.copy() for x in r[:n // 5]]
    return r
