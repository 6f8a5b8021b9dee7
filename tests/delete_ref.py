"""numpy model of string deletion (include/rb2_hip.h: rb2_hip_delete_strings) over a BWT array (global rows, ropes $ .. N back to back).

String k is row k of the `$` block.  Its rows are its LF walk from row k until the BWT symbol is `$`; deleting it drops those rows and
nothing else.  The walk spells the string last symbol first, which is the order a string has in an insert buffer (helpers.encode_batch),
so the walks of the survivors, each followed by a 0, are the buffer that builds the index of the survivors.
"""
import numpy as np


def lf_array(bwt):
    """lf[x] = row of the suffix one longer than that of row x (meaningless where bwt[x] is `$`)"""
    bwt = np.asarray(bwt, dtype=np.uint8)
    cnt = np.bincount(bwt, minlength=6)
    C = np.concatenate([[0], np.cumsum(cnt)[:5]]).astype(np.int64)
    lf = np.zeros(len(bwt), np.int64)
    for c in range(1, 6):
        idx = np.flatnonzero(bwt == c)
        lf[idx] = C[c] + np.arange(len(idx), dtype=np.int64)
    return lf


def n_strings(bwt):
    return int((np.asarray(bwt, dtype=np.uint8) == 0).sum())


def gone_rows(bwt, ids):
    """bool mask over the rows: the rows of the strings ids (their walks); ids in any order, duplicates allowed"""
    bwt = np.asarray(bwt, dtype=np.uint8)
    x = np.unique(np.asarray(ids, dtype=np.int64).reshape(-1))
    assert len(x) == 0 or (x[0] >= 0 and x[-1] < n_strings(bwt)), "an id is no string of the index"
    lf = lf_array(bwt)
    gone = np.zeros(len(bwt), bool)
    steps = 0
    while len(x):
        assert not gone[x].any() and steps <= len(bwt), "a row lies on two walks, or a walk does not end"
        gone[x] = True
        x = lf[x[bwt[x] != 0]]
        steps += 1
    return gone


def delete(bwt, ids):
    """(BWT without the rows of the strings ids, rows removed)"""
    bwt = np.asarray(bwt, dtype=np.uint8)
    gone = gone_rows(bwt, ids)
    return bwt[~gone], int(gone.sum())


def walks(bwt, ids=None):
    """the strings ids (default: all, in id order) as their walks spell them: one uint8 array per id, last symbol first"""
    bwt = np.asarray(bwt, dtype=np.uint8)
    ids = np.arange(n_strings(bwt), dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64).reshape(-1)
    lf = lf_array(bwt)
    out = np.zeros((len(ids), 64), np.uint8)
    lens = np.zeros(len(ids), np.int64)
    x, who, j = ids.copy(), np.arange(len(ids)), 0
    while len(x):
        c = bwt[x]
        live = c != 0
        lens[who[~live]] = j
        x, who, c = x[live], who[live], c[live]
        if j == out.shape[1]:
            out = np.concatenate([out, np.zeros_like(out)], axis=1)
        out[who, j] = c
        x = lf[x]
        j += 1
        assert j <= len(bwt) + 1, "a walk does not end"
    return [out[i, :lens[i]].copy() for i in range(len(ids))]


def buffer_of(strings):
    """walks -> the insert buffer that holds them in this order"""
    if not strings:
        return np.zeros(0, np.uint8)
    return np.ascontiguousarray(np.concatenate([np.concatenate([np.asarray(s, np.uint8), np.zeros(1, np.uint8)]) for s in strings]))


def survivors(bwt, ids):
    """the walks of the strings that are not in ids, in id order"""
    keep = np.ones(n_strings(bwt), bool)
    keep[np.asarray(ids, dtype=np.int64).reshape(-1)] = False
    return walks(bwt, np.flatnonzero(keep))


def new_ids(n, ids):
    """where the n old ids go: old id k -> k minus the deleted ids below k, -1 for a deleted one"""
    keep = np.ones(n, bool)
    keep[np.asarray(ids, dtype=np.int64).reshape(-1)] = False
    return np.where(keep, np.cumsum(keep) - 1, -1)
