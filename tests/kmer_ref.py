"""numpy reference of the k-mer enumeration of include/rb2_hip.h (rb2_hip_kmers), two ways:

  model()   over a query_ref.FM: the level-wise expansion the device runs, vectorised -- the two ranks of every interval of a level give
            the intervals of all four left extensions, an extension below min_occ is dropped for good;
  brute()   over the strings themselves, never a BWT: every window of k symbols, those with a code outside 1..4 dropped, np.unique.

Codes are packed as the header says: two bits per symbol, A C G T = 0 1 2 3, the symbol at text position p at bits 2 * (k - 1 - p)."""
import numpy as np

U = np.uint64


def pack(windows):
    """(n, k) nt6 codes 1..4 -> uint64 codes"""
    w = np.asarray(windows, dtype=np.uint64)
    k = w.shape[1]
    sh = U(2) * np.arange(k - 1, -1, -1, dtype=np.uint64)
    return np.bitwise_or.reduce((w - U(1)) << sh[None, :], axis=1) if len(w) else np.zeros(0, np.uint64)


def unpack(codes, k):
    codes = np.asarray(codes, dtype=np.uint64).reshape(-1)
    sh = U(2) * np.arange(k - 1, -1, -1, dtype=np.uint64)
    return ((codes[:, None] >> sh[None, :]) & U(3)).astype(np.uint8) + np.uint8(1)


def revcomp_codes(codes, k):
    """the codes of the reverse complements, symbol by symbol (no bit tricks: this is the reference)"""
    w = unpack(codes, k)
    return pack(5 - w[:, ::-1])


def is_canonical(codes, k):
    return np.asarray(codes, np.uint64) <= revcomp_codes(codes, k)


def brute(strings, k, min_occ=1, canonical=False):
    """(codes uint64 sorted, counts int64) of the k-mers of the strings with at least min_occ occurrences"""
    wins = []
    for s in strings:
        s = np.asarray(s, dtype=np.uint8)
        if len(s) >= k:
            w = np.lib.stride_tricks.sliding_window_view(s, k)
            wins.append(w[((w >= 1) & (w <= 4)).all(1)])
    if not wins:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    codes, cnt = np.unique(pack(np.concatenate(wins)), return_counts=True)
    keep = cnt >= min_occ
    if canonical:
        keep &= is_canonical(codes, k)
    return codes[keep], cnt[keep].astype(np.int64)


def model(fm, k, min_occ=1, canonical=False):
    """(codes, lo, hi) sorted by lo, and pre = the k-mers that met min_occ before the canonical filter"""
    code = np.zeros(1, np.uint64)
    lo = np.zeros(1, np.int64)
    hi = np.full(1, fm.N, np.int64)
    if fm.N < min_occ:
        code, lo, hi = code[:0], lo[:0], hi[:0]
    for l in range(k):
        cl, ch = fm.occ[lo], fm.occ[hi]                              # (n, 6) each: the two ranks of every item
        nlo = fm.C[None, 1:5] + cl[:, 1:5]
        nhi = fm.C[None, 1:5] + ch[:, 1:5]
        ncode = code[:, None] | (np.arange(4, dtype=np.uint64)[None, :] << U(2 * l))
        live = nhi - nlo >= min_occ
        code, lo, hi = ncode[live], nlo[live], nhi[live]
    pre = len(code)
    if canonical:
        keep = is_canonical(code, k)
        code, lo, hi = code[keep], lo[keep], hi[keep]
    o = np.argsort(lo, kind="stable")
    return code[o], lo[o], hi[o], pre


def spectrum(counts, hist_len):
    """hist[c] = k-mers with exactly c occurrences, the last bin holding hist_len - 1 or more"""
    if hist_len == 0:
        return np.zeros(0, np.int64)
    return np.bincount(np.minimum(np.asarray(counts, np.int64), hist_len - 1), minlength=hist_len).astype(np.int64)
