"""numpy reference of the FM-index queries of include/rb2_hip.h, over a BWT array (global rows, ropes $ .. N back to back).

Small indexes only: occ() keeps a full (N + 1) x 6 table.  The coordinates are those of the header: C[a] = rows in front of rope a,
occ(a, x) = a's in rows [0, x), patterns are nt6 codes in text order with `$` (0) allowed only as the last symbol.
"""
import numpy as np

COMP = np.array([0, 4, 3, 2, 1, 5], np.uint8)     # complement of an nt6 code ($ and N are their own)


class FM:
    def __init__(self, bwt):
        self.bwt = np.asarray(bwt, dtype=np.uint8)
        self.N = len(self.bwt)
        self.occ = np.zeros((self.N + 1, 6), np.int64)
        if self.N:
            self.occ[1:] = np.cumsum(np.eye(6, dtype=np.int64)[self.bwt], axis=0)
        cnt = self.occ[self.N]
        self.C = np.concatenate([[0], np.cumsum(cnt)[:5]]).astype(np.int64)

    def backward_search(self, pat):
        """(lo, hi, m) exactly as rb2_hip_backward_search"""
        pat = np.asarray(pat, dtype=np.int64)
        if ((pat < 0) | (pat > 5)).any() or (len(pat) and (pat[:-1] == 0).any()):
            return -1, -1, -1
        lo, hi, m = 0, self.N, 0
        for c in pat[::-1]:
            nl, nh = self.C[c] + self.occ[lo, c], self.C[c] + self.occ[hi, c]
            if nl >= nh:
                break
            lo, hi, m = int(nl), int(nh), m + 1
        return lo, hi, m

    def count(self, pat):
        lo, hi, m = self.backward_search(pat)
        return hi - lo if m == len(pat) else 0

    def extend(self, ik, is_back):
        """rld_extend (rld0.c:474-490): ok[a] = (x0, x1, x2) of the extension of bi-interval ik by a"""
        ik = [int(v) for v in ik]
        fb = 0 if is_back else 1
        x = min(max(ik[fb], 0), self.N)
        y = min(max(ik[fb] + ik[2], 0), self.N)
        tk, tl = self.occ[x], self.occ[y]
        ok = np.zeros((6, 3), np.int64)
        for a in range(6):
            ok[a, fb] = self.C[a] + tk[a]
            ok[a, 2] = tl[a] - tk[a]
        b = 1 - fb
        ok[0, b] = ik[b]
        ok[4, b] = ok[0, b] + ok[0, 2]
        ok[3, b] = ok[4, b] + ok[4, 2]
        ok[2, b] = ok[3, b] + ok[3, 2]
        ok[1, b] = ok[2, b] + ok[2, 2]
        ok[5, b] = ok[1, b] + ok[1, 2]
        return ok

    def walk(self, row):
        """the string whose `$` sits at row `row` of the $ block, in text order (inverse BWT by LF steps)"""
        out, x = [], int(row)
        while True:
            c = int(self.bwt[x])
            if c == 0:
                return np.array(out[::-1], np.uint8)
            out.append(c)
            x = int(self.C[c] + self.occ[x, c])

    def sym_interval(self, c):
        """the bi-interval of the one-symbol pattern c (fermi's fm6_set_intv)"""
        return [int(self.C[c]), int(self.C[COMP[c]]), int(self.occ[self.N, c])]


def revcomp(p):
    p = np.asarray(p, dtype=np.uint8)
    return COMP[p[::-1]]


def brute_count(strings, pat):
    """occurrences of pat (text order; a trailing 0 = the string end) in the strings, overlapping ones included"""
    pat = np.asarray(pat, dtype=np.uint8)
    n = 0
    for s in strings:
        t = np.concatenate([np.asarray(s, np.uint8), [0]])
        L = len(pat)
        if L == 0:
            n += len(t)
            continue
        for i in range(len(t) - L + 1):
            if t[i] == pat[0] and np.array_equal(t[i:i + L], pat):
                n += 1
    return n


def inserted_strings(reads, fwd=True, rev=False):
    """the strings a batch of helpers.encode_batch(reads, fwd, rev) inserts, in text order and in insertion order"""
    out = []
    for r in reads:
        r = np.asarray(r, dtype=np.uint8)
        if fwd:
            out.append(r)
        if rev:
            out.append(revcomp(r))
    return out
