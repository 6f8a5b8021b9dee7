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

    def extend_many(self, iks, is_back):
        """extend() for an (n, 3) array of bi-intervals at once: (n, 6, 3), by indexing occ and C (no loop over the intervals)"""
        iks = np.asarray(iks, dtype=np.int64).reshape(-1, 3)
        fb = 0 if is_back else 1
        b = 1 - fb
        tk = self.occ[np.clip(iks[:, fb], 0, self.N)]
        tl = self.occ[np.clip(iks[:, fb] + iks[:, 2], 0, self.N)]
        ok = np.zeros((len(iks), 6, 3), np.int64)
        ok[:, :, fb] = self.C[None, :] + tk
        ok[:, :, 2] = tl - tk
        ok[:, 0, b] = iks[:, b]
        for a, prev in ((4, 0), (3, 4), (2, 3), (1, 2), (5, 1)):   # the other end in the complement order $ T G C A N
            ok[:, a, b] = ok[:, prev, b] + ok[:, prev, 2]
        return ok

    def walk_all(self):
        """walk() from every row of the `$` block at once: (the strings, row k's at index k; visits), visits[x] = how often
        row x of the BWT was read -- the walks are the cycles of LF cut at the `$`s, so every row is read exactly once"""
        n = int(self.C[1])
        visits = np.zeros(self.N, np.int64)
        x = np.arange(n, dtype=np.int64)
        who = np.arange(n, dtype=np.int64)
        cols = []                                                   # step j: (the strings still walking, their j-th symbol from the end)
        while len(x):
            np.add.at(visits, x, 1)
            c = self.bwt[x]
            go = c != 0
            x, who, c = x[go], who[go], c[go].astype(np.int64)
            cols.append((who, c.astype(np.uint8)))
            x = self.C[c] + self.occ[x, c]
        lens = np.zeros(n, np.int64)
        for who, _ in cols:
            lens[who] += 1
        out = np.zeros((n, max(len(cols) - 1, 1)), np.uint8)
        for j, (who, c) in enumerate(cols[:-1] if cols else []):
            out[who, lens[who] - 1 - j] = c
        return [out[k, :lens[k]].copy() for k in range(n)], visits

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
