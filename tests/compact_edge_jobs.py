"""Inputs that put the dense merge's window formats (csrc/rb2_merge.h) at their edges BY CONSTRUCTION, for tests/test_compact_edges_gpu.py
(GPU) and tests/test_bcr_rounds_ref.py (the coverage they reach, from the model alone).  Generated from fixed seeds, nothing stored.

In input order on an empty index the rows that end a read are in read order: rope `$` takes the reads' last symbols in read order, and
for a fixed tail S the rows `S$` -- they sit in piece (S[0], S[1]), in front of every other row that starts with S -- take the symbol in
front of S of the reads that end in S, in read order.  A block of 4096 k reads that end in S and carry `N` in front of S exactly where
wanted therefore gives k windows with any exception counts, at any positions.  Every later round rewrites them (aligned: nothing is
inserted in front); reads of a LATER batch that end in S without its last symbol land in front of all of them and shift the whole block.
"""
import numpy as np

import helpers as H
from bcr_rounds_ref import WIN

A, C, G, T, N = 1, 2, 3, 4, 5

# exception counts of the designed windows of rope `$` and of piece (A,$): both sides of XCAP1 = 63 and XCAP2 = 127, none, one, all
EDGE_COUNTS = [0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 200, WIN, 0]
# piece (G,C), rows `GCA$`: formats C0 C0 C1 C0 C2 C0 P C1 C1 C2 C1 P C2 C2 P P C0 -- every ordered pair of formats is a pair of neighbours
PAIR_COUNTS = [0, 0, 1, 0, 64, 0, 128, 63, 62, 127, 33, 129, 65, 126, 200, 1500, 0]
# where the exceptions of a window go first: both ends, the groups a shift by 100 (g0 = 62, sh0 = 28) and by 1989 (g0 = 32, sh0 = 59) puts
# at the head of the stage, into its 65th group and just behind it, the ends of groups 0 and 1; the rest at random
FIRST = [0, WIN - 1, 62 * 64 + 27, 62 * 64 + 40, 63 * 64 + 3, 32 * 64 + 58, 32 * 64 + 60, 33 * 64, 61 * 64 + 63, 31 * 64 + 5, 63, 64]


def exception_mask(counts, rng):
    """one flag per position of len(counts) windows: window w holds exactly counts[w] exceptions"""
    m = np.zeros((len(counts), WIN), bool)
    for w, t in enumerate(counts):
        if t >= WIN:
            m[w] = True
            continue
        pos = FIRST[:t]
        if t > len(FIRST):
            rest = np.setdiff1d(np.arange(WIN), FIRST)
            pos = pos + list(rng.choice(rest, t - len(FIRST), replace=False))
        m[w, pos] = True
        assert m[w].sum() == t
    return m.reshape(-1)


def _bodies(n, lo, hi, rng):
    return [rng.integers(1, 5, size=int(k)).astype(np.uint8) for k in rng.integers(lo, hi + 1, size=n)]


def tail_block(mask, tail, rng, lo=0, hi=2, fill=(A, C, G, T)):
    """one read per flag: a short random body, then `N` where the flag is set (else one of `fill`), then the fixed tail"""
    tail = np.asarray(tail, np.uint8)
    w = np.where(mask, N, rng.choice(np.asarray(fill, np.uint8), size=len(mask))).astype(np.uint8)
    return [np.concatenate([b, w[i:i + 1], tail]) for i, b in enumerate(_bodies(len(mask), lo, hi, rng))]


def designed_job():
    """three batches.  The first builds the designed windows: rope `$` (the reads' last symbols: `N` where wanted, else T -- all 4096
    symbols of a window are new in the round that makes them), piece (A,$) (tail `A`: `N` or T in front of it) and the rows `GCA$` of piece
    (G,C), then 300 reads that leave piece (A,$) a partly filled last window with exceptions.  No read of the first batch ends in `GC`, so
    the 100 reads of the second batch and the 1989 of the third that do are inserted IN FRONT of the rows `GCA$`, some of them with an `N`:
    every window of the block is then put together from two old windows at a bit offset, through a stage of 65 groups.  The later batches
    also bring reads of mixed lengths with empty strings and extend the partly filled windows."""
    rng = np.random.default_rng(1201)
    b1 = tail_block(exception_mask(EDGE_COUNTS, rng), [], rng, 1, 3, fill=(T,))
    b1 += tail_block(exception_mask(EDGE_COUNTS, rng), [A], rng, 0, 2, fill=(T,))
    b1 += tail_block(exception_mask(PAIR_COUNTS, rng), [G, C, A], rng, 0, 2)
    b1 += tail_block(rng.random(300) < 0.07, [A], rng, 0, 2, fill=(T,))
    out = [H.encode_batch(b1)]
    for n_front, n_mixed, seed in ((100, 1500, 1202), (1989, 700, 1203)):
        rng = np.random.default_rng(seed)
        b = tail_block(rng.random(n_front) < 0.15, [G, C], rng, 0, 3)
        b += tail_block(rng.random(211) < 0.1, [A], rng, 0, 2, fill=(T,))
        mixed = _bodies(n_mixed, 0, 40, rng)
        for r in mixed[::9]:
            if len(r):
                r[rng.integers(0, len(r))] = N
        b += mixed
        out.append(H.encode_batch(b))
    return out


def graded_job():
    """two batches of reads of 30 to 60 symbols in which the probability of an `N` at a position rises with the value of the fourth and
    fifth symbol behind it: along a piece (b, x), whose rows are sorted by what follows `b x`, the exceptions per window climb from none
    past 128 -- compact windows with no, one and two lines and plain ones as neighbours, read back at every offset once the deeper rounds
    insert in front of them.  With a block of very short reads and a block of runs of `N` (plain windows among compact ones of a piece)."""
    out = []
    for n, seed in ((7000, 1301), (5000, 1302)):
        rng = np.random.default_rng(seed)
        reads = []
        for k in rng.integers(30, 61, size=n):
            r = rng.integers(1, 5, size=int(k)).astype(np.uint8)
            v = np.zeros(len(r))
            v[:-4] = (4.0 * (r[3:-1] - 1) + (r[4:] - 1)) / 15.0
            r[rng.random(len(r)) < 0.03 * v ** 1.5] = N           # (the value is taken from the bases, before any `N` is put in)
            reads.append(r)
        reads += _bodies(1500, 1, 6, rng)
        reads += [np.concatenate([np.full(int(k), N, np.uint8), rng.integers(1, 5, size=30).astype(np.uint8)]) for k in rng.integers(60, 86, size=60)]
        reads += [np.zeros(0, np.uint8)] * 5
        order = rng.permutation(len(reads))
        out.append(H.encode_batch([reads[i] for i in order]))
    return out


JOBS = {"designed": designed_job, "graded": graded_job}
_cache = {}


def job(name):
    if name not in _cache:
        _cache[name] = JOBS[name]()
    return _cache[name]
