"""Run streams that are hostile to the .fmd code of the device (k_fmds_* in csrc/rb2_fmd_save.h, fmd_runs in csrc/rb2_fmd_load.h, k_ld_* in
csrc/rb2_kernels.h), and their CPU model: the six ropes as run bytes, the count matrix, rank at any row, and what an image of the stream
exercises (events()).  The families are those of tests/fmd_plan_check.cpp, restricted to what a device can hold.

A stream is a list of maximal runs (l, c): neighbours differ, 1 <= l < 2^32, c in 0..5.  Nothing here expands a stream into symbols.
Used by tests/test_fmd_streams_ref.py (CPU) and tests/test_fmd_streams_gpu.py."""
import numpy as np

import fmd_ref
from fmd_save_ref import write_fmd

RUN_MAX = 1 << 32                         # every run is shorter: a 64-bit code behind a word boundary (runs >= 2^50, undefined) cannot occur
SEGS = (96, 97, 128)                      # RB2_FMDS_SEG of the encoder grid
BATCH = 2048                              # RB2_FMDS_BATCH of the encoder grid


# ---- the families -----------------------------------------------------------------------------------------------------------------------
# Symbols: single-symbol runs alternate $ and A (every stream has strings, as an index has), probe runs alternate C and G, the separator
# of the types streams is N.

def _ones(S, n):
    for _ in range(n):
        S.append((1, 1 if S and S[-1][1] == 0 else 0))


def _one(S, l):
    S.append((l, 3 if S and S[-1][1] == 2 else 2))


def _pow_probes(ks):
    return [(1 << k) + d for k in ks for d in (-1, 0, 1)]


def aligned(probes):
    """for a = 0 .. 96 and every probe l: a single-symbol runs, a run of l, 12 single-symbol runs -- one stream"""
    S = []
    for a in range(97):
        for l in probes:
            _ones(S, a); _one(S, l); _ones(S, 12)
    return S


def ones(n):
    S = []
    _ones(S, n)
    return S


TYPES_T = (16383, 16384, (1 << 30) - 1, 1 << 30, 5, 20000)
TYPES_FRONT = (0, 40, 80)
TYPES_REPEAT = 2                          # runs of 2^30 per stream: see types()


def types(T, front):
    """`front` single-symbol runs, TYPES_REPEAT x (a run of 2^30, a run of T), the tail of the plan check's kind 4.  A block behind one of
    2^30 symbols and more has one payload word: a run of T >= 16383 is alone in it when a run of 2^30 follows (its code does not fit
    behind T's), so the next header holds exactly T.  That needs a first block that is nearly full: with 80 runs in front the first
    run of 2^30 still fits into block 0 and the run of T does not; with 0 and 40 all four long runs share block 0 and the types come
    from the tail alone.  The plan check has six runs of 2^30 per stream; two are the fewest with which the eighteen images together
    show all nine header transitions and all four totals (tests/test_fmd_streams_ref.py asserts both), and keep a stream at 2^32 symbols."""
    S = []
    _ones(S, front)
    for _ in range(TYPES_REPEAT):
        _one(S, 1 << 30); S.append((T, 5))
    _ones(S, 200); _one(S, 20000); _ones(S, 3); _one(S, 20000); _one(S, 16384); _ones(S, 100)
    return S


def gamma_edge():
    """2^31 is the shortest run whose length prefix has five zeros, the last fmd_runs accepts (z > 5 is padding)"""
    S = []
    _ones(S, 5)
    for l in ((1 << 31) - 1, 1 << 31, (1 << 31) + 1):
        _one(S, l); _ones(S, 5)
    return S


def random_runs(n=16000, seed=20):
    """lengths log-uniform below 2^16, random symbols.  16 000 runs, 98 M symbols: the 100 000 runs of the plan check are 614 M symbols,
    600 000 batches of 49 us when a batch takes one leaf (RB2_FMDS_BATCH=2048) -- half a minute for that one encoding"""
    rng = np.random.RandomState(seed)
    e = rng.randint(0, 16, size=n)
    l = (1 << e) | (rng.randint(0, 1 << 16, size=n) & ((1 << e) - 1))
    d = rng.randint(1, 6, size=n)
    S, c = [], 0
    for k in range(n):
        c = (c + int(d[k])) % 6
        S.append((int(l[k]), c))
    return S


# name -> (maker, arguments).  The aligned family is one stream per probe set, each below 2^28 symbols, and the long probes are spread
# over several streams: with RB2_FMDS_BATCH=2048 the encoder spends a batch (49 us on an MI355X) per leaf of 1024 symbols, 5 s per 10^8.
FAMILIES = {}
FAMILIES["aligned_1_70_k7_12"] = (aligned, (list(range(1, 71)) + _pow_probes(range(7, 13)),))
FAMILIES["aligned_k13_15"] = (aligned, (_pow_probes(range(13, 16)),))
FAMILIES["aligned_k16_17"] = (aligned, (_pow_probes(range(16, 18)),))
FAMILIES["aligned_k18"] = (aligned, (_pow_probes([18]),))
FAMILIES["aligned_k19a"] = (aligned, ([(1 << 19) - 1, 1 << 19],))
FAMILIES["aligned_k19b"] = (aligned, ([(1 << 19) + 1],))
for _d in (-1, 0, 1):
    FAMILIES["aligned_k20%s" % "abc"[_d + 1]] = (aligned, ([(1 << 20) + _d],))
for _n in (2, 94, 95, 96, 97, 191, 5000, 300000):
    FAMILIES["ones_%d" % _n] = (ones, (_n,))
for _T in TYPES_T:
    for _f in TYPES_FRONT:
        FAMILIES["types_%d_%d" % (_T, _f)] = (types, (_T, _f))
FAMILIES["gamma_edge"] = (gamma_edge, ())
FAMILIES["random"] = (random_runs, ())
NAMES = list(FAMILIES)
SEG_NAMES = [n for n in NAMES if n.startswith(("aligned", "ones", "random"))]     # the streams the segment-entry conditions are about
TYPES_NAMES = [n for n in NAMES if n.startswith("types")]
HUGE = [n for n in NAMES if n.startswith(("types", "gamma"))]                     # streams with runs of 2^30 and more

_streams, _images = {}, {}


def stream(name):
    if name not in _streams:
        f, args = FAMILIES[name]
        S = f(*args)
        check(S)
        _streams[name] = S
    return _streams[name]


def check(S):
    r = _arr(S)
    assert ((r[:, 0] >= 1) & (r[:, 0] < RUN_MAX)).all() and ((r[:, 1] >= 0) & (r[:, 1] <= 5)).all(), "run length or symbol"
    assert (r[1:, 1] != r[:-1, 1]).all(), "neighbouring runs of one symbol"


def image(name, tmp):
    """the host writer's image of the stream (fmd_save_ref.write_fmd, one push per run), made once per process"""
    if name not in _images:
        _images[name] = write_fmd(tmp / (name + ".fmd"), pushes=stream(name))
    return _images[name]


# ---- the CPU model ------------------------------------------------------------------------------------------------------------------------

def _arr(S):
    return np.asarray(S, dtype=np.int64).reshape(-1, 2)


def totals(S):
    r = _arr(S)
    return np.array([r[r[:, 1] == a, 0].sum() for a in range(6)], dtype=np.int64)


def borders(S):
    """C[0 .. 6]: rope a is rows [C[a], C[a + 1]) of the stream, C from the stream's own symbol totals"""
    return np.concatenate([[0], np.cumsum(totals(S))]).astype(np.int64)


def rope_runs(S):
    """the runs (l, c) of the six ropes: the stream cut at the rope borders"""
    r, C = _arr(S), borders(S)
    start = np.concatenate([[0], np.cumsum(r[:, 0])])
    out = []
    for b in range(6):
        lo, hi = int(C[b]), int(C[b + 1])
        if lo == hi:
            out.append([])
            continue
        i0, i1 = int(np.searchsorted(start, lo, "right")) - 1, int(np.searchsorted(start, hi, "left"))
        s, e = np.maximum(start[i0:i1], lo), np.minimum(start[i0 + 1:i1 + 1], hi)
        out.append(list(zip((e - s).tolist(), r[i0:i1, 1].tolist())))
    return out


def run8(l, c):
    """one 8-byte run of the 43+3 codec (rle.h:53-75), as hipbwt.encode_runs writes runs of 2^19 symbols and more"""
    tail = [0x80 | (l >> (6 * k)) & 0x3f for k in range(7)]
    return np.array([0xF0 | (l >> 42) << 3 | c] + tail[::-1], np.uint8)


_LIMIT = {1: 1 << 4, 2: 1 << 8, 4: 1 << 19, 8: 1 << 43}


def _code(out, l, c, n):
    """a run of l symbols c in n bytes (n = 1, 2, 4, 8 and l below the width's limit)"""
    assert 1 <= l < _LIMIT[n]
    if n == 1:
        out.append(l << 3 | c)
    elif n == 8:
        out.extend(run8(l, c).tolist())
    else:
        tail = [0x80 | (l >> (6 * k)) & 0x3f for k in range(n - 1)]
        out.append((0xC0 if n == 2 else 0xE0) | (l >> (6 * (n - 1))) << 3 | c)
        out.extend(tail[::-1])


def min_width(l):
    return 1 if l < 16 else 2 if l < 256 else 4 if l < 1 << 19 else 8


def cut(S, canonical=True, seed=1):
    """the six ropes as 43+3 byte streams (uint8 arrays).  canonical: one code per run, of the least width, as hipbwt.encode_runs writes.
    Otherwise the same symbols in other bytes: a third of the runs of two symbols and more are split into two to four codes of the same
    symbol, and half of the codes are wider than they need to be."""
    rng = np.random.RandomState(seed)
    ropes = []
    for runs in rope_runs(S):
        out = bytearray()
        if canonical:
            for l, c in runs:
                _code(out, l, c, min_width(l))
        else:
            u = rng.randint(0, 1 << 30, size=(len(runs), 6))
            for (l, c), x in zip(runs, u.tolist()):
                parts = [l]
                if l >= 2 and x[0] % 3 == 0:
                    k = min(l, 2 + x[1] % 3)
                    cuts = sorted({1 + x[2 + j] % (l - 1) for j in range(k - 1)})
                    parts = [b - a for a, b in zip([0] + cuts, cuts + [l])]
                for j, p in enumerate(parts):
                    n = min_width(p)
                    w = (x[5] >> (2 * j)) & 3
                    while w and n < 8 and (x[5] >> 8 + j) & 1:
                        n *= 2; w -= 1
                    _code(out, p, c, n)
        ropes.append(np.frombuffer(bytes(out), np.uint8))
    return ropes


def counts(S):
    """M[b][a] = symbols a in rope b (what HipBwt.counts() returns)"""
    M = np.zeros((6, 6), np.int64)
    for b, runs in enumerate(rope_runs(S)):
        for l, c in runs:
            M[b, c] += l
    return M


class Ranks:
    """prefix counts of the six symbols at any global row, from the run list: cumsum and searchsorted"""
    def __init__(self, S):
        r = _arr(S)
        self.c = r[:, 1]
        self.start = np.concatenate([[0], np.cumsum(r[:, 0])])
        self.cum = np.zeros((len(r) + 1, 6), np.int64)
        for a in range(6):
            self.cum[1:, a] = np.cumsum(np.where(r[:, 1] == a, r[:, 0], 0))
        self.C = borders(S)

    def at(self, p):
        p = np.asarray(p, np.int64)
        i = np.minimum(np.searchsorted(self.start, p, "right") - 1, len(self.c) - 1)
        out = self.cum[i].copy()
        out[np.arange(len(p)), self.c[i]] += p - self.start[i]
        return out

    def rope(self, b, xs):
        return self.at(self.C[b] + np.asarray(xs, np.int64)) - self.at(self.C[b:b + 1])

    def probes(self, b, cap=1 << 20):
        """rows of rope b worth asking: every run start, the row before and the row behind, clipped to the rope, `cap` at the most"""
        lo, hi = int(self.C[b]), int(self.C[b + 1])
        s = self.start[(self.start >= lo) & (self.start <= hi)] - lo
        xs = np.unique(np.clip(np.concatenate([s - 1, s, s + 1, [0, hi - lo]]), 0, hi - lo))
        if len(xs) > cap:
            xs = xs[np.unique(np.linspace(0, len(xs) - 1, cap).astype(np.int64))]
        return xs


def ranks(S, b, xs):
    """the six prefix counts at rows xs of rope b"""
    return Ranks(S).rope(b, xs)


def decode43(rle):
    """a plain decoder of the 43+3 codec (rle.h): the runs (l, c) of a byte stream, code by code"""
    runs, i, rle = [], 0, bytes(rle)
    while i < len(rle):
        h = rle[i]
        n = 1 if h < 0x80 else 2 if h >> 5 == 6 else 4 if h >> 4 == 14 else 8
        l = h >> 3 & (15 if n == 1 else 3 if n == 2 else 1)
        for q in rle[i + 1:i + n]:
            assert q >> 6 == 2, "continuation byte"
            l = l << 6 | q & 0x3f
        runs.append((l, h & 7))
        i += n
    return runs


def merge(runs):
    """neighbouring runs of one symbol joined"""
    out = []
    for l, c in runs:
        if out and out[-1][1] == c:
            out[-1][0] += l
        else:
            out.append([l, c])
    return [(l, c) for l, c in out]


# ---- what an image exercises ------------------------------------------------------------------------------------------------------------------

def width(l):
    """bits of the code of a run of l symbols: the gamma code of its bit count, the bits below its leading one, three of the symbol"""
    y = l.bit_length() - 1
    return 2 * ((y + 1).bit_length() - 1) + 1 + y + 3


def entries(E, m):
    """(offset in its block, type of the block, type of the block in front) of every run of events() E whose number IN THE STREAM is a
    multiple of m.  On the device a segment is RB2_FMDS_SEG heads of one batch's head array, the heads carried over from the batch
    before included (fmds_encode in rb2_engine.hip), so these are the device's segment borders only while the stream is one batch: all
    of every stream here at the default batch of 2^24 heads.  With RB2_FMDS_BATCH=2048, and in any later batch, the device's borders
    lie elsewhere; the coverage conditions are about the stream, as the plan of the tests defines them."""
    return E["where"][::m]


def events(img, seg=96, batch=BATCH):
    """what the image holds, from fmd_ref.decode(img) alone (the names are those of Events in fmd_plan_check.cpp):
    blocks      per block (type, runs, used payload bits)
    word_end / bit_before / exact / refused_exact   codes that end on a word's last bit before the last word / one bit before the block's
                end / on the block's last bit / first codes of a next block that would have ended exactly on the last bit
    trans[a][b] header of type a followed by one of type b (the closing header included)
    totals      blocks of 16383, 16384, 2^30 - 1 and 2^30 symbols
    where       per run: (offset of the run in its block, type of the block, type of the block in front or -1)
    seg_entry / batch_entry   the rows of `where` of the runs whose number is a multiple of seg / batch (entries(E, m) for any other m)"""
    d = fmd_ref.decode(img)
    words = d["words"]
    E = {"blocks": [], "word_end": 0, "bit_before": 0, "exact": 0, "refused_exact": 0, "trans": np.zeros((3, 3), np.int64),
         "totals": {16383: 0, 16384: 0, (1 << 30) - 1: 0, 1 << 30: 0}, "where": []}
    nb = len(d["blocks"])
    tl = [t for t, _, _ in d["blocks"]] + [int(words[nb * fmd_ref.BLK]) >> 62]
    for j, (t, _, runs) in enumerate(d["blocks"]):
        C = 64 * ((fmd_ref.BLK - 1 if (j + 1) * fmd_ref.BLK % fmd_ref.CHUNK == 0 else fmd_ref.BLK) - fmd_ref.HDR_WORDS[t])
        u = 0
        for k, (c, l) in enumerate(runs):
            E["where"].append((k, t, tl[j - 1] if j else -1))
            u += width(l)
            assert u <= C
            E["word_end"] += u % 64 == 0 and u < C
            E["bit_before"] += u == C - 1
            E["exact"] += u == C
        E["blocks"].append((t, len(runs), u))
        if j + 1 < nb and d["blocks"][j + 1][2] and u + width(d["blocks"][j + 1][2][0][1]) == C:
            E["refused_exact"] += 1
        E["trans"][t][tl[j + 1]] += 1
        tot = sum(l for _, l in runs)
        if tot in E["totals"]:
            E["totals"][tot] += 1
    E["seg_entry"], E["batch_entry"] = entries(E, seg), entries(E, batch)
    E["runs"] = [(l, c) for c, l in d["runs"]]
    E["mcnt"] = d["mcnt"]
    return E


def locate(img, byte, seg):
    """where byte `byte` of the image lies: block, word, the runs of the block and their segment of `seg` runs -- counted from the first
    run of the stream, which is the device's segment only in a first batch (see entries()); with small batches take it as a hint"""
    if byte < 80:
        return "byte %d of the file header" % byte
    d = fmd_ref.parse(img)
    if byte >= 80 + d["n_bytes"]:
        f, w = divmod(byte - 80 - d["n_bytes"], 56)
        return "word %d of rank frame %d" % (w // 8, f)
    j, w = divmod((byte - 80) // 8, fmd_ref.BLK)
    E = events(img, seg)
    if j >= len(E["blocks"]):
        return "word %d of the closing header (block %d)" % (w, j)
    r0 = sum(n for _, n, _ in E["blocks"][:j])
    t, n, u = E["blocks"][j]
    return "block %d (type %d, %d runs, %d payload bits) word %d (%s); its runs are %d .. %d of the stream, segment %d of %d runs" % (
        j, t, n, u, w, "header" if w < fmd_ref.HDR_WORDS[t] else "payload", r0, r0 + n - 1, r0 // seg, seg)
