"""Round-by-round numpy model of the batch insertion in INPUT ORDER (so = 0), written from DESIGN.md section 3, and of what the dense
merge is handed and must decide per output window in every round (csrc/rb2_merge.h "window formats", k_part in csrc/rb2_kernels.h).

The whole BWT is one array (ropes $ .. N back to back).  One round = one string position, last symbol first:

  * every string still running inserts its symbol a_k in front of position e_k of the array AS IT WAS (round 0: the end of rope `$`);
  * a stable sort by e_k gives slot q, the final position is e_q + q, the new array is the merge of the old symbols and the new ones;
  * the string's next position is C[a] + occ(a, final position) on the NEW array; a string that has inserted its `$` is done.
    (C[a] = rows in front of rope a.  In the middle of a batch a symbol's own row comes one round after the symbol, so the model counts
    ROWS per piece as it goes -- a string in piece (b, x) that inserts a moves to piece (a, b) -- and the matrix gives the same sizes
    once the batch is through.)

After every round the model cuts the array into the 31 pieces (rope `$`, then (b, x) = the b's of rope x, from the 6 x 6 count matrix:
the bounds tests/test_query_gpu.py::test_piece_and_rope_boundaries derives) and every piece into windows of WIN symbols counted from the
piece's start, and reports per window what k_part puts into its work order and what k_merge has to choose (class Round).

Small inputs only (below ~10^6 symbols, ~100 rounds): every round makes a handful of O(N) passes.  Test infrastructure like
query_ref.py: the product never imports it.
"""
import numpy as np

WIN = 4096                                  # symbols per window (WPL leaves of 1024)
GSYM = 64                                   # symbols per group (one lane of the merge wave)
WG = 64                                     # groups per window
NR = 31                                     # pieces: rope $ + (b, x), b = A..N, x = $..N
PLAIN, C0, C1, C2 = 0, 1, 2, 3              # WF_PLAIN, WF_C0, WF_C1, WF_C2
NONE = 4                                    # model only: "this old window does not exist" (k_part hands it to the merge as C0)
XCAP1, XCAP2 = 63, 127
FMT_NAME = ["plain", "compact0", "compact1", "compact2"]
HNAME = ["P", "C0", "C1", "C2", "none"]


def format_of(xt):
    """the format a window with xt exceptions ($ and N symbols) gets when compact output is allowed"""
    xt = np.asarray(xt)
    return np.where(xt == 0, C0, np.where(xt <= XCAP1, C1, np.where(xt <= XCAP2, C2, PLAIN))).astype(np.uint8)


def split_batch(buf):
    """start and length (without the sentinel) of every reversed, 0-terminated string of a batch buffer"""
    buf = np.asarray(buf, dtype=np.uint8)
    ends = np.flatnonzero(buf == 0)
    assert len(buf) == 0 or buf[-1] == 0, "a batch ends with a sentinel"
    starts = np.concatenate([[0], ends[:-1] + 1]).astype(np.int64) if len(ends) else np.zeros(0, np.int64)
    return starts, (ends - starts).astype(np.int64)


def piece_sizes(matrix):
    """sizes of the 31 pieces in array order from the count matrix (matrix[x][b] = b's in rope x): rope `$` is one piece"""
    m = np.asarray(matrix, dtype=np.int64)
    return np.concatenate([[m[:, 0].sum()], m[:, 1:].T.reshape(-1)]).astype(np.int64)


def matrix_of(bwt):
    cnt = np.bincount(bwt, minlength=6).astype(np.int64)
    C = np.concatenate([[0], np.cumsum(cnt)])
    return np.stack([np.bincount(bwt[C[x]:C[x + 1]], minlength=6) for x in range(6)]).astype(np.int64)


class Round:
    """one round as the dense merge sees it.  Arrays with one entry per output window, in piece order:

    piece, j       the piece (0 .. 30) and the window's number inside it
    nvalid         symbols in the window (WIN, or fewer in the last window of a piece)
    xt, fmt        its `$` + `N` symbols and the format it is written in (plain in a round that may not write compact windows)
    ni, new_x      symbols that are new this round, and how many of those are `$` / `N`
    x_ends         its first and its last symbol are both exceptions
    i0, g0, sh0    piece position (as the piece was) of its first old symbol = 4096 j - inserts in front, its group and bit there
    nwg            old groups staged: (sh0 + nvalid - ni + 63) >> 6, 0 when nothing is old
    two            some staged group lies in the second old window (g0 + nwg > 64)
    h0, h1         formats of old windows i0 >> 12 and the next one after the round before (NONE: no such window)
    len0, len1     their exception counts (list lengths when compact; -1: no such window)
    x_front        exceptions of the first old window in groups in front of g0 (the merge must drop them)
    x_tail         exceptions of the second old window in the stage's 65th group (group g0 of it), counted when nwg == 65
    x_behind       exceptions of the second old window behind the stage (its groups > g0), counted when `two`

    and of the whole array: isnew (one flag per symbol: new this round), start / old_start (first row of every piece after / before the
    round, NR + 1 entries), old (the array as it was; the model's .bwt is the array as it is), ins (NR entries: the inserts every
    piece takes this round)
    """

    def __init__(self, batch, r, compact, last, **kw):
        self.batch, self.r, self.compact, self.last = batch, r, compact, last   # last: the batch's last round (nothing reads its windows as lists)
        self.__dict__.update(kw)

    def counts(self):
        c = np.bincount(self.fmt, minlength=4)
        return {FMT_NAME[k]: int(c[k]) for k in range(4)}


class RoundsModel:
    def __init__(self, compact=True):
        self.bwt = np.zeros(0, np.uint8)
        self.compact_ok = compact                                   # False: RB2_COMPACT=0
        self.fmt = [np.zeros(0, np.uint8) for _ in range(NR)]       # per piece: the formats / exception counts of its windows after the last round
        self.xt = [np.zeros(0, np.int64) for _ in range(NR)]
        self.stats = {"plain": 0, "compact0": 0, "compact1": 0, "compact2": 0, "compact_rounds": 0}
        self.nbatch = 0
        self.sz = np.zeros(NR, np.int64)                            # rows of every piece (mid-batch: a symbol's row comes a round after the symbol)

    def matrix(self):
        return matrix_of(self.bwt)

    def insert_multi(self, buf, keep=None):
        """run a batch; keep(round) is called with every Round"""
        for rd in self.rounds(buf):
            if keep is not None:
                keep(rd)

    def rounds(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        starts, lens = split_batch(buf)
        if len(starts) == 0:
            return
        max_len = int(lens.max())
        alive = np.arange(len(starts))                              # strings still running, in input order
        # round 0: behind the last row of rope `$` (one row per string of the index), in input order
        f = int(self.sz[0]) + np.arange(len(starts), dtype=np.int64)
        pc = np.zeros(len(starts), np.int64)                        # the piece each string inserts into
        for r in range(max_len + 1):
            a = buf[starts[alive] + r]
            # which rounds may write compact windows: in input order every interval is empty, so every round but the batch's last
            compact = self.compact_ok and r < max_len
            rd, nxt = self._round(f, a, pc, r, compact, r == max_len)
            self.stats["compact_rounds"] += int(compact)
            for k, v in rd.counts().items():
                self.stats[k] += v
            go = a != 0                                             # a string that has inserted its `$` is done
            # a string in piece (b, x) that inserts a moves to piece (a, b)
            rope = np.where(pc == 0, 0, (pc - 1) // 6 + 1)
            alive, f, pc = alive[go], nxt[go], (1 + (a[go].astype(np.int64) - 1) * 6 + rope[go])
            yield rd
        assert np.array_equal(piece_sizes(self.matrix()), self.sz), "after a batch every symbol but `$` has its row"
        self.nbatch += 1

    def _round(self, f_in, a, pc, r, compact, last):
        """f_in: the final position of every string's symbol (on the array as it will be: positions on the array as it was + slot, see
        below), a: the symbols, pc: the pieces.  Returns the Round and every string's final position of the NEXT round."""
        old = self.bwt
        n_old, q_tot = len(old), len(f_in)
        # DESIGN.md section 3 in its own words: string k inserts in front of position e_k of the array as it was; sorted by e (ties: input order)
        # its slot is q and its final position e_q + q.  The model carries the final positions (they are distinct, and C[a] + occ(a, .) of the
        # round before gives them directly: every symbol but `$` in front of the string's own has its row by the end of this round); e = f - q.
        order = np.argsort(f_in, kind="stable")
        f, as_ = f_in[order], a[order]
        assert q_tot == 0 or (np.diff(f) > 0).all()
        new = np.empty(n_old + q_tot, np.uint8)
        isnew = np.zeros(n_old + q_tot, bool)
        isnew[f] = True
        new[f] = as_
        new[~isnew] = old
        old_sz = self.sz
        new_sz = old_sz + np.bincount(pc, minlength=NR)
        # next round: rope a starts behind rope `$` (one row per string) and the ropes of the smaller symbols, whose rows are all there by then
        cnt = np.bincount(new, minlength=6).astype(np.int64)
        base = np.concatenate([[0, new_sz[0]], new_sz[0] + np.cumsum(cnt[1:5])])
        nxt_s = np.zeros(q_tot, np.int64)
        for s in range(1, 6):
            sel = as_ == s
            if sel.any():
                nxt_s[sel] = base[s] + np.searchsorted(np.flatnonzero(new == s), f[sel])   # C[a] + occ(a, final position)
        nxt = np.empty(q_tot, np.int64)
        nxt[order] = nxt_s

        # ---- pieces and windows of the new array, and what each window draws from
        old_p0 = np.concatenate([[0], np.cumsum(old_sz)])
        new_p0 = np.concatenate([[0], np.cumsum(new_sz)])
        self.sz = new_sz
        cm = np.concatenate([[0], np.cumsum(isnew)]).astype(np.int64)
        assert np.array_equal(cm[new_p0[1:]] - cm[new_p0[:-1]], new_sz - old_sz), "a piece takes its own inserts only"
        assert new_p0[-1] == len(new)
        exc_new = (new == 0) | (new == 5)
        cx = np.concatenate([[0], np.cumsum(exc_new)]).astype(np.int64)
        cnx = np.concatenate([[0], np.cumsum(exc_new & isnew)]).astype(np.int64)
        cxo = np.concatenate([[0], np.cumsum((old == 0) | (old == 5))]).astype(np.int64)
        # the engine's windows (k_setup: nwin = ceil(nleaves / WPL), nleaves = ceil(n / LEAF)): ceil(n / WIN) per piece, none for an empty piece
        nwin = (new_sz + WIN - 1) // WIN
        piece = np.repeat(np.arange(NR), nwin)
        j = np.arange(int(nwin.sum()), dtype=np.int64) - np.repeat(np.cumsum(nwin) - nwin, nwin)
        ws = new_p0[piece] + j * WIN
        nvalid = np.minimum(WIN, new_sz[piece] - j * WIN)
        we = ws + nvalid
        xt = cx[we] - cx[ws]
        ni = cm[we] - cm[ws]
        new_x = cnx[we] - cnx[ws]
        x_ends = exc_new[ws] & exc_new[we - 1]
        i0 = j * WIN - (cm[ws] - cm[new_p0[piece]])
        nold = nvalid - ni
        g0, sh0 = (i0 >> 6) & 63, i0 & 63
        nwg = np.where(nold > 0, (sh0 + nold + 63) >> 6, 0)
        two = g0 + nwg > WG
        ow = i0 >> 12
        # formats and exception counts of the old windows, per piece
        off = np.concatenate([[0], np.cumsum([len(x) for x in self.fmt])]).astype(np.int64)
        ofmt = np.concatenate(self.fmt + [np.zeros(1, np.uint8)])
        oxt = np.concatenate(self.xt + [np.zeros(1, np.int64)])
        onw = (off[1:] - off[:-1])[piece]

        def old_win(w):
            ok = w < onw
            ix = np.where(ok, off[piece] + w, len(ofmt) - 1)
            return np.where(ok, ofmt[ix], NONE).astype(np.uint8), np.where(ok, oxt[ix], -1)

        h0, len0 = old_win(ow)
        h1, len1 = old_win(ow + 1)

        def old_exc(lo, hi):                                        # exceptions at positions [lo, hi) of the old piece
            n = old_sz[piece]
            lo, hi = np.minimum(np.maximum(lo, 0), n), np.minimum(np.maximum(hi, 0), n)
            hi = np.maximum(hi, lo)
            return cxo[old_p0[piece] + hi] - cxo[old_p0[piece] + lo]

        x_front = np.where(nwg > 0, old_exc(ow * WIN, ow * WIN + g0 * GSYM), 0)
        x_tail = np.where(nwg == WG + 1, old_exc((ow + 1) * WIN + g0 * GSYM, (ow + 1) * WIN + (g0 + 1) * GSYM), 0)
        x_behind = np.where(two, old_exc((ow + 1) * WIN + (g0 + 1) * GSYM, (ow + 2) * WIN), 0)
        fmt = format_of(xt) if compact else np.full(len(xt), PLAIN, np.uint8)

        self.bwt = new
        cut = np.cumsum(nwin)[:-1]
        self.fmt = np.split(fmt, cut)
        self.xt = np.split(xt, cut)
        rd = Round(self.nbatch, r, compact, last, piece=piece, j=j, nvalid=nvalid, xt=xt, fmt=fmt, ni=ni, new_x=new_x, x_ends=x_ends, i0=i0, g0=g0, sh0=sh0,
                   nwg=nwg, two=two, h0=h0, h1=h1, len0=len0, len1=len1, x_front=x_front, x_tail=x_tail, x_behind=x_behind,
                   isnew=isnew, start=new_p0, old_start=old_p0, old=old, ins=new_sz - old_sz)
        return rd, nxt


# ---- coverage: which of the places where the format code can be wrong by one did the compact rounds of a job reach -------------------

def required_cases():
    req = ["out_xt=%d" % v for v in (0, 1, 63, 64, 127, 128)] + ["out_xt>1000"]
    req += ["read_len=%d" % v for v in (63, 64, 127)]
    req += ["two:%s,%s" % (HNAME[a], HNAME[b]) for a in range(4) for b in range(4)]
    req += ["one:%s" % HNAME[a] for a in range(4)]
    for side in ("h0", "h1"):
        for f in ("C1", "C2"):
            req += ["%s=%s:%s" % (side, f, c) for c in ("sh0!=0", "g0!=0", "65th_group")]
    req += ["h0=%s:exception_in_front_of_g0" % f for f in ("C1", "C2")]
    req += ["h1=%s:exception_behind_the_stage" % f for f in ("C1", "C2")]
    req += ["h1=%s:exception_in_65th_group" % f for f in ("C1", "C2")]
    req += ["ni>64:compact_old", "new_exception_into_list_window", "partial_last_window_compact_with_exceptions",
            "exception_at_0_and_4095", "window_of_exceptions_only"]
    return req


class Coverage:
    """collects the cases of required_cases() from the rounds of one or more jobs.  A window READS its old windows in the formats the
    round before wrote, so every case about h0 / h1 is a case of a round that follows a compact round."""

    def __init__(self):
        self.seen = set()

    def add(self, rd):
        S = self.seen
        reads0 = rd.nwg > 0                                         # (nothing old: the merge reads no list, whatever k_part handed over)
        lists0 = reads0 & (rd.h0 >= C1) & (rd.h0 <= C2)
        lists1 = rd.two & (rd.h1 >= C1) & (rd.h1 <= C2)
        for v in (63, 64, 127):
            if ((lists0 & (rd.len0 == v)) | (lists1 & (rd.len1 == v))).any():
                S.add("read_len=%d" % v)
        for a in range(4):
            if (reads0 & ~rd.two & (rd.h0 == a)).any():
                S.add("one:%s" % HNAME[a])
            for b in range(4):
                if (rd.two & (rd.h0 == a) & (rd.h1 == b)).any():
                    S.add("two:%s,%s" % (HNAME[a], HNAME[b]))
        for side, h, lists in (("h0", rd.h0, lists0), ("h1", rd.h1, lists1)):
            for fv, f in ((C1, "C1"), (C2, "C2")):
                m = lists & (h == fv)
                for name, cond in (("sh0!=0", rd.sh0 != 0), ("g0!=0", rd.g0 != 0), ("65th_group", rd.nwg == WG + 1)):
                    if (m & cond).any():
                        S.add("%s=%s:%s" % (side, f, name))
                if side == "h0" and (m & (rd.x_front > 0)).any():
                    S.add("h0=%s:exception_in_front_of_g0" % f)
                if side == "h1" and (m & (rd.x_behind > 0)).any():
                    S.add("h1=%s:exception_behind_the_stage" % f)
                if side == "h1" and (m & (rd.x_tail > 0)).any():
                    S.add("h1=%s:exception_in_65th_group" % f)
        if ((rd.ni > 64) & (lists0 | lists1 | (reads0 & (rd.h0 == C0)))).any():
            S.add("ni>64:compact_old")
        if ((rd.new_x > 0) & (lists0 | lists1)).any():
            S.add("new_exception_into_list_window")
        if not rd.compact:
            return
        for v in (0, 1, 63, 64, 127, 128):
            if (rd.xt == v).any():
                S.add("out_xt=%d" % v)
        if (rd.xt > 1000).any():
            S.add("out_xt>1000")
        if ((rd.nvalid < WIN) & (rd.xt > 0) & (rd.fmt != PLAIN)).any():
            S.add("partial_last_window_compact_with_exceptions")
        if ((rd.nvalid == WIN) & rd.x_ends & (rd.fmt >= C1)).any():
            S.add("exception_at_0_and_4095")
        if ((rd.xt == rd.nvalid) & (rd.nvalid == WIN)).any():
            S.add("window_of_exceptions_only")

    def missing(self):
        return [c for c in required_cases() if c not in self.seen]
