"""What the window directory ("the window directory") rests on, from the per-round model tests/bcr_rounds_ref.py alone, without
a GPU.  In a LITE round the rank of a new symbol a on the new piece is put together from three parts:

  * the prefix over the superblocks in front of its superblock (k_sbscan*, minus the prefix at the piece's first superblock),
  * the entry of its WINDOW in the directory: the a's of the windows of the same superblock in front of it (k_meta_win, from one record of six
    counts per window that k_merge<.., LITE> left), and
  * RKREL: the a's in front of it INSIDE its window (k_merge<.., LITE>).

The test builds the records, the prefixes and the totals with the kernels' arithmetic -- 16-bit fields, lane = window, eight windows per superblock, the
owner of a superblock taken from the pieces' first superblocks, a window past the piece's last leaf counted as zero WITHOUT being read (its record is
poisoned here) -- and compares the sum, for every symbol every round inserts, with the count on the model's array.  The per-leaf rule of the other
rounds is checked the same way.

A wrong rule must fail: the prefix of the symbol's LEAF (the per-leaf directory) with RKREL taken over the window counts the leaves of the window in
front of the symbol's leaf twice.

The model inserts in input order; the RLO and RCLO cases feed it every batch sorted in that order (tests/test_lean_fork_ref.py).
"""
import numpy as np
import pytest

import bcr_rounds_ref as R
import helpers as H
import test_lean_fork_ref as F

LEAF, SB, WPL, WIN = F.LEAF, F.SB, F.WPL, R.WIN
WSB = SB // WPL                                                      # windows per superblock
POISON = 0xffff


def jobs():
    """[(name, [reads of batch 0, ...])]: rope `$` is one piece that takes one symbol per string in round 0 of a batch, at its end -- so the number of
    strings sets where that piece ends, and the second batch of "sb" inserts into its second superblock"""
    def rnd(n, L, seed):
        return [r for r in H.splitmix_bases(n, L, seed=seed)]
    return [("leaf", [rnd(WIN + LEAF, 5, 21)]),                       # rope `$`: 5 leaves -- ends on a leaf boundary inside its second window
            ("win", [rnd(2 * WIN, 5, 22)]),                           # ... on a window boundary
            ("sb", [rnd(40000, 12, 23), rnd(2 * SB * LEAF - 40000, 12, 24)])]   # ... inside a window, then on a superblock boundary; pieces of more than one superblock


def directory_of_round(rd, new):
    """records, directory entries, totals and prefixes of the round's new side as k_merge<.., LITE>, k_meta_win and the scans write them"""
    size = np.diff(rd.start)
    lay = F.layout_from_sizes(size)
    nsb = lay["nsb_total"]
    cs = np.stack([np.concatenate([[0], np.cumsum(new == s)]) for s in range(6)]).astype(np.int64)   # cs[s][i] = symbols s in front of array position i
    # k_merge<.., LITE>: one record per window at own[gl / WPL], gl = the window's first leaf -- its six counts (<= WIN, 16-bit fields) and its fill
    rec = np.full((nsb * WSB, 6), POISON, np.int64)
    ws = rd.start[rd.piece] + rd.j * WIN
    gw = lay["leaf0"][rd.piece] // WPL + rd.j
    assert len(np.unique(gw)) == len(gw) and (gw < nsb * WSB).all()
    tot = (cs[:, ws + rd.nvalid] - cs[:, ws]).T
    assert tot.max(initial=0) <= WIN and (tot.sum(axis=1) == rd.nvalid).all()
    rec[gw] = tot
    # k_meta_win: lane = window; the superblock's owner is the last piece with sb0 <= sb; a window lies in the piece when its first leaf does
    w = np.arange(nsb * WSB)
    sb, gl = w // WSB, w * WPL
    owner = np.maximum(0, (lay["sb0"][None, :] <= sb[:, None]).sum(axis=1) - 1)
    ok = (gl >= lay["leaf0"][owner]) & (gl < lay["leaf0"][owner] + lay["nleaves"][owner])
    assert ok.sum() == len(gw) and ok[gw].all(), "the windows the merge wrote are the windows the directory reads"
    e = np.where(ok[:, None], rec, 0).reshape(nsb, WSB, 6)
    incl = np.cumsum(e, axis=1)
    assert incl.max(initial=0) <= SB * LEAF < 1 << 16, "a prefix inside a superblock fits its 16-bit field"
    meta = np.where(ok[:, None], (incl - e).reshape(-1, 6), POISON)
    sbtot = incl[:, -1, :] if nsb else np.zeros((0, 6), np.int64)
    sbpre = np.concatenate([np.zeros((1, 6), np.int64), np.cumsum(sbtot, axis=0)])   # SbBase + SbRec: in front of every superblock, pool-wide
    return {"lay": lay, "cs": cs, "meta": meta, "sbtot": sbtot, "sbpre": sbpre}


def ranks_of_round(rd, new, D):
    """for every symbol the round inserted: the model's rank on its piece, and the three sums"""
    lay, cs = D["lay"], D["cs"]
    f = np.flatnonzero(rd.isnew)
    a = new[f].astype(np.int64)
    p = np.searchsorted(rd.start, f, side="right") - 1                # (an empty piece starts where the next one does)
    p0 = rd.start[p]
    pp = f - p0
    lf = pp >> 10
    want = cs[a, f] - cs[a, p0]
    sbpart = D["sbpre"][lay["sb0"][p] + lf // SB, a] - D["sbpre"][lay["sb0"][p], a]
    sb_start = p0 + (pp // (SB * LEAF)) * (SB * LEAF)
    win_start, leaf_start = p0 + (pp >> 12 << 12), p0 + (lf << 10)
    rk_win, rk_leaf = cs[a, f] - cs[a, win_start], cs[a, f] - cs[a, leaf_start]
    assert rk_win.max(initial=0) <= WIN
    dir_win = D["meta"][lay["leaf0"][p] // WPL + (lf >> 2), a]        # the gather of k_advance<.., LITE>
    dir_leaf = cs[a, leaf_start] - cs[a, sb_start]                    # meta[leaf0 + lf] of a per-leaf round
    return {"want": want, "lite": sbpart + dir_win + rk_win, "leaf": sbpart + dir_leaf + rk_leaf, "wrong": sbpart + dir_leaf + rk_win,
            "piece": p, "pp": pp}


@pytest.mark.parametrize("so", [0, 1, 2])
def test_superblock_window_and_in_window_parts_add_up_to_the_rank(so):
    seen = set()
    rounds = symbols = wrong = text = 0
    for name, batches in jobs():
        m = R.RoundsModel()
        for k, reads in enumerate(batches):
            buf = F.sorted_batch(reads, so)
            text += len(buf)
            for rd in m.rounds(buf):
                new = m.bwt
                D = directory_of_round(rd, new)
                q = ranks_of_round(rd, new, D)
                assert np.array_equal(q["lite"], q["want"]), (name, k, rd.r)
                assert np.array_equal(q["leaf"], q["want"]), (name, k, rd.r)
                # the totals are what the per-leaf kernel writes: the symbols of the superblock's leaves that lie in its piece
                lay, cs = D["lay"], D["cs"]
                for pc in np.flatnonzero(np.diff(rd.start) > 0):
                    n, s0, e0 = int(rd.start[pc + 1] - rd.start[pc]), int(rd.start[pc]), int(rd.start[pc + 1])
                    for i in range(-(-n // (SB * LEAF))):
                        lo, hi = s0 + i * SB * LEAF, min(e0, s0 + (i + 1) * SB * LEAF)
                        assert np.array_equal(D["sbtot"][lay["sb0"][pc] + i], cs[:, hi] - cs[:, lo])
                    # the cases: only pieces that take symbols this round count
                    if rd.ins[pc] == 0:
                        continue
                    if n < WIN:
                        seen.add("shorter than a window")
                    if n % LEAF == 0 and n % WIN != 0:
                        seen.add("ends on a leaf boundary inside a window")
                    if n % WIN == 0 and n % (SB * LEAF) != 0:
                        seen.add("ends on a window boundary")
                    if n % (SB * LEAF) == 0:
                        seen.add("ends on a superblock boundary")
                    if -(-n // WIN) % WSB != 0:
                        seen.add("a superblock of fewer than 8 windows")
                    if n > SB * LEAF and (q["pp"][q["piece"] == pc] >= SB * LEAF).any():
                        seen.add("a symbol behind the piece's first superblock")
                bad = q["wrong"] != q["want"]
                wrong += int(bad.sum())
                # the wrong rule is wrong exactly where a symbol's leaf is not the first of its window and leaves in between hold its symbol
                first_leaf = (q["pp"] >> 10) % WPL == 0
                assert not bad[first_leaf].any()
                rounds += 1
                symbols += len(q["want"])
    assert seen == {"shorter than a window", "ends on a leaf boundary inside a window", "ends on a window boundary", "ends on a superblock boundary",
                    "a superblock of fewer than 8 windows", "a symbol behind the piece's first superblock"}, seen
    assert rounds > 30 and symbols == text                           # every symbol of every batch, sentinels included, was looked at once
    assert wrong > symbols // 4, (wrong, symbols)                    # three leaves of four are not the first of their window
