"""The identity the lean round rests on ("the lean round"), pinned on the CPU with the per-round model
tests/bcr_rounds_ref.py: in a round in which every interval is empty and every string is a group of its own, the position l a string
carries into the round (piece-relative, on the rope as the round leaves it) IS the final position E[q] + q of its new symbol, so

  * k_part's bisection key E[q] + q is L[q],
  * the place of the new symbol inside its output window, E[q] - i0 + jj in the work order's terms, is l & 4095
    (windows are 4096-aligned inside a piece), and its window is l >> 12.

The model runs in input order.  For the sorted orders the batch is handed to it sorted the way the order sorts it (RLO: the stored,
reversed strings in lexicographic order, the sentinel smallest; RCLO: the same with A <-> T, C <-> G): the BWT of a sorted order on an empty
index is the BWT of the sorted batch in input order -- the test checks that against the oracle before it relies on it -- and from the round in
which the symbols consumed so far tell all running strings apart, a string of the sorted order sits alone in its group at the row the model
has it at.  The identity is asserted in exactly those rounds (on an empty index every interval of a sorted batch is empty).
"""
import numpy as np
import pytest

import helpers as H
import bcr_rounds_ref as M

WIN = M.WIN


def mixed_lengths():
    """the recipe of tests/test_steady_round_gpu.py: strings that end at different rounds"""
    rng = np.random.RandomState(23)
    return [rng.randint(1, 5, size=5 + i % 36).astype(np.uint8) for i in range(1500)]


JOBS = {
    "1500x24": lambda: H.encode_batch_fixed(H.splitmix_bases(1500, 24)),
    "mixed": lambda: H.encode_batch(mixed_lengths()),
}


def sort_batch(buf, so):
    """the batch with its strings in the order `so` gives them, and the stored strings (sentinel included) as sort keys"""
    starts, lens = M.split_batch(buf)
    strs = [buf[s:s + n + 1] for s, n in zip(starts, lens)]

    def key(s):
        s = s.astype(np.int64)
        if so == 2:
            s = np.where((s >= 1) & (s <= 4), 5 - s, s)
        return tuple(s)
    keys = [key(s) for s in strs]
    order = sorted(range(len(strs)), key=lambda i: keys[i])        # (stable: equal strings keep the input order)
    return np.concatenate([strs[i] for i in order]), [keys[i] for i in order]


def one_member_groups(keys, r):
    """round r: do the r symbols consumed so far tell all strings that still run apart?"""
    alive = [k[:r] for k in keys if len(k) > r]
    return len(set(alive)) == len(alive)


@pytest.mark.parametrize("so", [1, 2])
@pytest.mark.parametrize("job", sorted(JOBS))
def test_final_position_is_l(job, so):
    buf, keys = sort_batch(JOBS[job](), so)
    model = M.RoundsModel()
    steady = 0
    for rd in model.rounds(buf):
        if not one_member_groups(keys, rd.r):
            assert steady == 0 or job == "mixed", "one-member groups stay one-member groups while no string ends"
            continue
        steady += 1
        f = np.flatnonzero(rd.isnew)                               # final positions of the round's inserts on the whole array, ascending = by slot
        piece = np.searchsorted(rd.start, f, side="right") - 1
        l = f - rd.start[piece]                                    # what the string carries: its row in its piece as the round leaves it
        first = np.concatenate([[0], np.cumsum(rd.ins)])[piece]    # slots of the pieces in front
        q = np.arange(len(f)) - first                              # slot inside the piece's insert list
        e = (f - np.arange(len(f))) - rd.old_start[piece]          # where it goes on the piece as it was
        assert np.array_equal(e + q, l), "final position E[q] + q is l"
        # per output window: the work order of k_part (i0 = 4096 j - inserts in front, ni) against l alone
        wbase = np.concatenate([[0], np.cumsum(np.bincount(rd.piece, minlength=M.NR))])
        w = wbase[piece] + (l >> 12)                               # the window l names
        assert (rd.piece[w] == piece).all() and (rd.j[w] == l >> 12).all()
        q0 = rd.j[w] * WIN - rd.i0[w]                              # first slot of the window
        jj = q - q0
        assert (jj >= 0).all() and (jj < rd.ni[w]).all(), "the window l >> 12 holds the insert"
        assert np.array_equal(e - rd.i0[w] + jj, l & (WIN - 1)), "place in the window: E - i0 + jj == l & 4095"
        for b in np.unique(rd.piece):                              # k_part: the smallest q with L[q] >= 4096 j is the window's first slot
            lb = l[piece == b]
            sel = rd.piece == b
            assert np.array_equal(np.searchsorted(lb, rd.j[sel] * WIN, side="left"), rd.j[sel] * WIN - rd.i0[sel])
    assert steady >= 5, "the job reaches rounds of one-member groups"
    # the model of the sorted batch is the BWT of the sorted order
    o = H.Oracle(so)
    o.insert_multi(JOBS[job]())
    want = np.concatenate([o.rope(b) for b in range(6)])
    o.close()
    assert np.array_equal(model.bwt, want)
