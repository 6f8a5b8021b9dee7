"""CPU test of the identity behind rb2_hip_contained: the walk that carries the interval of its own suffix
(tests/contain_ref.py) gives, on the oracle's BWT, what a brute force over string slices gives -- occurrences, equal strings, one
representative per class -- in all three sorting orders, for one strand and both, on a fixture where every flag and both ends of the walk
(the early exit, the string's own `$`) occur."""
import numpy as np
import pytest

import contain_ref as CR
import query_ref as Q

# strings, rows, the strings with flag 0 .. 4, steps with the early exit, walks it ended, symbols: the same in all three sorting orders
FIGURES = {False: (249, 9482, [129, 26, 88, 2, 4], 6149, 108, 9233), True: (498, 18964, [256, 52, 177, 5, 8], 12434, 214, 18466)}


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("so", [0, 1, 2])
def test_model_equals_brute_force(so, rev):
    _, bwt = CR.mixed(so, rev)
    fm = Q.FM(bwt)
    n = int(fm.C[1])
    strings, _ = fm.walk_all()
    want = CR.brute(strings)

    def invariant(row, lo, ahi, hi):
        assert ((lo <= row) & (row < ahi) & (ahi <= hi)).all()

    full = CR.contained(fm, early=False, check=invariant)
    info = {}
    rec = CR.contained(fm, check=invariant, info=info)
    lens = np.array([len(s) for s in strings])
    assert np.array_equal(full[:, 4], lens)
    live = lens > 0
    assert np.array_equal(full[live, 1:3], want[live]) and (full[~live] == [4, 0, 0, 0, 0]).all()
    assert np.array_equal(full[live, 0], (full[live, 3] > 0) + 2 * (want[live, 0] > want[live, 1]))
    # the early exit changes nothing but the steps, and only where the answer is "unique"
    assert np.array_equal(rec[:, 0], full[:, 0]) and (rec[:, 4] <= full[:, 4]).all()
    short = rec[:, 4] < full[:, 4]
    assert (full[short, :4] == [0, 1, 1, 0]).all() and np.array_equal(rec[:, :4], full[:, :4])
    assert ((rec[:, 4] == lens) | (rec[:, 0] == 0)).all()
    # every flag occurs, the early exit and the full walk are both exercised
    hist = np.bincount(rec[:, 0], minlength=5)
    assert (hist >= 2).all(), hist
    assert short.sum() <= info["early"] and n / 4 < short.sum() and info["early"] < n / 2, (short.sum(), info, n)
    assert (n, fm.N, hist.tolist(), int(rec[:, 4].sum()), info["early"], int(lens.sum())) == FIGURES[rev]
    # one rank-0 string per class; the ranks of a class are 0 .. n_equal - 1 in row order
    keys = [s.tobytes() for s in strings]
    classes = {}
    for k in np.flatnonzero(live):
        classes.setdefault(keys[k], []).append(k)
    for ks in classes.values():
        assert full[ks, 3].tolist() == list(range(len(ks))), ks      # (rank grows with the row, and with it the id)
        assert (full[ks, 2] == len(ks)).all()
    # after removing the flagged strings every survivor occurs once
    keep = [strings[k] for k in np.flatnonzero(rec[:, 0] == 0)]
    assert len(keep) == hist[0] and (CR.brute(keep) == [1, 1]).all()


def test_input_order_keeps_the_lowest_id():
    """in input order string k is the k-th inserted, so the representative of every class is the first read with that text"""
    for rev in (False, True):
        _, bwt = CR.mixed(0, rev)
        fm = Q.FM(bwt)
        want = Q.inserted_strings(CR.mixed_reads(), True, rev)
        strings, _ = fm.walk_all()
        assert [s.tobytes() for s in strings] == [np.asarray(s, np.uint8).tobytes() for s in want]
        rec = CR.contained(fm)
        seen = set()
        for k, s in enumerate(strings):
            if len(s):
                assert (rec[k, 3] == 0) == (s.tobytes() not in seen), k
                seen.add(s.tobytes())


def test_subsets_and_bad_ids():
    _, bwt = CR.mixed(0, False)
    fm = Q.FM(bwt)
    n = int(fm.C[1])
    full = CR.contained(fm)
    ids = np.array([5, -1, n, 5, 0, n - 1, 17])
    rec = CR.contained(fm, ids)
    assert (rec[[1, 2]] == [-1, 0, 0, 0, 0]).all() and np.array_equal(rec[[0, 3, 4, 5, 6]], full[[5, 5, 0, n - 1, 17]])


def test_walks_end_on_any_loaded_index():
    """LF is one-to-one on any six streams with consistent totals (what load_ropes accepts) and no row maps into the `$` block, so the
    walk from a string id can enter no cycle: it ends at a `$` within N steps whatever the streams hold, and flag -2 stays a guard.  The
    answers on such an index mean nothing, but they are defined: the GPU test compares them with this model"""
    _, bwt = CR.mixed(0, False)
    for seed in range(3):
        fm = Q.FM(CR.shuffled_ropes(bwt, seed))
        for early in (True, False):
            rec = CR.contained(fm, early=early)
            assert (rec[:, 0] >= 0).all() and rec[:, 4].sum() <= fm.N - int(fm.C[1])
    assert not np.array_equal(CR.contained(Q.FM(CR.shuffled_ropes(bwt, 0))), CR.contained(Q.FM(bwt)))
