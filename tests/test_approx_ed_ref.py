"""CPU tests of the references of the approximate search with insertions and deletions (tests/approx_ed_ref.py): the trie model over an
FM-index against the brute force over the windows of the strings, both against the plain statement of the distance, and against the
references of the search by substitutions (tests/approx_ref.py) for the two identities of include/rb2_hip.h.  No GPU needed."""
import numpy as np
import pytest

import approx_ed_ref as ER
import approx_ref as AR
from test_locate_ref import build, string_sets


def edit(rng, q, kind, at):
    """q with one edit at position `at`: 's' another symbol there, 'd' the symbol deleted, 'i' a symbol inserted in front of it"""
    q = np.asarray(q, np.uint8)
    if kind == "s":
        t = q.copy()
        t[at] = 1 + (t[at] + rng.randint(3)) % 4 if t[at] < 5 else rng.randint(1, 5)
        return t
    if kind == "d":
        return np.delete(q, at)
    return np.insert(q, at, rng.randint(1, 5)).astype(np.uint8)


def queries(strings, rng, k=40):
    """substrings with 0 .. 3 planted edits of every kind or an N, at the ends too; random words; the whole of a string; the empty query"""
    out = []
    pool = [s for s in strings if len(s) >= 2]
    for _ in range(k):
        s = pool[rng.randint(len(pool))]
        a = rng.randint(len(s) - 1)
        q = s[a:rng.randint(a + 1, min(len(s), a + 12)) + 1].copy()
        for _ in range(rng.randint(0, 4)):
            if len(q) < 2:
                break
            at = [0, len(q) - 1, rng.randint(len(q))][rng.randint(3)]
            if rng.rand() < 0.15:
                q[at] = 5
            else:
                q = edit(rng, q, "sdi"[rng.randint(3)], at)
        out.append(q)
    out += [rng.randint(1, 6, size=rng.randint(1, 7)).astype(np.uint8) for _ in range(12)]
    out += [max(strings, key=len).copy(), np.zeros(0, np.uint8), np.array([5], np.uint8), np.array([5, 5], np.uint8), np.array([2], np.uint8)]
    return out


def test_distance_of_the_definition():
    """sub, lev and ed on cases worked by hand, and the vectorised lev of brute() against the plain one"""
    A, C, G, T, N = 1, 2, 3, 4, 5
    assert ER.sub(A, A) == 0 and ER.sub(A, C) == 1 and ER.sub(A, N) == 1 and ER.sub(N, N) == 1
    assert ER.lev([], []) == 0 and ER.lev([A, C], []) == 2 and ER.lev([], [A, N]) == 2            # deleting an N costs 1
    assert ER.lev([A, C, G], [A, G]) == 1 and ER.lev([A, G], [A, C, G]) == 1 and ER.lev([A, C, G], [A, N, G]) == 1
    assert ER.ed([A, C, G, T], [A, C, G, T]) == 0 and ER.ed([A, C, T], [A, C, G, T]) == 1 and ER.ed([A, C, G, G, T], [A, C, G, T]) == 1
    assert ER.ed([C, G, T], [A, C, G, T]) == 2                       # the first symbols are aligned: C against A, then one deletion
    assert ER.ed([A], [A]) == 0 and ER.ed([C], [A]) == 1 and ER.ed([A], [N]) == 1
    assert ER.ed([A], [A, A]) == ER.INF and ER.ed([A, A], [A]) == ER.INF and ER.ed([A, A], [A, A]) == 0 and ER.ed([A, C, A], [A, A]) == 1
    rng = np.random.RandomState(3)
    for _ in range(60):
        n, m = rng.randint(0, 9), rng.randint(0, 9)
        W = rng.randint(1, 5, size=(5, n)).astype(np.uint8)
        Y = rng.randint(1, 6, size=m).astype(np.uint8)
        assert ER._lev_many(W, Y).tolist() == [ER.lev(w, Y) for w in W]


@pytest.mark.parametrize("name", ["repetitive", "repetitive-both", "tiny", "tiny-both"])
def test_model_equals_brute_force(name):
    reads, rev = string_sets()[name]
    fm, strings = build(reads, rev)
    rng = np.random.RandomState(len(strings))
    qs = queries(strings, rng)
    memo, total, cut, other = {}, 0, 0, 0
    for q in qs:
        for max_ed, min_occ in ((0, 1), (1, 1), (2, 2), (3, 1), (4, 3)) if len(q) <= 8 else ((0, 1), (1, 1), (2, 2)):
            want = ER.brute(strings, q, max_ed, min_occ, fm=fm, memo=memo)
            got = ER.model(fm, q, max_ed, min_occ)
            assert got == want, (q.tolist(), max_ed, min_occ, got[:3], want[:3])
            assert len(set(got)) == len(got) == len({(r[0], r[1], r[3]) for r in got})
            total += len(got)
            other += sum(r[3] != len(q) for r in got)
            cut += min_occ > 1 and len(got) < len(ER.model(fm, q, max_ed, 1))
            assert all(len(q) - max_ed <= r[3] <= len(q) + max_ed and r[2] <= max_ed and r[1] - r[0] >= min_occ for r in got)
            # identity 1: no edit = the backward search itself
            if max_ed == 0 and len(q):
                lo, hi, m = fm.backward_search(q)
                assert got == ([(lo, hi, 0, len(q))] if m == len(q) and not (q == 5).any() else [])
            # identity 2: every match by substitutions alone is a match here, with no more edits and the same length
            here = {(r[0], r[1], r[3]): r[2] for r in got}             # (a word and a longer one can share an interval: the length tells them apart)
            for lo, hi, n_mm, _ in AR.model(fm, q, max_ed, min_occ):
                assert here.get((lo, hi, len(q)), 9) <= n_mm
    assert total > 1000 and cut > 0 and other > 100, (total, cut, other)
    assert ER.model(fm, [1, 0, 2], 1) is None and ER.brute(strings, [6], 1) is None and ER.model(fm, [1] * 8193, 0) is None
    assert ER.model(fm, [], 2) == [] and ER.brute(strings, [], 2) == []


def test_records_spell_words_at_the_stated_distance():
    """every record of the model is a word of len symbols whose distance to the query, by the plain dynamic programme, is ed"""
    reads, rev = string_sets()["repetitive"]
    fm, strings = build(reads, rev)
    rng = np.random.RandomState(7)
    seen = 0
    for q in queries(strings, rng, 15):
        words = {}
        for n in range(max(1, len(q) - 2), len(q) + 3):
            for w in AR.windows(strings, n):
                S = np.frombuffer(w, np.uint8)
                words[fm.backward_search(S)[:2] + (n,)] = S
        for lo, hi, e, n in ER.model(fm, q, 2):
            S = words[(lo, hi, n)]
            assert len(S) == n and ER.ed(S, q) == e
            seen += 1
    assert seen > 100
