"""CPU tests of the references of the approximate search (tests/approx_ref.py): the backtracking model over an FM-index against the
brute force over the windows of the strings, the piece bound D against the true minimum of substitutions, and the packing of the
substitutions.  No GPU needed."""
import itertools

import numpy as np
import pytest

import approx_ref as AR
import query_ref as Q
from test_locate_ref import build, string_sets


def queries(strings, rng, k=70):
    """substrings with 0 .. 4 planted substitutions or N, at the ends too; random words; the whole of a string; the empty query"""
    out = []
    pool = [s for s in strings if len(s) >= 1]
    for _ in range(k):
        s = pool[rng.randint(len(pool))]
        a = rng.randint(len(s))
        q = s[a:rng.randint(a, min(len(s), a + 12)) + 1].copy()
        for _ in range(rng.randint(0, 5)):
            at = [0, len(q) - 1, rng.randint(len(q))][rng.randint(3)]
            q[at] = 5 if rng.rand() < 0.2 else 1 + (q[at] + rng.randint(3)) % 4 if q[at] < 5 else rng.randint(1, 5)
        out.append(q)
    out += [rng.randint(1, 6, size=rng.randint(1, 7)).astype(np.uint8) for _ in range(20)]
    out += [max(strings, key=len).copy(), np.zeros(0, np.uint8), np.array([5], np.uint8), np.array([5, 5], np.uint8)]
    return out


@pytest.mark.parametrize("name", ["repetitive", "repetitive-both", "tiny", "tiny-both"])
def test_model_equals_brute_force(name):
    reads, rev = string_sets()[name]
    fm, strings = build(reads, rev)
    rng = np.random.RandomState(len(strings))
    qs = queries(strings, rng)
    memo, total, cut = {}, 0, 0
    for q in qs:
        for max_mm, min_occ in ((0, 1), (1, 1), (2, 2), (3, 1), (4, 1), (4, 3)):
            want = AR.brute(strings, q, max_mm, min_occ, fm=fm, memo=memo)
            got = AR.model(fm, q, max_mm, min_occ)
            assert got == want, (q.tolist(), max_mm, min_occ, got[:3], want[:3])
            assert len(set(got)) == len(got)
            total += len(got)
            cut += min_occ > 1 and len(got) < len(AR.model(fm, q, max_mm, 1))
            if max_mm == 0 and len(q) and not (q == 5).any():       # no substitution: the backward search itself
                lo, hi, m = fm.backward_search(q)
                assert got == ([(lo, hi, 0, 0)] if m == len(q) else [])
            for lo, hi, n_mm, subs in got:                          # the record spells the match
                S = q.copy()
                for p, c in AR.unpack_subs(subs):
                    assert S[p] != c
                    S[p] = c
                assert len(AR.unpack_subs(subs)) == n_mm <= max_mm and fm.backward_search(S) == (lo, hi, len(q))
    assert total > 1000 and cut > 0, (total, cut)
    assert AR.model(fm, [1, 0, 2], 1) is None and AR.brute(strings, [6], 1) is None and AR.model(fm, [1] * 8193, 0) is None
    assert AR.model(fm, [], 2) == [] and AR.brute(strings, [], 2) == []


def _min_subs(words, q):
    """the fewest substitutions that turn q into one of the words, None when there is no word"""
    return min((int((w != q).sum()) for w in words), default=None)


@pytest.mark.parametrize("name", ["tiny", "tiny-both", "repetitive"])
def test_bound_never_exceeds_the_true_minimum(name):
    """D[p] <= the fewest substitutions of any match of q[0 .. p], for every prefix, every min_occ: exhaustively over all queries of up to
    five symbols out of A C G T N, and over queries cut from the strings"""
    reads, rev = string_sets()[name]
    fm, strings = build(reads, rev)
    memo = {}

    def count(w):
        return fm.count(np.array(w, np.uint8)) if len(w) else fm.N

    rng = np.random.RandomState(1)
    qs = [np.array(t, np.uint8) for L in range(1, 6) for t in itertools.product((1, 2, 3, 4, 5), repeat=L)]
    if name == "repetitive":
        qs = qs[::7] + [q for q in queries(strings, rng, 60) if 0 < len(q) <= 12]
    tight = positive = 0
    for min_occ in (1, 2):
        for q in qs:
            D, pieces = AR.bound(count, q, min_occ)
            assert all(s <= t for s, t in pieces) and all(a[0] > b[1] for a, b in zip(pieces, pieces[1:])), pieces      # disjoint, right to left
            assert all(D[p] <= D[p + 1] for p in range(len(q) - 1))
            for p in range(len(q)):
                L = p + 1
                if L not in memo:
                    memo[L] = AR.windows(strings, L)
                words = [np.frombuffer(w, np.uint8) for w, c in memo[L].items() if c >= min_occ]
                best = _min_subs(words, q[:L])
                if best is not None:
                    assert D[p] <= best, (q.tolist(), p, min_occ, D, best)
                    tight += D[p] == best
                    positive += D[p] > 0
    assert tight > 100 and positive > 100, (tight, positive)


def test_packing_round_trips():
    rng = np.random.RandomState(4)
    assert AR.pack_subs([]) == 0 and AR.unpack_subs(0) == []
    assert AR.pack_subs([(0, 1)]) == 1 and AR.pack_subs([(8191, 4), (0, 3)]) == (8191 << 3 | 4) | 3 << 16
    for _ in range(500):
        k = rng.randint(0, 5)
        subs = sorted(zip(rng.choice(8192, size=k, replace=False).tolist(), rng.randint(1, 5, size=k).tolist()), reverse=True)
        v = AR.pack_subs(subs[::-1])
        assert 0 <= v < 1 << 64 and AR.unpack_subs(v) == subs
        assert all(v >> (16 * j) & 0xFFFF for j in range(k)) and v >> (16 * k) == 0
    # the helpers of the package agree (they are what HipBwt.approx decodes with); importing them needs no GPU
    from ropebwt2_amd.hipbwt import pack_subs, unpack_subs
    for subs in ([], [(0, 1)], [(5, 2), (3, 4)], [(8191, 4), (100, 1), (7, 3), (0, 2)]):
        assert pack_subs(subs) == AR.pack_subs(subs) and unpack_subs(pack_subs(subs)) == subs
    with pytest.raises(ValueError):
        pack_subs([(1, 1)] * 2)
