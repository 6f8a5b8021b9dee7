"""CPU tests of the SMEM query: the numpy model (tests/smem_ref.py) against brute-force counting on the oracle's BWT, and the entry
points exported by librb2hip.so and by the HipBwt class.  No GPU needed."""
import numpy as np
import pytest

import query_ref as Q
import smem_ref as S
from test_query_ref import _build


def _queries(strings, rng, k=40):
    qs = []
    pick = lambda: strings[rng.randint(len(strings))]
    while len(qs) < k:
        kind = len(qs) % 4
        if kind == 0:                                               # a substring
            s = pick(); a = rng.randint(len(s) + 1)
            q = s[a:a + rng.randint(0, 31)].copy()
        elif kind == 1:                                             # two substrings of different strings glued together
            q = np.concatenate([pick()[:rng.randint(1, 16)], pick()[-rng.randint(1, 16):]]).astype(np.uint8)
        elif kind == 2:                                             # a string with a substituted base and an N
            q = pick().copy()
            if len(q):
                q[rng.randint(len(q))] = rng.randint(1, 5)
                q[rng.randint(len(q))] = 5 if rng.rand() < 0.5 else q[0]
        else:
            q = rng.randint(1, 5, size=rng.randint(1, 31)).astype(np.uint8)
        qs.append(np.asarray(q[:30], np.uint8))
    return qs


class _Brute:
    """occ(s, e) counted in the strings themselves, for every pair (s, e): the strings joined with their 0 terminators and searched
    for the bytes of q[s:e) (which hold no 0, so no hit spans two strings).  Q.brute_count gives the same numbers and is asked for a
    sample of the pairs of every query; asking it for all of them would take minutes."""
    def __init__(self, strings):
        self.strings = strings
        self.text = b"".join(np.asarray(s, np.uint8).tobytes() + b"\0" for s in strings)

    def count(self, pat):
        pat = np.asarray(pat, np.uint8).tobytes()
        n, at = 0, self.text.find(pat)
        while at >= 0:
            n += 1
            at = self.text.find(pat, at + 1)
        return n

    def smems(self, q, min_len, min_occ, rng=None):
        """(start, end, occurrences) from the definition"""
        L = len(q)
        occ = {(s, e): 0 if (q[s:e] == 5).any() else self.count(q[s:e]) for s in range(L) for e in range(s + 1, L + 1)}
        if rng is not None and occ:
            keys = sorted(occ)
            for k in rng.choice(len(keys), size=min(4, len(keys)), replace=False):
                s, e = keys[k]
                assert occ[s, e] == (0 if (q[s:e] == 5).any() else Q.brute_count(self.strings, q[s:e])), (q.tolist(), s, e)
        es = []
        for s in range(L):
            ok = [e for e in range(s + 1, L + 1) if occ[s, e] >= min_occ]
            es.append(max(ok) if ok else s)
        assert all(a <= b for a, b in zip(es, es[1:])), "e(s) must be non-decreasing"
        return [(s, e, occ[s, e]) for s, e in enumerate(es) if e > s and (s == 0 or es[s - 1] < e) and e - s >= min_len]


@pytest.mark.parametrize("so", [0, 1, 2])
def test_model_against_brute_force(so):
    fm, strings = _build(so, True, seed=70 + so)
    rng = np.random.RandomState(so)
    brute = _Brute(strings)
    found = 0
    for q in _queries(strings, rng):
        for min_occ in (1, 3):
            for min_len in (1, 8):
                got = S.smems(fm, q, min_len, min_occ)
                assert np.array_equal(got, S.smems_from_table(fm, q, S.occ_table(fm, q), min_len, min_occ))
                want = brute.smems(q, min_len, min_occ, rng if (min_occ, min_len) == (1, 1) else None)
                assert [tuple(r) for r in got[:, [0, 1, 4]].tolist()] == want, (q.tolist(), min_len, min_occ)
                found += len(want)
                for s, e, x0, x1, size in got.tolist():
                    lo, hi, m = fm.backward_search(q[s:e])
                    rlo, rhi, rm = fm.backward_search(Q.revcomp(q[s:e]))
                    assert m == rm == e - s and (x0, x1, size) == (lo, rlo, hi - lo) and rhi - rlo == size
                    ik = fm.sym_interval(int(q[s]))                 # the same bi-interval by forward extensions from the first symbol
                    for c in q[s + 1:e]:
                        ik = fm.extend(ik, False)[Q.COMP[int(c)]].tolist()
                    assert ik == [x0, x1, size]
                    ik = fm.sym_interval(int(q[e - 1]))             # and by backward extensions from the last
                    for c in q[s:e - 1][::-1]:
                        ik = fm.extend(ik, True)[int(c)].tolist()
                    assert ik == [x0, x1, size]
    assert found > 100


def test_model_edge_cases():
    fm, strings = _build(0, True, seed=75)
    assert S.smems(fm, [], 1, 1).shape == (0, 5)
    assert S.smems(fm, [5, 5, 5], 1, 1).shape == (0, 5)
    assert S.smems(fm, [1, 0, 2], 1, 1) is None and S.smems(fm, [7], 1, 1) is None and S.smems(fm, [0], 1, 1) is None
    s = next(x for x in strings if len(x) >= 12 and not (x == 5).any())
    got = S.smems(fm, s, 1, 1)
    assert got[:, :2].tolist() == [[0, len(s)]]                     # a whole string is its own single SMEM
    q = np.concatenate([s[:6], [5], s[6:]]).astype(np.uint8)        # an N splits it; no match spans the N
    got = S.smems(fm, q, 1, 1)
    assert len(got) >= 2 and all(e <= 6 or b >= 7 for b, e in got[:, :2].tolist())
    assert (np.diff(got[:, 0]) > 0).all() and (np.diff(got[:, 1]) > 0).all()
    assert len(S.smems(fm, q, len(q), 1)) == 0


def test_smem_symbols_exported():
    from ropebwt2_amd import build_all, load_hip_lib
    build_all()
    L = load_hip_lib()
    for s in ("rb2_hip_smem", "rb2_hip_smem_dev"):
        assert hasattr(L, s), s


def test_smem_methods_exist():
    from ropebwt2_amd import HipBwt
    for m in ("smem", "smem_raw", "smem_dev"):
        assert hasattr(HipBwt, m), m
