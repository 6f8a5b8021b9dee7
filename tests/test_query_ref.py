"""CPU tests of the FM-index query side: the numpy reference (tests/query_ref.py) against brute force on the oracle's BWT, and the
four query entry points exported by librb2hip.so.  No GPU needed."""
import numpy as np
import pytest

import helpers as H
import query_ref as Q


def _build(so, rev, seed):
    reads = H.repetitive_reads(120, seed=seed, max_len=30)
    reads2 = H.repetitive_reads(60, seed=seed + 100, max_len=30)
    o = H.Oracle(so)
    o.insert_multi(H.encode_batch(reads, True, rev))
    o.insert_multi(H.encode_batch(reads2, True, rev))
    strings = Q.inserted_strings(reads, True, rev) + Q.inserted_strings(reads2, True, rev)
    fm = Q.FM(o.bwt())
    o.close()
    return fm, strings


def _patterns(strings, rng, k=60):
    pats = []
    for _ in range(k):
        s = strings[rng.randint(len(strings))]
        if len(s) == 0:
            continue
        a = rng.randint(len(s))
        b = rng.randint(a, len(s) + 1)
        pats.append(s[a:b])
    pats += [rng.randint(1, 6, size=rng.randint(1, 8)).astype(np.uint8) for _ in range(30)]
    return pats


@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("rev", [False, True])
def test_reference_against_brute_force(so, rev):
    fm, strings = _build(so, rev, seed=11 + so)
    assert fm.N == sum(len(s) + 1 for s in strings)
    assert fm.C[1] == len(strings)
    rng = np.random.RandomState(so * 2 + rev)
    for p in _patterns(strings, rng):
        assert fm.count(p) == Q.brute_count(strings, p), p
        pd = np.concatenate([p, [0]]).astype(np.uint8)               # P$: strings that end in P
        assert fm.count(pd) == sum(1 for s in strings if len(s) >= len(p) and np.array_equal(s[len(s) - len(p):], p)), p
    assert fm.backward_search([]) == (0, fm.N, 0)
    assert fm.backward_search([0, 1])[0] == -1 and fm.backward_search([6])[2] == -1
    # m: the longest suffix that occurs
    lo, hi, m = fm.backward_search([5, 5, 5, 5, 5, 5, 5, 1, 2])
    assert fm.count([5, 5, 5, 5, 5, 5, 5, 1, 2][9 - m:]) == hi - lo > 0
    # LF walks from the $ block give back every string; in input order row k is string k
    walked = [fm.walk(r) for r in range(fm.C[1])]
    if so == 0:
        for k, s in enumerate(strings):
            assert np.array_equal(walked[k], s), k
    else:
        key = lambda a: a.tobytes()
        assert sorted(map(key, walked)) == sorted(map(key, (np.asarray(s, np.uint8) for s in strings)))
    if so == 1:                                                     # RLO: the strings come out in reverse-lexicographic order
        rk = [s[::-1].tobytes() for s in walked]
        assert rk == sorted(rk)


@pytest.mark.parametrize("so", [0, 1, 2])
def test_reference_extend_bi_intervals(so):
    """with both strands, chains of backward and forward extensions keep x[0] = lo(Q), x[1] = lo(revcomp Q), x[2] = count(Q)"""
    fm, strings = _build(so, True, seed=40 + so)
    rng = np.random.RandomState(so)
    checked = 0
    for _ in range(40):
        s = strings[rng.randint(len(strings))]
        if len(s) < 2 or (s == 5).any():
            continue
        a = rng.randint(len(s))
        q = s[a:a + 1].copy()
        ik = fm.sym_interval(int(q[0]))
        b = a + 1
        while True:
            back = rng.rand() < 0.5
            if back and a > 0:
                a -= 1; c = int(s[a]); ok = fm.extend(ik, True); q = s[a:b]
                ik = ok[c].tolist()
            elif b < len(s):
                c = int(s[b]); b += 1; ok = fm.extend(ik, False); q = s[a:b]
                ik = ok[Q.COMP[c]].tolist()                         # forward extension by a is indexed by the complement of a
            else:
                break
            lo, hi, m = fm.backward_search(q)
            rlo, rhi, rm = fm.backward_search(Q.revcomp(q))
            assert m == len(q) and rm == len(q)
            assert ik == [lo, rlo, hi - lo], (q, ik)
            checked += 1
    assert checked > 20


@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("rev", [False, True])
def test_vectorised_helpers_match_the_scalar_ones(so, rev):
    """extend_many against extend, walk_all against walk; walk_all reads every row of the BWT exactly once"""
    fm, strings = _build(so, rev, seed=70 + so)
    rng = np.random.RandomState(so * 2 + rev)
    iks = np.array([[x, rng.randint(0, fm.N + 1), 1] for x in range(fm.N)] + [[fm.N, fm.N, 0], [0, 0, fm.N], [0, 3, 0]], np.int64)
    wide = np.stack([rng.randint(0, fm.N + 1, size=300), rng.randint(0, fm.N + 1, size=300), np.zeros(300, np.int64)], 1)
    wide[:, 2] = [rng.randint(0, fm.N - x + 1) for x in wide[:, 0]]
    wide[:, [0, 1]] = np.where((np.arange(300) % 2 == 0)[:, None], wide[:, [0, 1]], wide[:, [1, 0]])   # (so x[1] + x[2] <= N as well, half the time)
    iks = np.concatenate([iks, wide, [[-3, 2, 5], [fm.N - 1, 0, 4], [2, fm.N + 2, 1]]])                 # out of range: clipped as extend clips
    for is_back in (0, 1):
        got = fm.extend_many(iks, is_back)
        assert got.shape == (len(iks), 6, 3) and got.dtype == np.int64
        want = np.stack([fm.extend(ik, is_back) for ik in iks])
        assert np.array_equal(got, want), np.flatnonzero((got != want).reshape(len(iks), -1).any(1))[:5]
    assert fm.extend_many(np.zeros((0, 3), np.int64), 1).shape == (0, 6, 3)
    walked, visits = fm.walk_all()
    assert len(walked) == fm.C[1] == len(strings)
    for r, w in enumerate(walked):
        assert w.dtype == np.uint8 and np.array_equal(w, fm.walk(r)), r
    assert visits.shape == (fm.N,) and (visits == 1).all(), np.flatnonzero(visits != 1)[:5]
    assert any(len(w) == 0 for w in walked) and max(len(w) for w in walked) == max(len(s) for s in strings)


def test_walk_all_on_the_empty_index():
    fm = Q.FM(np.zeros(0, np.uint8))
    walked, visits = fm.walk_all()
    assert walked == [] and len(visits) == 0
    fm = Q.FM(np.zeros(3, np.uint8))                                # three empty strings
    walked, visits = fm.walk_all()
    assert [len(w) for w in walked] == [0, 0, 0] and visits.tolist() == [1, 1, 1]


def test_query_symbols_exported():
    from ropebwt2_amd import build_all, load_hip_lib
    build_all()
    L = load_hip_lib()
    for s in ("rb2_hip_backward_search", "rb2_hip_backward_search_dev", "rb2_hip_extend", "rb2_hip_extract"):
        assert hasattr(L, s), s


def test_pattern_encoding():
    from ropebwt2_amd.hipbwt import encode_pattern, pack_patterns
    assert encode_pattern("ACgtN$").tolist() == [1, 2, 3, 4, 5, 0]
    assert encode_pattern(b"").tolist() == []
    with pytest.raises(ValueError):
        encode_pattern("ACX")
    pat, off = pack_patterns(["AC", "", np.array([4, 0], np.uint8)])
    assert off.tolist() == [0, 2, 2, 4] and pat.tolist() == [1, 2, 4, 0]
