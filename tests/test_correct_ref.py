"""CPU tests of the correction model (tests/correct_ref.py): the incremental rule over a BWT equals the naive restatement over the windows
of the strings, which never looks at a BWT, budget cases included; on a coverage fixture the model restores every read with one planted
substitution and changes no clean read; with pairs the output of correct_into is closed under reverse complement.  No GPU needed."""
import numpy as np
import pytest

import correct_ref as CR
import helpers as H
import query_ref as Q
from test_locate_ref import build, string_sets


def _reads(strings, rng, n=8):
    """reads the rule has something to do on: strings of the set as they are, with one or two substitutions, with an N"""
    out = [np.zeros(0, np.uint8)]
    for i in range(n):
        s = strings[rng.randint(len(strings))].copy()
        for _ in range(i % 3):
            if len(s):
                s[rng.randint(len(s))] = rng.randint(1, 5)
        if i % 4 == 3 and len(s):
            s[rng.randint(len(s))] = 5
        out.append(s)
    return out


@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("name", ["repetitive", "repetitive-both", "tiny", "tiny-both"])
def test_model_against_brute_force(name, so):
    """k in {1, 2, 5, 12, L, L + 1}, min_occ 1 .. 3, max_fix 1 and 8; then budgets around the clean windows and around the probes the
    read needs.  Over all sets some budget ends in the profile, some in the alternatives and some in a re-evaluation (asserted below)"""
    reads, rev = string_sets()[name]
    fm, strings = build(reads, rev, so)
    occ = CR.fm_counter(fm)
    tabs = {}
    rng = np.random.RandomState(len(strings) + so)
    runs = fixed = 0
    where = []
    for q in _reads(strings, rng):
        L = len(q)
        for k in sorted({1, 2, 5, 12, max(L, 1), L + 1}):
            tab = tabs.setdefault(k, CR.window_counts(strings, k))
            for min_occ in (1, 2, 3):
                for max_fix in (1, 8):
                    a = CR.correct_one(occ, q, k, min_occ, max_fix, 1 << 40)
                    b = CR.brute_one(tab, q, k, min_occ, max_fix, 1 << 40)
                    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:] and a[1] >= 0, (name, so, q.tolist(), k, min_occ, max_fix, a, b)
                    assert a[1] <= max_fix and (q != a[0]).sum() <= a[1]
                    runs += 1
                    fixed += a[1] > 0
                    if L < k:
                        assert a[1:] == (0, L, 0) and np.array_equal(a[0], q)
                        continue
                    clean = sum(all(1 <= c <= 4 for c in q[j:j + k]) for j in range(L - k + 1))
                    for mp in sorted({clean - 1, clean, clean + 1, clean + 3, a[3] - 1, a[3], a[3] + 1} - set(range(-9, 1))):
                        c = CR.correct_one(occ, q, k, min_occ, max_fix, mp, where)
                        d = CR.brute_one(tab, q, k, min_occ, max_fix, mp)
                        assert np.array_equal(c[0], d[0]) and c[1:] == d[1:], (name, so, q.tolist(), k, min_occ, max_fix, mp, c, d)
                        assert (c[1] <= -2) == (mp < a[3]) and (c[1] <= -2 or (np.array_equal(c[0], a[0]) and c[1:] == a[1:]))
                        if mp < clean:
                            assert c[1] == -2 and np.array_equal(c[0], q)        # more clean windows than probes: over budget with no fix
    assert runs > 200 and fixed >= 1, (runs, fixed)                 # (every set exercises the path behind a fix)
    _WHERE[(name, so)] = set(where)


_WHERE = {}


def test_budgets_ended_everywhere():
    """(runs behind the test above) the budgets of the sets together ended in every part of the rule"""
    seen = set().union(*_WHERE.values()) if _WHERE else set()
    assert len(_WHERE) == 12 and seen == {"profile", "alternatives", "re-evaluation"}, seen


@pytest.fixture(scope="module")
def cov():
    truth, reads, pos = CR.coverage_fixture()
    o = H.Oracle(0)
    o.insert_multi(H.encode_batch(reads, True, True))
    fm = Q.FM(o.bwt())
    o.close()
    return truth, reads, pos, fm


def test_coverage_fixture_is_restored(cov):
    """every read with one planted substitution comes back as the error-free read, with one fix; no clean read changes.  A condition on
    the fixture (its seed is committed in correct_ref.py), checked on the model alone"""
    truth, reads, pos, fm = cov
    k, L = CR.COV_K, CR.COV_LEN
    assert len(reads) == 600 and (pos >= 0).sum() == 300 and all(len(r) == L for r in reads)
    assert {0, L - 1, k - 1} <= set(pos.tolist()) and fm.N == 2 * 600 * (L + 1)
    texts, cnt, weak, probes = CR.correct_raw(fm, reads, k, CR.COV_MIN_OCC)
    bad = [i for i in range(len(reads)) if not np.array_equal(texts[i], truth[i])]
    assert not bad, (len(bad), bad[:5], pos[bad[:5]].tolist())
    assert np.array_equal(cnt, (pos >= 0).astype(np.int64)) and (weak == 0).all()
    clean = pos < 0
    assert (probes[clean] == L - k + 1).all() and probes[~clean].min() > L - k + 1
    print("probes per read: %.1f on average, %d at most" % (probes.mean(), probes.max()))
    assert probes.max() <= 869                                       # HipBwt.correct's default budget is not met by this fixture
    # the same from the windows of the strings, by the naive restatement, for a part of the reads
    strings = Q.inserted_strings(reads, True, True)
    some = list(range(0, 600, 7))
    t2, c2, w2, p2 = CR.brute_raw(strings, [reads[i] for i in some], k, CR.COV_MIN_OCC)
    assert all(np.array_equal(a, texts[i]) for a, i in zip(t2, some)) and np.array_equal(c2, cnt[some]) and np.array_equal(w2, weak[some]) and np.array_equal(p2, probes[some])


def test_correct_into_with_pairs_is_closed_under_reverse_complement(cov):
    truth, reads, pos, fm = cov
    strings = Q.inserted_strings(reads, True, True)
    out, info, added = CR.correct_into(strings, CR.COV_K, CR.COV_MIN_OCC, pairs=True, fm=fm, budget=1000)
    assert len(out) == len(strings) and added == sum(len(s) + 1 for s in strings)
    for i in range(0, len(out), 2):
        assert np.array_equal(out[i + 1], Q.revcomp(out[i]))
    have = {bytes(bytearray(s)) for s in out}
    assert all(bytes(bytearray(Q.revcomp(s))) in have for s in out)
    assert all(np.array_equal(a, b) for a, b in zip(out[::2], truth))
    assert info[:6].tolist() == [1200, 300, 300, 0, 0, 0] and info[6] == len(CR.batches([41] * 1200, 1000, True)) and info[7] == 24 * 41
    # without pairs every string is corrected on its own: the same strings here, where every read is restored
    out1, info1, _ = CR.correct_into(strings, CR.COV_K, CR.COV_MIN_OCC, fm=fm)
    assert all(np.array_equal(a, b) for a, b in zip(out, out1)) and info1[:8].tolist() == [1200, 600, 600, 0, 0, 0, 1, 1200 * 41]
    # the counts of the strings' own windows give what the index gives
    out2, info2, _ = CR.correct_into(strings[:100], CR.COV_K, 1, pairs=True)
    out3, info3, _ = CR.correct_into(strings[:100], CR.COV_K, 1, pairs=True, fm=None, budget=41)
    assert all(np.array_equal(a, b) for a, b in zip(out2, out3)) and info3[6] == 50 and info3[7] == 82 and info2[6] == 1
    with pytest.raises(AssertionError):
        CR.correct_into(strings[:3], CR.COV_K, 1, pairs=True)
