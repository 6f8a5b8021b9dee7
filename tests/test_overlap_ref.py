"""CPU tests of the overlap model (tests/overlap_ref.py) against brute force over string slices that never looks at a BWT, and of the four
entry points of the overlap queries exported by librb2hip.so.  No GPU needed."""
import numpy as np
import pytest

import overlap_ref as OR
import query_ref as Q
from test_locate_ref import build, string_sets

NAMES = ["repetitive", "repetitive-both", "tiny", "tiny-both"]
HITS = {"tiny": 59, "tiny-both": 139}                                # (query, length, string) hits at min_ovlp 1 and 3 together; the others: > 3000


def queries(strings, rng):
    """(the N-free strings; more: with an N inside, mutated, longer than any string)"""
    plain = [np.asarray(s, np.uint8) for s in strings if len(s) and not (np.asarray(s) == 5).any()]
    more = []
    for s in plain[::3]:
        if len(s) >= 3:
            t = s.copy(); t[rng.randint(1, len(s) - 1)] = 5         # an N inside: the suffixes behind it still overlap
            more.append(t)
            t = s.copy(); t[rng.randint(0, len(s))] = 1 + (t[0] % 4)  # (may leave the string as it was)
            more.append(t)
    longest = max(plain, key=len)
    more += [np.concatenate([rng.randint(1, 5, size=7).astype(np.uint8), longest]), np.concatenate([longest, longest]),
             np.array([5], np.uint8), np.array([1, 5], np.uint8), np.zeros(0, np.uint8)]
    more += [s for s in strings if len(s) and (np.asarray(s) == 5).any()][:5]
    return plain, more


@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_model_against_brute_force(name, so):
    reads, rev = string_sets()[name]
    fm, inserted = build(reads, rev, so)
    n = int(fm.C[1])
    strings = inserted if so == 0 else [fm.walk(k) for k in range(n)]   # sorted orders: string k is row k of the $ block
    assert sorted(s.tobytes() for s in strings) == sorted(np.asarray(s, np.uint8).tobytes() for s in inserted)
    hd = OR.head(fm)
    assert sorted(hd.tolist()) == list(range(n))
    plain, more = queries(strings, np.random.RandomState(len(strings)))
    hits = multi = 0
    for i, q in enumerate(plain + more):
        own = i < len(plain)                                        # a string of the index
        longer = len(q) + 1
        for min_ovlp in (1, 3, longer):
            got = OR.overlaps(fm, q, min_ovlp)
            assert got == OR.brute_overlaps(strings, q, min_ovlp), (q.tolist(), min_ovlp)
            assert min_ovlp < longer or not got
            if min_ovlp < longer and own:
                hits += len(got)
                multi += min_ovlp == 1 and len({l for _, l in got}) > 1
        if own:                                                     # it finds itself at its full length
            assert any(np.array_equal(strings[k], q) for k, l in OR.overlaps(fm, q, 1) if l == len(q))
    print("%s so=%d: %d queries, %d hits, %d queries with more than one length" % (name, so, 2 * len(plain), hits, multi))
    if name in HITS:
        assert hits == HITS[name]
    else:
        assert hits > 3000 and 2 * multi > len(plain)
    # the queries in step (what the GPU tests compare with) against the definition, suffix by suffix; truncated too
    qs = plain + more
    for min_ovlp in (1, 3, 50):
        for max_recs in (1, 2, 64):
            stored, rec, cnt = OR.overlap_raw(fm, qs, min_ovlp, max_recs)
            cut = 0
            for i, q in enumerate(qs):
                r, c = OR.overlap(fm, q, min_ovlp, max_recs)
                assert c == cnt[i] and np.array_equal(rec[i, :len(r)], r) and (rec[i, len(r):] == 0).all(), (q.tolist(), min_ovlp, max_recs)
                cut += c > max_recs
            assert stored == int(np.minimum(cnt, max_recs).sum())
            assert min_ovlp == 50 or max_recs == 64 or cut > 0      # something was truncated
            assert max_recs < 64 or cut == 0


def test_truncation_keeps_the_shortest():
    reads, rev = string_sets()["tiny"]
    fm, strings = build(reads, rev)
    q = np.array([1, 2, 1, 2, 1, 2, 1], np.uint8)                   # overlaps at 1, 3, 5 and 7
    full, c = OR.overlap(fm, q, 1)
    assert c == 4 and full[:, 0].tolist() == [1, 3, 5, 7] and (full[:, 2] - full[:, 1]).tolist() == [4, 2, 2, 2]
    for max_recs in (1, 2):
        r, c = OR.overlap(fm, q, 1, max_recs)
        assert c == 4 and np.array_equal(r, full[:max_recs])
    r, c = OR.overlap(fm, q, 3, 1)
    assert c == 3 and r[:, 0].tolist() == [3]
    assert OR.overlap(fm, q, 8)[1] == 0


def test_malformed_queries_and_ranges():
    reads, rev = string_sets()["tiny-both"]
    fm, strings = build(reads, rev)
    n = int(fm.C[1])
    qs = [np.array(q, np.uint8) for q in ([1, 0], [0], [1, 6, 2], [2, 2], [7], [])]
    stored, rec, cnt = OR.overlap_raw(fm, qs, 1, 3)
    assert cnt.tolist() == [-1, -1, -1, 2, -1, 0] and stored == 2
    assert (rec[[0, 1, 2, 4, 5]] == 0).all() and (rec[3, 2] == 0).all() and rec[3, :2, 0].tolist() == [1, 2]
    for i, q in enumerate(qs):
        assert OR.overlap(fm, q, 1)[1] == cnt[i] and OR.malformed(q) == (cnt[i] < 0)
    hd = OR.head(fm)
    stored, ids, cnt = OR.string_ids_raw(fm, [(0, 3), (-1, 2), (2, 12), (0, n + 1), (5, 4), (n, n), (0, n)], 5)
    assert cnt.tolist() == [3, -1, 10, -1, -1, 0, n] and stored == 3 + 5 + 5
    assert ids[0].tolist() == hd[:3].tolist() + [0, 0] and ids[2].tolist() == hd[2:7].tolist() and (ids[[1, 3, 4, 5]] == 0).all()
    assert OR.string_ids(fm, 0, n, n)[0].tolist() == hd.tolist()


def test_empty_index():
    fm = Q.FM(np.zeros(0, np.uint8))
    assert len(OR.head(fm)) == 0
    stored, rec, cnt = OR.overlap_raw(fm, [np.array([1, 2], np.uint8), np.zeros(0, np.uint8), np.array([0], np.uint8)], 1, 2)
    assert stored == 0 and cnt.tolist() == [0, 0, -1] and (rec == 0).all()
    assert OR.overlap(fm, [1, 2], 1)[1] == 0 and OR.overlaps(fm, [1, 2], 1) == set()
    assert OR.string_ids(fm, 0, 0, 3)[1] == 0 and OR.string_ids(fm, 0, 1, 3)[1] == -1
    assert OR.overlap_raw(fm, [], 1, 2)[0] == 0


def test_overlap_symbols_exported():
    from ropebwt2_amd import build_all, load_hip_lib
    build_all()
    L = load_hip_lib()
    for s in ("rb2_hip_overlap", "rb2_hip_overlap_dev", "rb2_hip_string_ids", "rb2_hip_string_ids_dev"):
        assert hasattr(L, s), s
    from ropebwt2_amd import HipBwt
    for m in ("overlap_raw", "overlap_dev", "string_ids_raw", "string_ids_dev", "overlaps"):
        assert callable(getattr(HipBwt, m, None)), m
