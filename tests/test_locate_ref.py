"""CPU tests of the suffix-array model (tests/locate_ref.py) against brute force that never looks at the BWT, and of the five entry
points of the sampled suffix array exported by librb2hip.so.  No GPU needed."""
import numpy as np
import pytest

import helpers as H
import locate_ref as LR
import query_ref as Q


def string_sets():
    """small sets with duplicates, empty strings, strings of length 1, one and both strands (input order: string k = the k-th inserted)"""
    a = H.repetitive_reads(90, seed=5, max_len=30)                  # lengths 0 .. 30, duplicates, a few N
    assert any(len(r) == 0 for r in a) and any(len(r) == 1 for r in a)
    b = [np.array(r, np.uint8) for r in ([1], [1], [], [2, 2, 2, 2], [2, 2, 2], [1, 2, 1, 2, 1, 2, 1], [], [4], [1, 2, 1, 2, 1, 2, 1], [5, 5, 1])]
    return {"repetitive": (a, False), "repetitive-both": (a[:50], True), "tiny": (b, False), "tiny-both": (b, True)}


def build(reads, rev, so=0):
    o = H.Oracle(so)
    half = len(reads) // 2
    for part in (reads[:half], reads[half:]):                       # two batches: the second one's strings get the later ids
        o.insert_multi(H.encode_batch(part, True, rev))
    fm = Q.FM(o.bwt())
    o.close()
    return fm, Q.inserted_strings(reads, True, rev)


def patterns(strings, rng, k=150):
    """substrings, random patterns, both with a trailing `$`, the empty pattern and `$` alone: some hundreds"""
    pats = []
    for _ in range(k):
        s = strings[rng.randint(len(strings))]
        if len(s) == 0:
            continue
        a = rng.randint(len(s))
        pats.append(s[a:rng.randint(a, len(s)) + 1].copy())
    pats += [rng.randint(1, 6, size=rng.randint(1, 6)).astype(np.uint8) for _ in range(60)]
    pats += [np.concatenate([p, [0]]).astype(np.uint8) for p in pats[::3]]
    pats += [np.zeros(0, np.uint8), np.zeros(1, np.uint8)]
    return pats


def model_places(fm, pat, max_hits=1 << 40):
    lo, hi, m = fm.backward_search(pat)
    if m != len(pat):
        return set(), 0
    hits, cnt = LR.locate(fm, lo, hi, max_hits)
    return set(map(tuple, hits.tolist())), cnt


@pytest.mark.parametrize("name", ["repetitive", "repetitive-both", "tiny", "tiny-both"])
def test_model_against_brute_force(name):
    reads, rev = string_sets()[name]
    fm, strings = build(reads, rev)
    sid, pos, lens = LR.suffix_array(fm)
    assert lens.tolist() == [len(s) for s in strings]
    # every (string, position) with 0 <= position <= len occurs exactly once
    want = sorted((k, i) for k, s in enumerate(strings) for i in range(len(s) + 1))
    assert sorted(zip(sid.tolist(), pos.tolist())) == want
    assert sid[:len(strings)].tolist() == list(range(len(strings))) and pos[:len(strings)].tolist() == lens.tolist()
    pats = patterns(strings, np.random.RandomState(len(strings)))
    assert len(pats) > 200
    found = 0
    for p in pats:
        got, cnt = model_places(fm, p)
        assert got == LR.brute_places(strings, p), p.tolist()
        assert cnt == len(got)                                      # the rows of an interval are distinct places
        found += bool(got)
    assert found > 100


def test_sorted_order_ids_are_rows_of_the_dollar_block():
    """RLO: string ids are ranks in reverse-lexicographic order, not input positions; the places are those of the sorted strings"""
    reads, rev = string_sets()["repetitive"]
    fm, strings = build(reads, rev, so=1)
    ordered = sorted((np.asarray(s, np.uint8) for s in strings), key=lambda s: s[::-1].tobytes())
    sid, pos, lens = LR.suffix_array(fm)
    assert lens.tolist() == [len(s) for s in ordered]
    for p in patterns(strings, np.random.RandomState(2), k=60):
        got, _ = model_places(fm, p)
        key = lambda places, ss: sorted((ss[k].tobytes(), i) for k, i in places)
        assert key(got, ordered) == key(LR.brute_places(ordered, p), ordered), p.tolist()


def test_truncation_and_malformed_intervals():
    reads, rev = string_sets()["tiny-both"]
    fm, strings = build(reads, rev)
    sid, pos, _ = LR.suffix_array(fm)
    h, c = LR.locate(fm, 3, 9, 4)
    assert c == 6 and h.tolist() == [[sid[x], pos[x]] for x in range(3, 7)]
    assert LR.locate(fm, 5, 5, 4)[1] == 0 and LR.locate(fm, fm.N, fm.N, 1)[1] == 0
    for lo, hi in ((-1, 2), (0, fm.N + 1), (5, 4)):
        h, c = LR.locate(fm, lo, hi, 4)
        assert c == -1 and len(h) == 0
    stored, hit, cnt = LR.locate_raw(fm, [(0, 3), (-1, 2), (2, 12)], 5)
    assert stored == 8 and cnt.tolist() == [3, -1, 10] and (hit[0, 3:] == 0).all() and (hit[1] == 0).all()


def test_empty_index():
    fm = Q.FM(np.zeros(0, np.uint8))
    sid, pos, lens = LR.suffix_array(fm)
    assert len(sid) == len(pos) == len(lens) == 0
    assert LR.locate(fm, 0, 0, 3)[1] == 0 and LR.locate(fm, 0, 1, 3)[1] == -1


def test_locate_symbols_exported():
    from ropebwt2_amd import build_all, load_hip_lib
    build_all()
    L = load_hip_lib()
    for s in ("rb2_hip_ssa_build", "rb2_hip_ssa_drop", "rb2_hip_ssa_info", "rb2_hip_locate", "rb2_hip_locate_dev"):
        assert hasattr(L, s), s
    from ropebwt2_amd import HipBwt
    for m in ("build_ssa", "drop_ssa", "ssa_info", "locate_raw", "locate", "locate_dev", "find"):
        assert callable(getattr(HipBwt, m, None)), m
