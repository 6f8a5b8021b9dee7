"""CPU tests of the irreducible-overlap model (tests/irreducible_ref.py: the arithmetic of k_irreducible over query_ref.FM) against brute
force over string slices that never looks at a BWT.  The model names the strings revcomp(T) of the neighbours T: the edges are compared as
(text of the neighbour, l, ext) with the model's ids reverse-complemented, which is the test of that claim.  No GPU needed."""
import numpy as np
import pytest

import helpers as H
import irreducible_ref as IR
import overlap_ref as OR
import query_ref as Q
from test_locate_ref import build, string_sets
from test_overlap_ref import queries

PARAMS = [(mo, me) for mo in (1, 3, 8) for me in (1, 4, 1000)]


def _strings(fm, inserted, so):
    return inserted if so == 0 else [fm.walk(k) for k in range(int(fm.C[1]))]   # sorted orders: string k is row k of the $ block


def _brute_texts(strings, q, min_ovlp, max_ext):
    return sorted((np.asarray(strings[k], np.uint8).tobytes(), l, e) for k, l, e in IR.brute_irreducible(strings, q, min_ovlp, max_ext))


def _model_texts(fm, strings, q, min_ovlp, max_ext):
    recs, cnt, steps = IR.irreducible(fm, q, min_ovlp, max_ext)
    assert cnt == len(recs) == len({(l, e, zlo) for l, e, zlo, _ in recs})
    return sorted((Q.revcomp(strings[s]).tobytes(), l, e) for s, l, e in IR.edges_of(fm, recs)), recs


@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("name", ["repetitive-both", "tiny-both"])
def test_model_against_brute_force(name, so):
    reads, rev = string_sets()[name]
    fm, inserted = build(reads, rev, so)
    strings = _strings(fm, inserted, so)
    own = [np.asarray(s, np.uint8) for s in strings if len(s)]      # every non-empty string of the index is a query
    plain, more = queries(strings, np.random.RandomState(len(strings)))
    edges = multi = reduced = 0
    for i, q in enumerate(own + more):
        for min_ovlp, max_ext in PARAMS:
            want = _brute_texts(strings, q, min_ovlp, max_ext)
            got, recs = _model_texts(fm, strings, q, min_ovlp, max_ext)
            assert got == want, (q.tolist(), min_ovlp, max_ext)
            assert len(got) == sum(zhi - zlo for _, _, zlo, zhi in recs)          # exactly zhi - zlo strings T per record
            if i < len(own):                                         # counted as distinct (text, l, ext): copies of a string are one edge
                ov = {(k, l) for k, l in OR.brute_overlaps(strings, q, min_ovlp) if l < len(q)}
                edges += len(set(want))
                multi += len(set(want)) > 1
                reduced += len(ov) > len(want)                      # the reduction removes at least one overlap
    print("%s so=%d: %d queries, %d edges, %d cases with several edges, %d reduced" % (name, so, len(own) + len(more), edges, multi, reduced))
    if name == "repetitive-both":                                    # not vacuous
        assert edges > 2000 and multi > 250 and reduced > 600


@pytest.mark.parametrize("name", ["repetitive", "tiny"])
def test_one_strand_merely_returns(name):
    reads, rev = string_sets()[name]
    fm, strings = build(reads, rev)
    n = int(fm.C[1])
    for q in [np.asarray(s, np.uint8) for s in strings if len(s)][:40]:
        for min_ovlp, max_ext in ((1, 4), (3, 1000)):
            recs, cnt, steps = IR.irreducible(fm, q, min_ovlp, max_ext)
            assert cnt == len(recs) and all(0 <= zlo < zhi <= n and 1 <= e <= max_ext and min_ovlp <= l < len(q) for l, e, zlo, zhi in recs)


def test_malformed_empty_and_raw():
    reads, rev = string_sets()["tiny-both"]
    fm, strings = build(reads, rev)
    qs = [np.array(q, np.uint8) for q in ([1, 0], [0], [1, 6, 2], [1, 2, 1, 2, 1], [7], [], [1] * 8193, [5], [2, 5])]
    stored, rec, cnt = IR.irreducible_raw(fm, qs, 1, 4, 1 << 16, 3)
    assert cnt.tolist() == [-1, -1, -1, cnt[3], -1, 0, -1, 0, 0] and cnt[3] >= 1 and stored == min(cnt[3], 3)
    assert (rec[[0, 1, 2, 4, 5, 6, 7, 8]] == 0).all() and (rec[3, :stored, 1] >= 1).all()
    for i, q in enumerate(qs):
        assert IR.malformed(q) == (cnt[i] == -1) and (IR.brute_irreducible(strings, q, 1, 4) is None) == (cnt[i] == -1)
    fm0 = Q.FM(np.zeros(0, np.uint8))
    stored, rec, cnt = IR.irreducible_raw(fm0, [np.array([1, 2], np.uint8), np.zeros(0, np.uint8), np.array([0], np.uint8)], 1, 4)
    assert stored == 0 and cnt.tolist() == [0, 0, -1] and (rec == 0).all()
    assert IR.irreducible_raw(fm0, [], 1, 4)[0] == 0


def test_step_budget_sweep():
    """at steps - 1 the count is <= -2 and the records are a subset of the full answer; at steps the query is complete"""
    reads, rev = string_sets()["repetitive-both"]
    fm, strings = build(reads, rev)
    cut = 0
    for q in [np.asarray(s, np.uint8) for s in strings if len(s) >= 3][::5]:
        full, cnt, steps = IR.irreducible(fm, q, 2, 6)
        assert cnt == len(full) and steps >= 1
        assert IR.irreducible(fm, q, 2, 6, steps) == (full, cnt, steps)
        for ms in sorted({1, steps // 2, steps - 1} - {0}):
            if ms >= steps:
                continue
            part, c, st = IR.irreducible(fm, q, 2, 6, ms)
            assert c <= -2 and st == ms and -2 - c == len(part) and part == full[:len(part)]
            cut += len(part) > 0
    assert cut > 10


def test_hand_made_chain():
    """reads of 20 symbols at every second position of a random genome of 80, both strands, input order: at min_ovlp = 10 every read but
    the last has exactly the edge to its successor (l = 18, ext = 2), though it overlaps the four reads behind that one too"""
    reads = IR.chain_reads(IR.CHAIN_SEED)
    assert len(reads) == 31
    strings = Q.inserted_strings(reads, True, True)
    for i in range(len(reads)):
        want = {(2 * (i + 1), 18, 2)} if i + 1 < len(reads) else set()
        assert IR.brute_irreducible(strings, reads[i], 10, 1000) == want, i
        want = {(2 * (i - 1) + 1, 18, 2)} if i > 0 else set()         # the other strand runs the other way
        assert IR.brute_irreducible(strings, strings[2 * i + 1], 10, 1000) == want, i
    o = H.Oracle(0)
    o.insert_multi(H.encode_batch(reads, True, True))
    fm = Q.FM(o.bwt())
    o.close()
    for i in range(len(reads) - 1):
        recs, cnt, _ = IR.irreducible(fm, reads[i], 10, 1000)
        assert cnt == 1 and IR.edges_of(fm, recs) == {(2 * (i + 1) + 1, 18, 2)}   # the id of revcomp(T): id ^ 1 is the neighbour
        assert len(IR._candidates(strings, reads[i], 10, 1000)) == min(5, len(reads) - 1 - i)
