"""CPU tests of the unitig model (tests/unitig_ref.py: chains, texts) against the brute force that takes its edges from string slices and
glues slices (brute_unitigs), on the two tile inputs -- whose counts are pinned here, so that the inputs cannot drift into a case that
tests nothing --, a circular genome, and the small string sets of the other query tests.  No GPU needed."""
import functools

import numpy as np
import pytest

import unitig_ref as U
from query_ref import inserted_strings, revcomp
from test_locate_ref import string_sets


@functools.lru_cache(maxsize=None)
def tile(name, circular=False):
    """(genome, strings, edges as an (m, 4) array, the brute-force unitigs, canonical and all) of a tile input, computed once"""
    g, _, strings = U.tile_case(name, circular)
    edges = np.array(U.brute_edges(strings, U.MIN_OVLP, U.MAX_EXT), np.int64).reshape(-1, 4)
    return g, strings, edges, U.brute_unitigs(strings, U.MIN_OVLP, U.MAX_EXT), U.brute_unitigs(strings, U.MIN_OVLP, U.MAX_EXT, canonical=False)


@pytest.mark.parametrize("name", sorted(U.TILES))
def test_tile_inputs_give_the_pinned_counts(name):
    _, n_strings, n_edges, n_chains, canon = U.TILES[name]
    g, strings, edges, brute, brute_all = tile(name)
    assert len(strings) == n_strings and len(edges) == n_edges
    vtx, info = U.chains(len(strings), edges)
    assert info.tolist()[:2] == [n_chains, 0] and info[3] == 0 and len(brute_all) == n_chains
    assert [(len(p), len(t)) for t, p, _ in brute] == canon
    both = (g.tobytes(), revcomp(g).tobytes())
    assert all(t in both[0] or t in both[1] for t, _, _ in brute_all)          # every unitig is a piece of the genome or of its reverse complement
    if name == "plain":
        assert brute[0][0] == both[0]


@pytest.mark.parametrize("name", sorted(U.TILES))
def test_model_against_brute_force_on_the_tiles(name):
    _, strings, edges, brute, brute_all = tile(name)
    vtx, info = U.chains(len(strings), edges)
    assert U.unitigs_of(strings, vtx) == brute and U.unitigs_of(strings, vtx, canonical=False) == brute_all
    for k in (2, 5):
        assert U.unitigs_of(strings, vtx, min_reads=k) == [r for r in brute if len(r[1]) >= k]
    urec, txt, inf = U.texts(strings, vtx, canonical=True)
    assert inf.tolist() == [len(brute), sum(len(t) for t, _, _ in brute), 0] and np.array_equal(urec[:, 2], np.cumsum(urec[:, 3]) - urec[:, 3])
    assert info[2] == max(len(p) for _, p, _ in brute_all)


def test_circular_genome():
    """reads that run on round the end of the genome: two circular chains, one per strand, cut at their smallest ids"""
    _, strings, edges, brute, brute_all = tile("plain", True)
    vtx, info = U.chains(len(strings), edges)
    assert info.tolist() == [2, 2, len(strings) // 2, 0]
    assert [(p[0], c) for _, p, c in brute_all] == [(0, True), (1, True)] and len(brute) == 1
    assert U.unitigs_of(strings, vtx) == brute and U.unitigs_of(strings, vtx, canonical=False) == brute_all
    h = vtx[0]
    assert h.tolist()[:3] == [0, 0, 0] and h[3] >= 1                             # the closing link: in ext_in of the head, in no rank and no off
    assert len(brute[0][0]) == len(strings[0]) + vtx[vtx[:, 0] == 0, 2].max()


@pytest.mark.parametrize("name", ["repetitive-both", "tiny-both"])
@pytest.mark.parametrize("min_ovlp", [3, 8])
def test_model_against_brute_force_on_the_string_sets(name, min_ovlp):
    reads, rev = string_sets()[name]
    strings = inserted_strings(reads, True, rev)
    edges = np.array(U.brute_edges(strings, min_ovlp), np.int64).reshape(-1, 4)
    vtx, info = U.chains(len(strings), edges)
    for canonical in (False, True):
        for k in (1, 2):
            assert U.unitigs_of(strings, vtx, canonical, k) == U.brute_unitigs(strings, min_ovlp, canonical=canonical, min_reads=k), (name, min_ovlp, canonical, k)
    assert info[0] == len(U.brute_unitigs(strings, min_ovlp, canonical=False)) and (name == "tiny-both" or len(edges) > 20)


@pytest.mark.parametrize("name,min_ovlp", [("repetitive-both", 3), ("repetitive-both", 8), ("tiny-both", 3), ("tiny-both", 8), ("plain", U.MIN_OVLP), ("repeat", U.MIN_OVLP)])
def test_canonical_keeps_one_of_every_pair(name, min_ovlp):
    """the mirror image of a chain under v <-> v ^ 1: where it is a chain too the rule keeps exactly one of the two, and a chain that is
    its own mirror image once.  The tile graphs are symmetric (u -> v mirrors to v^1 -> u^1), so there every chain has its mirror image;
    the graphs of the small string sets are not quite -- copies, contained reads and N are in them -- and there the pairs that exist count"""
    if name in U.TILES:
        strings, edges = tile(name)[1:3]
        assert {(s ^ 1, d ^ 1, e) for s, d, _, e in edges.tolist()} == {(d, s, len(strings[s]) - len(strings[d]) + e) for s, d, _, e in edges.tolist()}
    else:
        strings = inserted_strings(string_sets()[name][0], True, True)
        edges = np.array(U.brute_edges(strings, min_ovlp), np.int64).reshape(-1, 4)
    vtx, _ = U.chains(len(strings), edges)
    every = {frozenset(p) for _, p, _ in U.unitigs_of(strings, vtx, canonical=False)}
    kept = {frozenset(p) for _, p, _ in U.unitigs_of(strings, vtx, canonical=True)}
    mirror = lambda c: frozenset(v ^ 1 for v in c)
    assert kept <= every and all(min(c) % 2 == 0 for c in kept)
    pairs = [c for c in every if mirror(c) in every]
    assert len(pairs) == len(every) if name in U.TILES else len(pairs) >= 2
    for c in pairs:
        assert ((c in kept) + (mirror(c) in kept) == 1) if mirror(c) != c else (c in kept), sorted(c)


def test_made_up_graphs():
    """the degrees decide: duplicates, self loops, merges, forks, a tail into a cycle, ignored edges"""
    E = lambda rows: np.array(rows, np.int64).reshape(-1, 4)
    vtx, info = U.chains(4, E([[0, 1, 9, 2], [1, 2, 9, 3], [2, 3, 9, 4]]))
    assert vtx.tolist() == [[0, 0, 0, -1], [0, 1, 2, 2], [0, 2, 5, 3], [0, 3, 9, 4]] and info.tolist() == [1, 0, 4, 0]
    vtx, info = U.chains(3, E([[0, 1, 9, 2], [1, 2, 9, 3], [2, 0, 9, 4]]))
    assert vtx.tolist() == [[0, 0, 0, 4], [0, 1, 2, 2], [0, 2, 5, 3]] and info.tolist() == [1, 1, 3, 0]
    vtx, info = U.chains(2, E([[1, 1, 9, 5], [0, 0, 9, 0], [-1, 0, 9, 1], [0, 2, 9, 1]]))
    assert vtx.tolist() == [[0, 0, 0, -1], [1, 0, 0, 5]] and info.tolist() == [2, 1, 1, 3]
    vtx, info = U.chains(2, E([[0, 1, 9, 1], [0, 1, 9, 1]]))
    assert vtx[:, 0].tolist() == [0, 1] and info.tolist() == [2, 0, 1, 0]
    vtx, info = U.chains(4, E([[3, 1, 9, 1], [1, 2, 9, 1], [2, 0, 9, 1], [0, 1, 9, 1]]))       # a tail 3 -> 1 into the cycle 1 2 0: it opens at 1
    assert vtx.tolist() == [[1, 2, 2, 1], [1, 0, 0, -1], [1, 1, 1, 1], [3, 0, 0, -1]] and info.tolist() == [2, 0, 3, 0]
    assert U.chains(0, E([]))[1].tolist() == [0, 0, 0, 0] and U.chains(0, E([[0, 0, 1, 1]]))[1].tolist() == [0, 0, 0, 1]


def test_short_pieces_and_damaged_rows():
    """an ext larger than its read gives zeros in front of the piece and flag bit 1; a row whose head is no vertex is a chain of its own"""
    strings = [np.array(s, np.uint8) for s in ([1, 2, 3, 4], [3, 4, 1], [4, 1, 2, 2], [2, 2])]
    vtx, _ = U.chains(4, np.array([[0, 1, 2, 1], [1, 2, 2, 5], [2, 3, 2, 1]], np.int64))
    urec, txt, inf = U.texts(strings, vtx)
    assert urec.tolist() == [[0, 4, 0, 11, 2]] and txt.tolist() == [1, 2, 3, 4, 1, 0, 4, 1, 2, 2, 2] and inf.tolist() == [1, 11, 1]
    vtx[3, 0] = 99
    urec, txt, inf = U.texts(strings, vtx)
    assert urec.tolist() == [[0, 3, 0, 10, 2], [3, 1, 10, 2, 2]] and txt.tolist() == [1, 2, 3, 4, 1, 0, 4, 1, 2, 2, 2, 2] and inf.tolist() == [2, 12, 2]
