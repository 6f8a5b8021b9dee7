"""CPU tests of the two references of rb2_hip_graph_clean (tests/graph_clean_ref.py): the model against brute force on random small lists,
the two pinned inputs -- the plain tile of unitig_ref with planted tips and with planted bubbles -- whose counts test_graph_clean_gpu.py
asserts too, the mirror symmetry, and the repeat tile, which cleaning must leave alone.  No GPU needed."""
import numpy as np
import pytest

import graph_clean_ref as GC
import unitig_ref as U

# name: (n_tip, n_bub, seed, strings, edges, chains, canonical unitigs before, rounds, tip rows, bubble rows)
PINNED = {"tips": (3, 0, 1, 162, 160, 14, 7, 2, 6, 0),
          "bubbles": (0, 3, 2, 162, 164, 18, 9, 2, 2, 8)}
_made = {}


def pinned(name):
    """(genome, strings, edges (m, 4) int64) of a pinned input, computed once"""
    if name not in _made:
        g, reads, _ = U.tile_case("plain")
        strings = GC.error_reads(reads, *PINNED[name][:3])
        edges = np.array(U.brute_edges(strings, U.MIN_OVLP, U.MAX_EXT), np.int64).reshape(-1, 4)
        edges.setflags(write=False)
        _made[name] = (g, strings, edges)
    return _made[name]


def random_list(r):
    """(n_str, edges): a few paths and cycles over at most 40 vertices, extra rows between them, duplicates, self loops and invalid rows"""
    n = int(r.randint(1, 41))
    rows, order, i = [], r.permutation(n), 0
    while i < n:
        k = int(r.randint(1, 9))
        c = order[i:i + k].tolist()
        rows += [(a, b) for a, b in zip(c, c[1:])]
        if r.randint(5) == 0:
            rows.append((c[-1], c[0]))                              # a cycle (of one: a self loop)
        i += k
    for _ in range(int(r.randint(0, 9))):
        rows.append((int(r.randint(n)), int(r.randint(n))))
    for _ in range(int(r.randint(0, 3))):
        rows.append(rows[r.randint(len(rows))] if rows else (0, 0))
    rows = [(a, b, int(r.randint(20, 60)), int(r.randint(1, 30))) for a, b in rows]
    if r.randint(2):                                                # symmetric under v <-> v ^ 1, where the ids allow it
        rows += [(b ^ 1, a ^ 1, l, e) for a, b, l, e in rows if (a ^ 1) < n and (b ^ 1) < n]
    for _ in range(int(r.randint(0, 4))):
        bad = [(-1, 0, 30, 5), (0, n, 30, 5), (0, 0, 30, 0), (n + 3, -2, 30, -1)][r.randint(4)]
        rows.insert(int(r.randint(len(rows) + 1)), bad)
    rows = [rows[k] for k in r.permutation(len(rows))]
    return n, np.array(rows, np.int64).reshape(-1, 4)


@pytest.mark.parametrize("seed", range(8))
def test_model_equals_brute_force_on_random_lists(seed):
    r = np.random.RandomState(1000 + seed)
    removed = 0
    for _ in range(400):
        n, edges = random_list(r)
        kw = dict(max_tip_reads=int(r.randint(0, 4)), max_bubble_reads=int(r.randint(0, 5)), pairs=int(r.randint(2)), max_rounds=int(r.randint(1, 5)))
        out, info = GC.clean(n, edges, **kw)
        rows, rounds, tips, bubbles, ignored = GC.brute_clean(n, edges, **kw)
        assert [tuple(x) for x in out.tolist()] == rows, (n, edges.tolist(), kw)
        assert info.tolist()[:6] == [len(rows), len(rows), rounds, tips, bubbles, ignored], (n, edges.tolist(), kw)
        assert info[6] == U.chains(n, out)[1][0] and info[7] == 0
        removed += tips + bubbles
    assert removed > 100, "the random lists hold too few tips and bubbles to test anything"


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_inputs_assemble_to_the_genome(name):
    g, strings, edges = pinned(name)
    _, _, _, n_str, m, n_chains, n_unitigs, rounds, tips, bubbles = PINNED[name]
    vtx, cinfo = U.chains(len(strings), edges)
    before = U.unitigs_of(strings, vtx, True, 1)
    assert (len(strings), len(edges), int(cinfo[0]), len(before)) == (n_str, m, n_chains, n_unitigs)
    if name == "tips":
        assert max(len(t) for t, _, _ in before) == 275
    out, info = GC.clean(len(strings), edges)
    assert info.tolist() == [154, 154, rounds, tips, bubbles, 0, info[6], 0]
    rows, b_rounds, b_tips, b_bubbles, _ = GC.brute_clean(len(strings), edges)
    assert [tuple(x) for x in out.tolist()] == rows and (b_rounds, b_tips, b_bubbles) == (rounds, tips, bubbles)
    after = U.unitigs_of(strings, U.chains(len(strings), out)[0], True, 3)
    assert len(after) == 1 and len(after[0][1]) == 78
    assert after[0][0] == np.asarray(g, np.uint8).tobytes()


def _mirror(rows):
    return sorted((d ^ 1, s ^ 1) for s, d in rows)


@pytest.mark.parametrize("name", sorted(PINNED))
def test_mirror_symmetry_is_kept_after_every_round(name):
    _, strings, edges = pinned(name)
    pairs = lambda a: sorted((s, d) for s, d, _, _ in a.tolist())
    assert pairs(edges) == _mirror(pairs(edges))
    for rounds in (1, 2):
        out, _ = GC.clean(len(strings), edges, max_rounds=rounds)
        assert pairs(out) == _mirror(pairs(out)), rounds
    n, bb = GC.backbone(60, tips=[(10, 1), (20, 2), (30, -2), (40, 3)], bubbles=[(5, 1, 1), (15, 1, 2), (45, 2, 1)])
    for rounds in (1, 2, 3):
        out, info = GC.clean(n, bb, max_rounds=rounds)
        assert pairs(out) == _mirror(pairs(out)), rounds
        assert info[3] + info[4] > 0


def test_repeat_tile_keeps_its_five_unitigs():
    _, _, strings = U.tile_case("repeat")
    edges = np.array(U.brute_edges(strings, U.MIN_OVLP, U.MAX_EXT), np.int64).reshape(-1, 4)
    out, info = GC.clean(len(strings), edges)
    assert np.array_equal(out, edges) and info.tolist()[:6] == [len(edges), len(edges), 1, 0, 0, 0]
    got = U.unitigs_of(strings, U.chains(len(strings), out)[0], True, 1)
    assert [(len(v), len(t)) for t, v, _ in got] == U.TILES["repeat"][4]
