"""GPU tests of tip and bubble removal (include/rb2_hip.h: rb2_hip_graph_clean[_dev]; kernels in csrc/rb2_clean.h) and of
HipBwt.graph_clean / assemble(clean=...).  The rows kept and info are deterministic by definition, so everything is compared exactly with
the model (tests/graph_clean_ref.py, which tests/test_graph_clean_ref.py holds against brute force), through the host and the device
entry.  The lists are made up where the point is the graph -- the class of every kind of chain, and the sizes at which a kernel can go
wrong: more rows and more vertices than a block of the scan holds, a chain far longer than a wave with more heads in a wave than the
gathering takes, a vertex with more out-rows than a wave has lanes -- and come from reads with planted errors where the point is the
assembly."""
import os
import subprocess
import sys

import numpy as np
import pytest

import graph_clean_ref as GC
import helpers as H
import unitig_ref as U
from test_graph_clean_ref import PINNED, pinned

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILL = -7                                                            # what the calls must leave where they store nothing
DEFAULTS = dict(max_tip_reads=2, max_bubble_reads=3, pairs=1, max_rounds=8)
CLEAN = dict(max_tip_reads=2, max_bubble_reads=3, pairs=True, max_rounds=8)


def path(*vs, ext=5):
    return [(a, b, 30, ext) for a, b in zip(vs, vs[1:])]


def line(a, b):
    return path(*range(a, b))


@pytest.fixture(scope="module")
def g(hip):
    g = hip.HipBwt(0)
    yield g
    g.close()


def clean_dev(g, n, edges, cap, null=False, **kw):
    """graph_clean_dev on an out buffer of cap + 2 rows filled with FILL: (m', info, the whole buffer as the device left it).  The rows
    of the input must be what they were"""
    edges = np.ascontiguousarray(edges, np.int64).reshape(-1, 4)
    rows = np.full((cap + 2, 4), FILL, np.int64)
    d_e, d_o = g.dev_alloc(max(edges.nbytes, 8)), g.dev_alloc(rows.nbytes)
    try:
        if edges.nbytes:
            g.L.rb2_hip_memcpy(g.h, d_e, edges.ctypes.data, edges.nbytes, 0)
        g.L.rb2_hip_memcpy(g.h, d_o, rows.ctypes.data, rows.nbytes, 0)
        kept, info = g.graph_clean_dev(n, len(edges), d_e if len(edges) else None, None if null else d_o, cap, **dict(DEFAULTS, **kw))
        g.sync()
        back = np.zeros_like(edges)
        if edges.nbytes:
            g.L.rb2_hip_memcpy(g.h, back.ctypes.data, d_e, edges.nbytes, 1)
        g.L.rb2_hip_memcpy(g.h, rows.ctypes.data, d_o, rows.nbytes, 1)
    finally:
        g.dev_free(d_e)
        g.dev_free(d_o)
    assert np.array_equal(back, edges), "the input rows were written"
    assert kept == info[0] and info[1] == min(kept, cap) and info[7] == 0, (kept, info)
    assert (rows[min(kept, cap):] == FILL).all(), "something was written behind the rows stored"
    return kept, info, rows


def equal(g, n, edges, **kw):
    """host and device entry against the model: exact rows and info.  Returns the model's info"""
    edges = np.array(edges, np.int64).reshape(-1, 4)
    kw = dict(DEFAULTS, **kw)
    want, w_info = GC.clean(n, edges, **kw)
    before = edges.copy()
    out, info = g.graph_clean(edges, n, **kw)
    print("graph_clean(n %d, m %d, %s): info %s" % (n, len(edges), kw, info.tolist()))
    assert info.tolist() == w_info.tolist(), (info.tolist(), w_info.tolist())
    assert np.array_equal(out, want), "host entry"
    assert np.array_equal(edges, before)
    kept, d_info, rows = clean_dev(g, n, edges, len(want), **kw)
    assert d_info.tolist() == w_info.tolist(), (d_info.tolist(), w_info.tolist())
    assert np.array_equal(rows[:kept], want), "device entry"
    return w_info


# ---- the rules, one small list each: (vertices, rows, limits, the rounds, tip rows and bubble rows reasoned out by hand) ----

TIP_ON_TIP = line(0, 20) + path(5, 20, 21, 22) + path(40, 21)        # the in-tip 40 goes first; 20 21 22 is an out-tip of three only then
RULES = {
    # a dead end of exactly max_tip_reads goes, one of a read more stays
    "tip_at_the_limit": (25, line(0, 20) + path(5, 20, 21) + path(10, 22, 23, 24), {}, (2, 1, 0)),
    "in_tip_at_the_limit": (25, line(0, 20) + path(20, 21, 5) + path(22, 23, 24, 10), {}, (2, 1, 0)),
    "tips_off": (25, line(0, 20) + path(5, 20, 21), dict(max_tip_reads=0), (1, 0, 0)),
    # nothing but short dead ends behind 9: all stay
    "fork_of_two_tips": (22, line(0, 10) + path(9, 20) + path(9, 21), {}, (1, 0, 0)),
    "join_of_two_tips": (22, line(0, 10) + path(20, 0) + path(21, 0), {}, (1, 0, 0)),
    # the second round sees a clean cycle, which takes no part
    "tip_on_a_cycle": (21, line(0, 6) + path(5, 0) + path(3, 20), {}, (2, 1, 0)),
    "one_read_against_seven": (21, line(0, 16) + path(2, 20, 10), {}, (2, 0, 2)),
    "seven_reads_never_lose": (21, line(0, 16) + path(2, 20, 10), dict(max_bubble_reads=8), (2, 0, 2)),
    "bubbles_off": (21, line(0, 16) + path(2, 20, 10), dict(max_bubble_reads=0), (1, 0, 0)),
    "equal_reads_by_minpid": (24, line(0, 3) + path(2, 3, 4, 5) + path(2, 20, 21, 5) + line(5, 9), {}, (2, 0, 2)),
    # 6 and 7 are one read with pairs: a full tie, both stay; without pairs 7 loses
    "full_tie_pairs_1": (13, line(0, 3) + path(2, 6, 9) + path(2, 7, 9) + line(9, 13), dict(pairs=1), (1, 0, 0)),
    "full_tie_pairs_0": (13, line(0, 3) + path(2, 6, 9) + path(2, 7, 9) + line(9, 13), dict(pairs=0), (2, 0, 2)),
    "three_arms": (23, line(0, 6) + path(5, 10) + line(10, 14) + path(2, 20, 21, 10) + path(2, 22, 10), {}, (2, 0, 4)),
    "three_arms_limit_1": (23, line(0, 6) + path(5, 10) + line(10, 14) + path(2, 20, 21, 10) + path(2, 22, 10), dict(max_bubble_reads=1), (2, 0, 2)),
    "one_q_two_p": (33, line(0, 3) + line(28, 31) + line(10, 14) + path(2, 3, 10) + path(2, 20, 10) + path(30, 31, 10) + path(30, 32, 10), {}, (2, 0, 4)),
    "tip_on_a_tip_1_round": (41, TIP_ON_TIP, dict(max_tip_reads=3, max_rounds=1), (1, 1, 0)),
    "tip_on_a_tip_2_rounds": (41, TIP_ON_TIP, dict(max_tip_reads=3, max_rounds=2), (2, 2, 0)),
    "tip_on_a_tip": (41, TIP_ON_TIP, dict(max_tip_reads=3), (3, 2, 0)),
    "no_vertices": (0, [], {}, (1, 0, 0)),
    "no_vertices_some_rows": (0, path(0, 1, 2), {}, (1, 0, 0)),
    "no_rows": (5, [], {}, (1, 0, 0)),
    "one_vertex_no_rows": (1, [], {}, (1, 0, 0)),
    # odd counts: the 32-bit arrays and the byte arrays of the scratch end inside a word.  A lone row hangs on nothing: it stays
    "three_vertices_one_row": (3, path(0, 1), {}, (1, 0, 0)),
}


@pytest.mark.parametrize("name", sorted(RULES))
def test_rules(g, name):
    n, rows, kw, (rounds, tips, bubbles) = RULES[name]
    info = equal(g, n, rows, **kw)
    assert info.tolist()[2:5] == [rounds, tips, bubbles], "the list does not show what it was made for"


def test_duplicates_self_loops_and_invalid_rows(g):
    """a duplicate of the row into a tip (both go, as tip rows), a self loop beside the path, rows that name no vertex or extend by nothing;
    with both limits zero the call filters the invalid rows and nothing else"""
    n = 25
    rows = line(0, 20) + path(5, 20, 21) + path(5, 20) + path(15, 15) + path(22, 22) + path(10, 23) + path(10, 23)
    bad = [(-1, 3, 30, 5), (3, n, 30, 5), (4, 5, 30, 0), (1 << 40, -(1 << 40), 30, -1)]
    rows = rows[:7] + bad[:2] + rows[7:] + bad[2:]
    info = equal(g, n, rows)
    assert info[3] >= 2 and info[5] == 4
    info = equal(g, n, rows, max_tip_reads=0, max_bubble_reads=0)
    assert info.tolist()[:6] == [len(rows) - 4, len(rows) - 4, 1, 0, 0, 4]
    info = equal(g, 3, path(0, 1) + path(2, 2) + bad[:1])             # three vertices and three rows: a row, a self loop, an invalid row
    assert info.tolist()[:6] == [2, 2, 1, 0, 0, 1]


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_inputs(g, name):
    _, strings, edges = pinned(name)
    info = equal(g, len(strings), edges)
    assert info.tolist()[:6] == [154, 154] + list(PINNED[name][7:10]) + [0]


# ---- the smallest shapes at which the kernels can go wrong ----

def test_backbone_beyond_a_block_of_the_scan(g):
    """more than 4096 rows and more than 4096 vertices (a block of the scan numbers 4096 items), with removed and kept rows, and heads of
    chains, on both sides of the boundary; with pairs and without, and cut by max_rounds"""
    n, edges = GC.backbone(2500, tips=[(i, 1 + i % 3) if i % 100 else (i, -2) for i in range(25, 2475, 50)], bubbles=[(i, 1 + i % 2, 1 + (i // 70) % 3) for i in range(30, 2400, 70)])
    assert n > 4096 and len(edges) > 4096
    kept = set(map(tuple, GC.clean(n, edges)[0].tolist()))
    gone = np.array([tuple(r) not in kept for r in edges.tolist()])
    assert gone[:4096].any() and gone[4096:].any() and (~gone[:4096]).any() and (~gone[4096:]).any()
    heads = np.flatnonzero(U.chains(n, edges)[0][:, 0] == np.arange(n))
    assert (heads < 4096).sum() > 10 and (heads >= 4096).sum() > 10
    info = equal(g, n, edges)
    assert info[3] > 20 and info[4] > 20 and info[2] >= 2
    equal(g, n, edges, pairs=0)
    equal(g, n, edges, max_rounds=1)


def test_one_chain_of_70001_vertices_in_shuffled_ids(g):
    """one path through 70 001 vertices whose ids are shuffled, with eight tips and eight one-read bubbles along it: chains of thousands of
    vertices whose members meet in every wave, more than four heads to a wave, and more than 16 doublings"""
    r = np.random.RandomState(7)
    N, extra = 70001, 24
    ids = r.permutation(N + extra)
    rows = path(*range(N))
    for k in range(8):
        at = 4000 + 8000 * k
        rows += path(at, N + 3 * k) + path(at + 2000, N + 3 * k + 1, at + 2002) + path(N + 3 * k + 2, at + 4000)
    edges = ids[np.array(rows, np.int64)[:, :2]]
    edges = np.concatenate([edges, np.array(rows, np.int64)[:, 2:]], axis=1)
    info = equal(g, N + extra, edges, pairs=0)
    assert info[3] == 16 and info[4] == 16 and info[2] == 2


def test_a_vertex_with_130_out_rows(g):
    """130 one-read arms from one p to one q, more than a wave has lanes: all but the arm of the smallest id lose"""
    rows = line(0, 5) + line(200, 205)
    for k in range(130):
        rows += path(4, 10 + k, 200)
    info = equal(g, 205, rows, pairs=0)
    assert info.tolist()[2:5] == [2, 0, 258]
    info = equal(g, 205, rows, pairs=1)                              # 10 and 11 are one read: both stay
    assert info.tolist()[2:5] == [2, 0, 256]


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_caps(g, entry):
    """m' comes back whatever cap is; the rows below cap are stored and nothing else is written; cap 0 with NULL counts"""
    n, edges = GC.backbone(60, tips=[(10, 1), (20, 2), (30, -2), (40, 3)], bubbles=[(5, 1, 1), (15, 1, 2), (45, 2, 1)])
    want, w_info = GC.clean(n, edges)
    k = len(want)
    assert 3 < k < len(edges)
    for cap in (0, 1, k - 1, k, k + 3):
        if entry == "host":
            kept, out, info = g.graph_clean_raw(edges, n, 2, 3, 1, 8, cap, fill=FILL)
        else:
            kept, info, out = clean_dev(g, n, edges, cap, null=cap == 0)
        assert kept == k and info.tolist() == [k, min(k, cap)] + w_info.tolist()[2:], (cap, info.tolist())
        assert np.array_equal(out[:min(k, cap)], want[:cap]) and (out[min(k, cap):] == FILL).all(), cap


# ---- end to end: reads with planted errors assemble to the genome ----

@pytest.mark.parametrize("name", sorted(PINNED))
def test_assemble_with_cleaning(hip, name):
    genome, strings, edges = pinned(name)
    a = hip.HipBwt(0)
    try:
        a.insert_multi(H.encode_batch(strings[0::2], True, True))
        n = len(strings)
        assert [s.tobytes() for s in a.extract(np.arange(n), 64)] == [s.tobytes() for s in strings]
        a.build_ssa(2)
        hashes = a.rope_hashes()
        today = [(np.asarray(t, np.uint8).tobytes(), [int(v) for v in p], c) for t, p, c in a.unitigs(U.MIN_OVLP, min_reads=3)]
        frag, info = a.assemble(U.MIN_OVLP, min_reads=3)
        assert isinstance(info, np.ndarray) and info.tolist() == [len(edges), len(edges), 0, 0, 0, 0, 0, 0]
        frag = [(t.tobytes(), p.tolist(), c) for t, p, c in frag]
        assert frag == today and frag == U.unitigs_of(strings, U.chains(n, edges)[0], True, 3) and len(frag) > 1
        none, info_none = a.assemble(U.MIN_OVLP, min_reads=3, clean=None)
        assert [(t.tobytes(), p.tolist(), c) for t, p, c in none] == today and info_none.tolist() == info.tolist()
        us, (ginfo, cinfo) = a.assemble(U.MIN_OVLP, min_reads=3, clean=CLEAN)
        print("%s: %d fragments, graph %s, clean %s" % (name, len(frag), ginfo.tolist(), cinfo.tolist()))
        assert ginfo.tolist() == info.tolist()
        assert cinfo.tolist() == GC.clean(n, edges)[1].tolist() and cinfo.tolist()[:6] == [154, 154] + list(PINNED[name][7:10]) + [0]
        assert len(us) == 1 and len(us[0][1]) == 78 and not us[0][2]
        assert us[0][0].tobytes() == np.asarray(genome, np.uint8).tobytes()
        assert a.rope_hashes() == hashes and a.ssa_info()["valid"]
        a.insert_multi(H.encode_batch(strings[0:2:2], True, True))   # an insert works behind it
        assert a._n_strings() == n + 2
    finally:
        a.close()


# ---- fatal argument checks: each fires before any kernel runs ----

FATAL = [("negative_n", "n_str and m must be"), ("negative_m", "n_str and m must be"), ("negative_cap", "cap must be"), ("negative_tip", "must not be negative"),
         ("negative_bubble", "must not be negative"), ("max_rounds", "max_rounds must be at least 1"), ("pairs", "pairs must be 0 or 1"), ("null_edges", "edges is NULL"),
         ("null_out", "out is NULL"), ("overlap", "out overlaps edges"), ("overlap_front", "out overlaps edges"), ("dev_max_rounds", "max_rounds must be at least 1"),
         ("dev_overlap", "out overlaps edges"), ("dev_null_out", "out is NULL")]


@pytest.mark.parametrize("case,what", FATAL, ids=[c for c, _ in FATAL])
def test_fatal_parameters(hip, case, what):
    """each leaves through the fatal handler with the function's name and a message of its own, the buffers untouched"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "graph_clean_child.py"), case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out, err = p.stdout.decode(), p.stderr.decode()[-1500:]
    assert p.returncode == 7 and "the call returned" not in out, (p.returncode, out, err)
    assert "handler: [rb2_hip] graph_clean" in out and what in out and "unchanged ok" in out, out
