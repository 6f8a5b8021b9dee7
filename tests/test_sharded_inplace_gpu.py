"""Void in-place rounds, leaf splits and re-spreads on a SHARDED index (rb2_hip_multi_*, csrc/rb2_multi.h): the counterpart of
test_inplace_paths_gpu.py for the host code a rank of a MultiBwt runs.

A rank never queues rounds behind a verdict: round_merge_sparse runs with spec = false and waits for the verdict of every in-place round.
A void round is taken back at depth 1 (take_back) and redone densely (round_merge_any: void_to_dense, then a dense round whose k_setup is
rebuilt from h->gcnt -- under PEER the matrix k_mround summed over the peers, under RCCL the all-reduced one).  Under PEER the other
ranks' k_advance of the same round store their strings into the void rank's next-round arrays meanwhile; under RCCL the void attempt must
leave the send buffer alone and the dense redo fill it before the exchange.

Every case runs forced sparse (FORCED), compares the count matrix with the oracle after every batch and all six ropes at the end, and
asserts from the per-rank layout_stats() / rewind_stats() that its path ran.  The jobs and the owner maps are sharded_void_jobs.py,
whose reach is proved on the CPU (test_sharded_void_jobs.py).  Every figure a case asserts on is printed first.
"""
import numpy as np
import pytest

import helpers as H
import sharded_void_jobs as J
from test_inplace_paths_gpu import Env, FORCED, fixture_c

pytestmark = pytest.mark.gpu

JOBS = {"mixed": J.mixed_job, "c": lambda: fixture_c()[0]}
MIXED = 1                                       # the mixed void batch is batch 1 of the mixed job
_jobs, _want, _default = {}, {}, {}


def jobs_of(name):
    if name not in _jobs:
        _jobs[name] = JOBS[name]()
    return _jobs[name]


def oracle_of(name, so):
    """(count matrix, six ropes) after every batch of a job -- the oracle runs once per job and order"""
    if (name, so) not in _want:
        o, out = H.Oracle(so), []
        for buf in jobs_of(name):
            o.insert_multi(buf)
            out.append((o.counts().copy(), o.ropes()))
        o.close()
        _want[(name, so)] = out
    return _want[(name, so)]


def snap(m):
    """per local rank: layout_stats() and rewind_stats() in one dict"""
    return [dict(m.engine(k).layout_stats(), **m.engine(k).rewind_stats()) for k in range(m.n)]


def run_batches(m, name, so, what, first=0):
    """batches first.. of a job into m, the count matrix checked after each; per batch: (per-rank stats before, after, m.stats() before, after)"""
    want, log = oracle_of(name, so), []
    for i, buf in enumerate(jobs_of(name)):
        if i < first:
            continue
        s0, g0 = snap(m), m.stats()
        m.insert_multi(buf)
        s1, g1 = snap(m), m.stats()
        assert np.array_equal(m.counts(), want[i][0]), "%s: count matrix after batch %d" % (what, i)
        log.append((s0, s1, g0, g1))
    return log


def check_ropes(m, name, so, what):
    ropes = oracle_of(name, so)[-1][1]
    for b in range(6):
        got = m.rope(b)
        assert len(got) == len(ropes[b]) and np.array_equal(got, ropes[b]), \
            "%s: rope %d differs at %s" % (what, b, np.flatnonzero(got[:len(ropes[b])] != ropes[b][:len(got)])[:5])


def delta(s0, s1, key):
    return [b[key] - a[key] for a, b in zip(s0, s1)]


def check_void_batch(entry, n, what):
    """case a over the mixed batch: rank 0 went void, no rank ever rewound (a sharded rank never queues behind a verdict), and (n >= 2)
    for some rank j: void rounds of rank 0 + in-place rounds of rank j > rounds -- at least one round in which rank 0 was void and redone
    densely while rank j finished in place and pushed its strings into rank 0's arrays"""
    s0, s1, g0, g1 = entry
    dv, ds, R = delta(s0, s1, "void_rounds"), delta(s0, s1, "sparse_rounds"), g1["rounds"] - g0["rounds"]
    fig = "%s: mixed batch dvoid %s dsparse %s R %d" % (what, dv, ds, R)
    print(fig)
    assert dv[0] > 0, fig
    assert all(s["rewinds"] == 0 and s["rounds_taken_back"] == 0 for s in s1), (fig, s1)
    if n >= 2:
        assert max(dv[0] + ds[j] for j in range(1, n)) > R, fig


def check_syncs(log, rccl, what):
    """host_syncs_in_rounds (rb2_multi.h multi_rank_batch): rank 0's verdict waits, sparse_rounds + void_rounds of engine(0); RCCL adds one
    event wait per round -- per batch, from just after construction"""
    for i, (s0, s1, g0, g1) in enumerate(log):
        d = g1["host_syncs_in_rounds"] - g0["host_syncs_in_rounds"]
        want = (s1[0]["sparse_rounds"] + s1[0]["void_rounds"]) - (s0[0]["sparse_rounds"] + s0[0]["void_rounds"])
        if rccl:
            want += g1["rounds"] - g0["rounds"]
        print("%s: batch %d host syncs %d, want %d" % (what, i, d, want))
        assert d == want, (what, i, d, want)


def check_rank_queries(m, name, so, what):
    """case c: rank1a on the layouts the batches left (some rank still sparse) at piece boundaries +-1, 0, the rope's length and a few
    random places -- before anything (rope(), rope_hashes()) makes every rank dense"""
    st = snap(m)
    print("%s: sparse_now %s" % (what, [s["sparse_now"] for s in st]))
    assert any(s["sparse_now"] for s in st), (what, st)
    cnt, ropes = oracle_of(name, so)[-1]
    rng = np.random.RandomState(5 + so)
    for b in range(6):
        ro = ropes[b]
        bounds = np.concatenate([[0], np.cumsum(cnt[:, b])])     # piece (b, x) holds the b's of rope x (include/rb2_hip.h)
        assert bounds[-1] == len(ro)
        xs = {int(x) + d for x in bounds for d in (-1, 0, 1)} | {int(x) for x in rng.randint(0, len(ro) + 1, size=4)}
        for x in sorted(xs):
            if 0 <= x <= len(ro):
                assert np.array_equal(m.rank1a(b, x), np.bincount(ro[:x], minlength=6)), "%s: rank1a(%d, %d)" % (what, b, x)


def run_void_job(hip, n, so, env, transport="peer", queries=False):
    """the mixed job on n ranks with void_owner_map under FORCED + env (set before the handle: the knobs are read in rb2_hip_create) with
    case a's and b's assertions; returns (rope hashes, compact rounds summed over the ranks, per-rank stats at the end)"""
    what = "n %d so %d %s %s" % (n, so, transport, env)
    owners = J.void_owner_map(jobs_of("mixed")[MIXED], n)
    with Env(**dict(FORCED, **env)):
        m = hip.MultiBwt(so, [0] * n, transport, owners=owners)
        try:
            log = run_batches(m, "mixed", so, what)
            check_void_batch(log[MIXED], n, what)
            check_syncs(log, transport == "rccl", what)
            end = log[-1][1]
            if queries:
                check_rank_queries(m, "mixed", so, what)
            check_ropes(m, "mixed", so, what)
            compact = sum(m.engine(k).window_stats()["compact_rounds"] for k in range(m.n))
            hashes = m.rope_hashes()
        finally:
            m.close()
    return hashes, compact, end


def default_run(hip, n, so):
    if (n, so) not in _default:
        _default[(n, so)] = run_void_job(hip, n, so, {})
    return _default[(n, so)]


# ---- a + b + c: one rank void, the others in place in the same rounds (PEER); verdict waits counted; rank queries on mixed layouts ----

@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_void_rank_beside_in_place_ranks(hip, n, so):
    """n = 1 is PEER with one rank: nranks == 1 but no send buffer"""
    _default[(n, so)] = run_void_job(hip, n, so, {}, queries=True)


# ---- d: the RCCL transport on a group of one ------------------------------------------------------------------------------------

@pytest.mark.parametrize("self_msgs", ["0", "1"])
@pytest.mark.parametrize("so", [0, 2])
def test_rccl_group_of_one_void_rounds(hip, so, self_msgs):
    """the void attempt leaves the send buffer alone, the dense redo fills it before ncclSend / k_munpack; one event wait per round on
    top of the verdict waits"""
    _, _, end = run_void_job(hip, 1, so, {"RB2_RCCL_SELF": self_msgs}, transport="rccl")
    print("rccl so %d self %s: %s" % (so, self_msgs, end))
    assert end[0]["void_rounds"] > 0 and end[0]["sparse_rounds"] > 0, end


# ---- e: the fallback knobs a rank reaches (multi_rank_batch: choose_layout, round_counts without spec, round_merge_sparse, round_merge_any) ----

KNOBS = {
    "dir_ride0": {"RB2_DIR_RIDE": "0"},             # round_merge_sparse: the directory scan as launches of its own
    "ts_blocks1": {"RB2_TS_BLOCKS": "1"},           # round_counts: the single-launch counting tail (k_tscan_setup) on one block ...
    "ts_blocks3": {"RB2_TS_BLOCKS": "3"},           # ... on three
    "ts_max2": {"RB2_TS_MAX": "2"},                 # round_counts: k_tscan1-3 + k_tfix
    "leaf_pipe0": {"RB2_LEAF_PIPE": "0"},           # round_merge_sparse: k_merge_leaf grid
    "leaf_pipe4": {"RB2_LEAF_PIPE": "4"},
    "sparse_head0": {"RB2_SPARSE_HEAD": "0"},       # multi_rank_batch: no dense head -- in place (and void) from round 0
    "compact0": {"RB2_COMPACT": "0"},               # round_merge_any: dense rounds write plain windows only
}


@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_knobs_on_sharded_void_rounds(hip, knob, n, so):
    hashes, compact, _ = run_void_job(hip, n, so, KNOBS[knob])
    if knob == "compact0":
        h0, c0, _ = default_run(hip, n, so)
        print("n %d so %d: compact rounds %d, default %d" % (n, so, compact, c0))
        assert compact == 0 and c0 > 0, (compact, c0)
        assert hashes == h0


# ---- f: leaf splits and re-spreads per rank ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 8])
def test_splits_and_respreads_per_rank(hip, n):
    """fixture c (long reads with runs of N, both strands; short repetitive reads) on the default owner map"""
    so, what = 2, "c n %d" % n
    with Env(**FORCED):
        m = hip.MultiBwt(so, [0] * n, "peer")
        try:
            log = run_batches(m, "c", so, what)
            end = log[-1][1]
            check_ropes(m, "c", so, what)
        finally:
            m.close()
    splits, respreads = sum(s["leaf_splits"] for s in end), sum(s["respreads"] for s in end)
    print("%s: leaf splits %s (sum %d), re-spreads %s (sum %d), void %s" % (what, [s["leaf_splits"] for s in end], splits,
                                                                           [s["respreads"] for s in end], respreads, [s["void_rounds"] for s in end]))
    assert splits > 0 and respreads > 0
    assert all(s["rewinds"] == 0 for s in end), end


# ---- g: a loaded index, then the void batch --------------------------------------------------------------------------------------

@pytest.mark.parametrize("so", [0, 2])
@pytest.mark.parametrize("n", [2, 8])
def test_loaded_index_then_void_batch(hip, n, so):
    from ropebwt2_amd.hipbwt import encode_runs
    what = "loaded n %d so %d" % (n, so)
    cnt0, ropes0 = oracle_of("mixed", so)[0]
    with Env(**FORCED):
        m = hip.MultiBwt(so, [0] * n, "peer", owners=J.void_owner_map(jobs_of("mixed")[MIXED], n))
        try:
            m.load_ropes([encode_runs(r) for r in ropes0])
            assert np.array_equal(m.counts(), cnt0), what
            log = run_batches(m, "mixed", so, what, first=MIXED)
            check_void_batch(log[0], n, what)
            check_syncs(log, False, what)
            check_ropes(m, "mixed", so, what)
        finally:
            m.close()


# ---- h: the same index as one engine ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("so", [0, 1, 2])
def test_same_index_as_one_engine(hip, so):
    """rb2_hip_multi_rope_hash == rb2_hip_rope_hash across mixed layouts: case a on 3 ranks against one HipBwt, both forced sparse"""
    want = default_run(hip, 3, so)[0]
    with Env(**FORCED):
        one = hip.HipBwt(so)
        for buf in jobs_of("mixed"):
            one.insert_multi(buf)
        got = one.rope_hashes()
        one.close()
    assert got == want, (got, want)
