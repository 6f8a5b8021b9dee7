"""Rounds of one-member groups ("the steady round"): once the device has reported a round in which every interval was
empty and k_sym placed every tile itself, the host knows every interval empty and the dense rounds of one engine launch no k_prep<AE> (the
k_advance instantiation without the group search was measured and not kept: steady_stats()["advance_single"] stays 0).  Every job compares
the six ropes and the 6x6 count matrix with the oracle after EVERY batch and reads rb2_hip_steady_stats.

Small batches are over before the host hears anything, so the jobs that must reach the new path are waited for (RB2_HIP_LAZY_INSERT=0: a
lazy host-buffer insert is never held back) and stay one round ahead of the last report (RB2_STEADY_AHEAD=1): the path is taken from the
round after the report.
"""
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

K1 = {"RB2_STEADY_AHEAD": "1", "RB2_HIP_LAZY_INSERT": "0"}
DENSE = {"RB2_SPARSE_LAMBDA": "0"}
FORCED = {"RB2_SPARSE_LAMBDA": "1e18", "RB2_SPARSE_MAXPEN": "0"}

_want = {}


def oracle_of(key, so, batches, before=None):
    """(count matrix, six ropes) after every batch: the oracle runs once per job and order, whatever the number of engine variants"""
    if (key, so) not in _want:
        o = H.Oracle(so)
        if before is not None:
            o.insert_multi(before)
        out = []
        for buf in batches:
            o.insert_multi(buf)
            out.append((o.counts().copy(), [o.rope(b).copy() for b in range(6)]))
        o.close()
        _want[(key, so)] = out
    return _want[(key, so)]


def check_job(key, make, so, batches, env=None, before=None, stats=None):
    """insert the batches into make(); ropes and counts after every batch against the oracle; returns stats(g) (default: steady_stats)"""
    env = env or {}
    want = oracle_of(key, so, batches, before)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        g = make()
        for i, buf in enumerate(batches):
            g.insert_multi(buf)
            cnt, ropes = want[i]
            assert np.array_equal(cnt, g.counts()), "count matrix differs after batch %d" % i
            for b in range(6):
                rg = g.rope(b)
                assert len(ropes[b]) == len(rg), "rope %d length after batch %d" % (b, i)
                assert np.array_equal(ropes[b], rg), "rope %d differs after batch %d at %s" % (b, i, np.flatnonzero(ropes[b] != rg)[:5])
        st = stats(g) if stats else g.steady_stats()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    g.close()
    return st


def took_the_path(st):
    assert st["prep_skipped"] > 0, st
    assert st["used_from"] >= st["reported_at"] >= 0, st


# ---- tile edges: a last tile of one string (513, 1025), a tile one short of full (511), bucket boundaries inside the tile run; 24 symbols
# ---- are two cursor refills in rounds without k_prep ---------------------------------------------------------------------------------

@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("n", [511, 513, 1025])
def test_tile_edges(hip, so, n):
    codes = H.splitmix_bases(n, 24, seed=300 + n)
    took_the_path(check_job(("edges", n), lambda: hip.HipBwt(so), so, [H.encode_batch_fixed(codes)], env=K1))


# ---- strings that end at different rounds: sentinel rows inside fused tiles, tiles that lose strings in rounds without k_prep ---------

def mixed_lengths():
    rng = np.random.RandomState(23)
    return [rng.randint(1, 5, size=5 + i % 36).astype(np.uint8) for i in range(1500)]


@pytest.mark.parametrize("so", [0, 1])
def test_strings_end_at_different_rounds(hip, so):
    took_the_path(check_job("mixed", lambda: hip.HipBwt(so), so, [H.encode_batch(mixed_lengths())], env=K1))


# ---- a loaded index: the second batch starts with non-empty intervals and crosses into the state on the way ----------------------------

def two_batches():
    codes = H.splitmix_bases(3000, 30, seed=77)
    return H.encode_batch_fixed(codes[:1500]), H.encode_batch_fixed(codes[1500:])


@pytest.mark.parametrize("so", [1, 2])
@pytest.mark.parametrize("loaded", [False, True])
def test_second_batch_crosses_into_the_state(hip, so, loaded):
    """loaded: the first batch arrives as run-length coded ropes (load_ropes), the second is the only insert"""
    from ropebwt2_amd.hipbwt import encode_runs
    b0, b1 = two_batches()
    want = oracle_of("two", so, [b0, b1])
    if not loaded:
        st = check_job("two", lambda: hip.HipBwt(so), so, [b0, b1], env=dict(K1, **DENSE))
    else:
        ropes = [encode_runs(r) for r in want[0][1]]

        def make():
            g = hip.HipBwt(so)
            g.load_ropes(ropes)
            return g
        st = check_job("two_loaded", make, so, [b1], env=dict(K1, **DENSE), before=b0)
    took_the_path(st)
    assert st["reported_at"] > 0, st                               # (round 0 of a sorted batch on an index: every interval is [0, n0))


def test_64_bit_positions(hip):
    """RB2_POS=64: the instantiation for 8-byte positions, and the report without the narrow mode's (round, largest piece) word"""
    b0, b1 = two_batches()
    took_the_path(check_job("two", lambda: hip.HipBwt(1), 1, [b0, b1], env=dict(K1, RB2_POS="64", **DENSE)))


# ---- never steady: two identical reads stay one group in the sorted orders -----------------------------------------------------------

def with_a_duplicate():
    codes = H.splitmix_bases(1500, 24, seed=55)
    codes[1200] = codes[37]
    return H.encode_batch_fixed(codes)


@pytest.mark.parametrize("so", [1, 2])
def test_identical_reads_never_reach_the_state(hip, so):
    st = check_job("dup", lambda: hip.HipBwt(so), so, [with_a_duplicate()], env=K1)
    assert st["advance_single"] == 0 and st["prep_skipped"] == 0 and st["reported_at"] == -1 and st["used_from"] == -1, st


def test_identical_reads_in_input_order(hip):
    """input order: every string is a group of its own from round 0 on; the new path may run, parity only"""
    check_job("dup", lambda: hip.HipBwt(0), 0, [with_a_duplicate()], env=K1)


# ---- void rounds: an in-place round voids after the state was reached ------------------------------------------------------------

def hot_spot_batches():
    """second batch: 16 random symbols behind 40 A's (rounds go from the last symbol to the first) -- rows differ from round ~8 on, and from round
    16 on every string inserts A into the few leaves that hold the suffixes A..A + its own 16: the forced in-place rounds there are void"""
    first = H.encode_batch_fixed(H.splitmix_bases(1000, 60, seed=31))
    tail = H.splitmix_bases(1500, 16, seed=32)
    reads = np.concatenate([np.full((1500, 40), 1, np.uint8), tail.astype(np.uint8)], axis=1)
    return first, H.encode_batch_fixed(reads)


def test_void_round_after_the_state(hip):
    b0, b1 = hot_spot_batches()
    # the same job on the dense layout says when the state is first reported ...
    dense = check_job("hot", lambda: hip.HipBwt(1), 1, [b0, b1], env=dict(K1, **DENSE))
    took_the_path(dense)
    # ... and forced in place: void rounds behind that round, the host forgets the report, the rounds redone report again, the job goes on
    both = check_job("hot", lambda: hip.HipBwt(1), 1, [b0, b1], env=dict(K1, **FORCED), stats=lambda g: (g.steady_stats(), g.layout_stats()))
    st, lay = both
    assert lay["void_rounds"] > 0 and lay["sparse_rounds"] > 0, (st, lay)
    took_the_path(st)
    assert st["reported_at"] > dense["reported_at"], (st, dense, lay)   # (restarted by a rollback behind the first report)


# ---- the switch -----------------------------------------------------------------------------------------------------------------------

def test_switch_off(hip):
    st = check_job(("edges", 1025), lambda: hip.HipBwt(1), 1, [H.encode_batch_fixed(H.splitmix_bases(1025, 24, seed=300 + 1025))], env=dict(K1, RB2_STEADY="0"))
    assert st["advance_single"] == 0 and st["prep_skipped"] == 0, st
    assert st["reported_at"] >= 0, st                              # (the report is still read)


# ---- two PEER ranks on one device keep their kernels ----------------------------------------------------------------------------------

@pytest.mark.parametrize("so", [0, 2])
def test_two_peer_ranks_agree(hip, so):
    from ropebwt2_amd import MultiBwt
    codes = H.splitmix_bases(1025, 24, seed=300 + 1025)

    def stats(m):
        return [m.engine(k).steady_stats() for k in range(2)]
    for st in check_job(("edges", 1025), lambda: MultiBwt(so, [0, 0], "peer"), so, [H.encode_batch_fixed(codes)], env=K1, stats=stats):
        assert st["advance_single"] == 0 and st["prep_skipped"] == 0 and st["reported_at"] == -1 and st["used_from"] == -1, st
