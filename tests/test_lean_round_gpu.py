"""The lean round ("the lean round"): a dense round of one engine that the host knows to be a round of one-member groups
and empty intervals when it queues its counting phase (RB2_STEADY_LEAN=1, the default): k_sym writes no INS_E / INS_A, k_part bisects on L and
k_merge takes a new symbol's place in its window from L & 4095 and its symbol from A & 7.  (The second stage -- k_sym reads A only and sets no
head flag, k_advance takes every string for a group head -- passed these jobs, was measured and taken out: DESIGN.md; RB2_STEADY_LEAN=2 runs
stage 1.)  Every job compares the six ropes and the 6 x 6 count matrix with the oracle after EVERY batch and reads rb2_hip_lean_stats.

The jobs, their environment (the host stays one round behind the report, inserts are waited for) and the oracle cache are those of
tests/test_steady_round_gpu.py.

Not among the jobs: a round that is counted lean and then run in place (the recount of round_merge_any).  No knob produces one -- the host
decides on the layout of round r (choose_layout) before it queues the round's counting phase, a counting phase queued ahead of its round is the
one behind an in-place round (k_sym<.., SPLIT>), which is never lean, and RB2_SPARSE_LAMBDA / RB2_SPARSE_MAXPEN act in choose_layout only.  The
recount is a guard for a caller that does not exist yet.
"""
import numpy as np
import pytest

import helpers as H
import bcr_rounds_ref as M
import test_steady_round_gpu as S

pytestmark = pytest.mark.gpu

STAGES = [1]                                                       # (the stages the library has)


def lean_env(stage, **more):
    return dict(S.K1, RB2_STEADY_LEAN=str(stage), **more)


def all_stats(g):
    return g.steady_stats(), g.lean_stats(), g.layout_stats()


def ran_lean(st, stage):
    steady, lean, _ = st
    assert lean["stage"] == stage, st
    assert lean["rounds"] > 0, st
    assert lean["rounds"] <= steady["prep_skipped"], st             # (a lean round is a dense round without a k_prep launch)
    S.took_the_path(steady)


# ---- tile edges: a last tile of one string, pair blocks whose second tile is missing or lies in another bucket, two cursor refills ------

@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("n", [511, 513, 1025])
def test_tile_edges(hip, so, n, stage):
    codes = H.splitmix_bases(n, 24, seed=300 + n)
    ran_lean(S.check_job(("edges", n), lambda: hip.HipBwt(so), so, [H.encode_batch_fixed(codes)], env=lean_env(stage), stats=all_stats), stage)


# ---- more than 64 inserts in one window: the second turn of the insert loop and the re-read of step 5 ------------------------------------

@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("so", [0, 1])
def test_more_than_64_inserts_in_a_window(hip, so, stage):
    n = 1500
    buf = H.encode_batch_fixed(H.splitmix_bases(n, 30, seed=41))
    want = S.oracle_of("ni64", so, [buf])
    # from the sizes alone: a piece never has more windows than at the end of the batch, every round inserts n symbols, so some window of every
    # round takes more than 64 of them
    nwin = int(((M.piece_sizes(want[0][0]) + M.WIN - 1) // M.WIN).sum())
    assert n > 64 * nwin, (n, nwin)
    ran_lean(S.check_job("ni64", lambda: hip.HipBwt(so), so, [buf], env=lean_env(stage), stats=all_stats), stage)


# ---- strings that end at different rounds: sentinels arrive inside lean rounds, the windows go compact with one or two exception lines ----

@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("so", [0, 1])
def test_strings_end_at_different_rounds(hip, so, stage):
    ran_lean(S.check_job("mixed", lambda: hip.HipBwt(so), so, [H.encode_batch(S.mixed_lengths())], env=lean_env(stage), stats=all_stats), stage)


# ---- a loaded index: the second batch crosses from non-empty intervals into the state ----------------------------------------------------

@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("pos", ["0", "64"])
@pytest.mark.parametrize("so", [1, 2])
def test_second_batch_on_a_loaded_index(hip, so, pos, stage):
    b0, b1 = S.two_batches()
    st = S.check_job("two", lambda: hip.HipBwt(so), so, [b0, b1], env=lean_env(stage, RB2_POS=pos, **S.DENSE), stats=all_stats)
    ran_lean(st, stage)
    assert st[0]["reported_at"] > 0, st                            # (round 0 of a sorted batch on an index: every interval is [0, n0))


# ---- never steady: two identical reads stay one group in the sorted orders ---------------------------------------------------------------

@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("so", [1, 2])
def test_identical_reads_never_run_lean(hip, so, stage):
    _, lean, _ = S.check_job("dup", lambda: hip.HipBwt(so), so, [S.with_a_duplicate()], env=lean_env(stage), stats=all_stats)
    assert lean["rounds"] == 0 and lean["stage"] == stage, lean


# ---- void rounds behind lean rounds: the rollback forgets the report, the rounds redone write their insert lists, lean rounds come back ------

@pytest.mark.parametrize("stage", STAGES)
def test_void_round_after_the_state(hip, stage):
    b0, b1 = S.hot_spot_batches()
    dense = S.check_job("hot", lambda: hip.HipBwt(1), 1, [b0, b1], env=lean_env(stage, **S.DENSE), stats=all_stats)
    ran_lean(dense, stage)
    forced = S.check_job("hot", lambda: hip.HipBwt(1), 1, [b0, b1], env=lean_env(stage, **S.FORCED), stats=all_stats)
    steady, lean, lay = forced
    assert lay["void_rounds"] > 0 and lay["sparse_rounds"] > 0, forced
    ran_lean(forced, stage)
    assert steady["reported_at"] > dense[0]["reported_at"], (forced, dense)   # (restarted by a rollback behind the first report: the lean rounds behind it follow the NEW report)


# ---- the switches ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("env", [{"RB2_STEADY_LEAN": "0"}, {"RB2_STEADY": "0"}, {"RB2_STEADY": "0", "RB2_STEADY_LEAN": "2"}])
def test_switched_off(hip, env):
    buf = H.encode_batch_fixed(H.splitmix_bases(1025, 24, seed=300 + 1025))
    steady, lean, _ = S.check_job(("edges", 1025), lambda: hip.HipBwt(1), 1, [buf], env=dict(S.K1, **env), stats=all_stats)
    assert lean["rounds"] == 0 and lean["stage"] == 0, lean
    assert steady["reported_at"] >= 0, steady                     # (the report is still read)
    if "RB2_STEADY" not in env:
        S.took_the_path(steady)                                    # (lean off: the rounds without k_prep of the steady round as before)


def test_a_stage_beyond_the_last_is_the_last(hip):
    buf = H.encode_batch_fixed(H.splitmix_bases(1025, 24, seed=300 + 1025))
    ran_lean(S.check_job(("edges", 1025), lambda: hip.HipBwt(1), 1, [buf], env=lean_env(2), stats=all_stats), STAGES[-1])


# ---- two PEER ranks on one device keep their kernels -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("so", [0, 2])
def test_two_peer_ranks_never_run_lean(hip, so):
    from ropebwt2_amd import MultiBwt
    codes = H.splitmix_bases(1025, 24, seed=300 + 1025)

    def stats(m):
        return [m.engine(k).lean_stats() for k in range(2)]
    for lean in S.check_job(("edges", 1025), lambda: MultiBwt(so, [0, 0], "peer"), so, [H.encode_batch_fixed(codes)], env=S.K1, stats=stats):
        assert lean["rounds"] == 0, lean
