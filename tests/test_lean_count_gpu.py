"""The lean count ("the lean count"; RB2_STEADY_LEAN=2): in a lean round whose counting tail is the three-launch form,
one small launch (k_count_lean) reads A alone and writes the tile records and the chunk totals in the place of the k_sym and k_tscan1 launches;
k_advance takes every string for a group head; every RB2_LEAN_AUDIT-th lean round of a batch is counted by k_sym as in stage 1.

The jobs, their environment and the oracle cache are those of tests/test_steady_round_gpu.py.  Every job runs with RB2_TS_MAX=0 (the
three-launch tail whatever the number of tiles) and RB2_LEAN_VERIFY=1: k_sym and k_tscan1 run as well, into buffers of their own, and a kernel
counts the words in which the records or the chunk totals differ -- none may.  Ropes and count matrix are compared with the oracle after every
batch (S.check_job).
"""
import os

import numpy as np
import pytest

import helpers as H
import test_steady_round_gpu as S

pytestmark = pytest.mark.gpu

TAIL3 = {"RB2_TS_MAX": "0"}


def count_env(stage=2, **more):
    return dict(S.K1, RB2_STEADY_LEAN=str(stage), RB2_LEAN_VERIFY="1", **dict(TAIL3, **more))


def all_stats(g):
    return g.steady_stats(), g.lean_stats(), g.lean_count_stats(), g.layout_stats()


def counted_lean(st):
    steady, lean, cnt, _ = st
    assert lean["stage"] == 2, st
    assert cnt["mismatches"] == 0, st
    assert cnt["counted"] > 0, st
    assert cnt["verified"] >= cnt["counted"], st                    # (a round counted again after a rollback is verified twice)
    assert cnt["counted"] + cnt["audit"] == lean["rounds"] <= steady["prep_skipped"], st
    S.took_the_path(steady)


# ---- tile and bucket edges: short last tiles, a tile of one string, buckets of no and of one string; every bucket starts at an odd byte ----

@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("n", [40, 511, 513, 1025])
def test_tile_and_bucket_edges(hip, so, n):
    codes = H.splitmix_bases(n, 24, seed=300 + n)
    counted_lean(S.check_job(("edges", n), lambda: hip.HipBwt(so), so, [H.encode_batch_fixed(codes)], env=count_env(), stats=all_stats))


# ---- the other lean jobs ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("so", [0, 1])
def test_strings_end_at_different_rounds(hip, so):
    counted_lean(S.check_job("mixed", lambda: hip.HipBwt(so), so, [H.encode_batch(S.mixed_lengths())], env=count_env(), stats=all_stats))


@pytest.mark.parametrize("pos", ["0", "64"])
@pytest.mark.parametrize("so", [1, 2])
def test_second_batch_on_a_loaded_index(hip, so, pos):
    b0, b1 = S.two_batches()
    counted_lean(S.check_job("two", lambda: hip.HipBwt(so), so, [b0, b1], env=count_env(RB2_POS=pos, **S.DENSE), stats=all_stats))


def test_void_round_after_the_state(hip):
    b0, b1 = S.hot_spot_batches()
    st = S.check_job("hot", lambda: hip.HipBwt(1), 1, [b0, b1], env=count_env(**S.FORCED), stats=all_stats)
    assert st[3]["void_rounds"] > 0 and st[3]["sparse_rounds"] > 0, st
    counted_lean(st)


@pytest.mark.parametrize("so", [1, 2])
def test_identical_reads_are_never_counted_this_way(hip, so):
    _, lean, cnt, _ = S.check_job("dup", lambda: hip.HipBwt(so), so, [S.with_a_duplicate()], env=count_env(), stats=all_stats)
    assert lean["rounds"] == 0 and cnt == {"counted": 0, "audit": 0, "verified": 0, "mismatches": 0}, (lean, cnt)


# ---- a chunk border: more than SCHUNK = 1024 tiles, so two blocks of k_count_lean, the second one short; full tiles at odd bytes ------------

def test_two_chunks(hip):
    n = 530000
    codes = H.splitmix_bases(n, 24, seed=77)
    key = ((codes - 1).astype(np.uint64) << (2 * np.arange(24, dtype=np.uint64))).sum(axis=1)   # (codes 1..4: two bits a base, 48 bits a read)
    assert len(np.unique(key)) == n, "the reads are distinct: every group of the sorted order ends up with one member"
    buf = H.encode_batch_fixed(codes)

    def run(env):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            g = hip.HipBwt(1)
            g.insert_multi(buf)
            out = g.rope_hashes(), g.counts().copy(), all_stats(g)
            g.close()
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        return out
    h2, c2, st2 = run(count_env(2, **S.DENSE))
    h1, c1, st1 = run(count_env(1, **S.DENSE))
    counted_lean(st2)
    assert st1[1]["stage"] == 1 and st1[1]["rounds"] > 0 and st1[2]["counted"] == 0, st1
    assert h2 == h1 and np.array_equal(c2, c1)
    assert int(c2.sum()) == n * 25


# ---- audit rounds and the switches --------------------------------------------------------------------------------------------------------

def edges_job(hip, env):
    buf = H.encode_batch_fixed(H.splitmix_bases(1025, 24, seed=300 + 1025))
    return S.check_job(("edges", 1025), lambda: hip.HipBwt(1), 1, [buf], env=env, stats=all_stats)


def test_every_round_audited(hip):
    steady, lean, cnt, _ = edges_job(hip, count_env(RB2_LEAN_AUDIT="1"))
    assert lean["stage"] == 2 and lean["rounds"] > 0, lean
    assert cnt["counted"] == 0 and cnt["verified"] == 0 and cnt["mismatches"] == 0 and cnt["audit"] == lean["rounds"], (lean, cnt)


def test_every_third_round_audited(hip):
    steady, lean, cnt, _ = edges_job(hip, count_env(RB2_LEAN_AUDIT="3"))
    assert cnt["counted"] > 0 and cnt["audit"] > 0 and cnt["mismatches"] == 0, cnt
    assert cnt["counted"] + cnt["audit"] == lean["rounds"], (lean, cnt)
    assert cnt["counted"] in (2 * cnt["audit"], 2 * cnt["audit"] + 1, 2 * cnt["audit"] + 2), cnt


def test_never_audited(hip):
    steady, lean, cnt, _ = edges_job(hip, count_env(RB2_LEAN_AUDIT="0"))
    assert cnt["audit"] == 0 and cnt["counted"] == lean["rounds"] > 0 and cnt["mismatches"] == 0, (lean, cnt)


@pytest.mark.parametrize("env", [{"RB2_STEADY_LEAN": "1"}, {"RB2_STEADY_LEAN": "0"}, {"RB2_STEADY": "0"}])
def test_switched_off(hip, env):
    steady, lean, cnt, _ = edges_job(hip, dict(S.K1, RB2_LEAN_VERIFY="1", **dict(TAIL3, **env)))
    assert cnt == {"counted": 0, "audit": 0, "verified": 0, "mismatches": 0}, cnt
    assert lean["stage"] == (1 if env.get("RB2_STEADY_LEAN") == "1" else 0), lean


def test_the_one_launch_tail_keeps_stage_1(hip):
    """few tiles and the default RB2_TS_MAX: the counting tail is k_tscan_setup, which reads the records of a k_sym launch"""
    buf = H.encode_batch_fixed(H.splitmix_bases(1025, 24, seed=300 + 1025))
    steady, lean, cnt, _ = S.check_job(("edges", 1025), lambda: hip.HipBwt(1), 1, [buf], env=dict(S.K1, RB2_STEADY_LEAN="2"), stats=all_stats)
    assert lean["stage"] == 1 and lean["rounds"] > 0, lean        # (the stage in force: stage 2 has met no round it could take)
    assert cnt == {"counted": 0, "audit": 0, "verified": 0, "mismatches": 0}, cnt
