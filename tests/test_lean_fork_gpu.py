"""The forked round ("the forked round"; RB2_LEAN_FORK, default 1): the counting tail of a round counted by k_count_lean
(k_count_lean, the tile scans, k_tfix with the count-dependent half of setup_body) runs on a side stream beside k_part<.., FORK>, k_merge and the
directory of the same round; k_part lays out the new side itself, from the old piece sizes and the bucket sizes; k_advance waits for both.

The jobs, their environment and the oracle cache are those of tests/test_steady_round_gpu.py and tests/test_lean_count_gpu.py.  Every job runs
with RB2_TS_MAX=0 (the three-launch tail whatever the number of tiles) and WITHOUT RB2_LEAN_VERIFY (a verified round is never forked).  Ropes and
count matrix are compared with the oracle after every batch (S.check_job); rb2_hip_lean_fork_stats says which rounds were forked: every round
counted by k_count_lean, and no other.
"""
import ctypes
import os

import numpy as np
import pytest

import helpers as H
import test_steady_round_gpu as S
import test_lean_count_gpu as C

pytestmark = pytest.mark.gpu


def fork_env(**more):
    return dict(S.K1, RB2_STEADY_LEAN="2", **dict(C.TAIL3, **more))


def all_stats(g):
    return g.steady_stats(), g.lean_stats(), g.lean_count_stats(), g.layout_stats(), g.lean_fork_stats()


def forked_where_counted(st):
    steady, lean, cnt, _, fork = st
    assert fork["on"] == 1, st
    assert lean["stage"] == 2, st
    assert cnt["verified"] == 0 and cnt["mismatches"] == 0, st
    assert fork["forked"] == cnt["counted"] > 0, st                  # every round counted by k_count_lean, and no other
    assert cnt["counted"] + cnt["audit"] == lean["rounds"] <= steady["prep_skipped"], st
    S.took_the_path(steady)


def never_forked(st, on=0):
    fork = st[4]
    assert fork == {"forked": 0, "on": on}, st


# ---- tile and bucket edges: short last tiles, buckets of no and of one string, pieces that do not fill a window ------------------------------

@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("n", [40, 511, 513, 1025])
def test_tile_and_bucket_edges(hip, so, n):
    codes = H.splitmix_bases(n, 24, seed=300 + n)
    forked_where_counted(S.check_job(("edges", n), lambda: hip.HipBwt(so), so, [H.encode_batch_fixed(codes)], env=fork_env(), stats=all_stats))


# ---- strings that end in different rounds: bucket sizes and piece sizes move apart, the $ piece grows ------------------------------------------

@pytest.mark.parametrize("so", [0, 1])
def test_strings_end_at_different_rounds(hip, so):
    forked_where_counted(S.check_job("mixed", lambda: hip.HipBwt(so), so, [H.encode_batch(S.mixed_lengths())], env=fork_env(), stats=all_stats))


# ---- a loaded index: compact old windows, both position widths of k_part<.., FORK> -----------------------------------------------------------

@pytest.mark.parametrize("pos", ["0", "64"])
@pytest.mark.parametrize("so", [1, 2])
def test_second_batch_on_a_loaded_index(hip, so, pos):
    b0, b1 = S.two_batches()
    forked_where_counted(S.check_job("two", lambda: hip.HipBwt(so), so, [b0, b1], env=fork_env(RB2_POS=pos, **S.DENSE), stats=all_stats))


# ---- void in-place rounds behind forked rounds: the side stream is joined before the rollback drains -------------------------------------------

def test_void_round_after_the_state(hip):
    b0, b1 = S.hot_spot_batches()
    st = S.check_job("hot", lambda: hip.HipBwt(1), 1, [b0, b1], env=fork_env(**S.FORCED), stats=all_stats)
    assert st[3]["void_rounds"] > 0 and st[3]["sparse_rounds"] > 0, st
    forked_where_counted(st)


# ---- more than SCHUNK tiles (two blocks of k_count_lean, many blocks of k_part): forked and on one stream, the same index ---------------------

def test_two_chunks(hip):
    n = 530000
    buf = H.encode_batch_fixed(H.splitmix_bases(n, 24, seed=77))

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
    hf, cf, stf = run(fork_env(**S.DENSE))
    h0, c0, st0 = run(fork_env(RB2_LEAN_FORK="0", **S.DENSE))
    forked_where_counted(stf)
    never_forked(st0)
    assert st0[2]["counted"] > 0, st0
    assert hf == h0 and np.array_equal(cf, c0)
    assert int(cf.sum()) == n * 25


# ---- audit rounds and the switches --------------------------------------------------------------------------------------------------------------

def edges_job(hip, env, make=None):
    buf = H.encode_batch_fixed(H.splitmix_bases(1025, 24, seed=300 + 1025))
    return S.check_job(("edges", 1025), make or (lambda: hip.HipBwt(1)), 1, [buf], env=env, stats=all_stats)


def test_every_round_audited(hip):
    st = edges_job(hip, fork_env(RB2_LEAN_AUDIT="1"))
    assert st[1]["rounds"] > 0 and st[2]["counted"] == 0 and st[2]["audit"] == st[1]["rounds"], st
    never_forked(st, on=1)


def test_every_third_round_audited(hip):
    st = edges_job(hip, fork_env(RB2_LEAN_AUDIT="3"))
    assert st[2]["audit"] > 0, st
    forked_where_counted(st)


@pytest.mark.parametrize("env", [{"RB2_LEAN_VERIFY": "1"}, {"RB2_STEADY_LEAN": "1"}, {"RB2_STEADY": "0"}, {"RB2_LEAN_FORK": "0"}])
def test_switched_off(hip, env):
    st = edges_job(hip, dict(fork_env(), **env))
    never_forked(st, on=0 if ("RB2_LEAN_VERIFY" in env or "RB2_LEAN_FORK" in env) else 1)
    if "RB2_LEAN_VERIFY" in env or "RB2_LEAN_FORK" in env:
        assert st[2]["counted"] > 0, st                             # (counted by k_count_lean all the same, on the one stream)


def test_the_one_launch_tail_is_not_forked(hip):
    """few tiles and the default RB2_TS_MAX: the counting tail is k_tscan_setup, a stage-1 round"""
    buf = H.encode_batch_fixed(H.splitmix_bases(1025, 24, seed=300 + 1025))
    st = S.check_job(("edges", 1025), lambda: hip.HipBwt(1), 1, [buf], env=dict(S.K1, RB2_STEADY_LEAN="2"), stats=all_stats)
    assert st[1]["stage"] == 1 and st[1]["rounds"] > 0, st
    never_forked(st, on=1)


def test_a_callers_stream_is_never_forked_from(hip):
    """rb2_hip_use_stream: the rounds run on the caller's stream alone (the side stream is the handle's own and stays idle)"""
    with open("/proc/self/maps") as f:                               # the HIP runtime the engine itself runs on
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    assert paths, "the engine has loaded no HIP runtime"
    rt = ctypes.CDLL(paths[0])
    stream = ctypes.c_void_p()
    assert rt.hipStreamCreate(ctypes.byref(stream)) == 0

    def make():
        g = hip.HipBwt(1)
        g.L.rb2_hip_use_stream(g.h, stream)
        return g
    try:
        st = edges_job(hip, fork_env(), make)                       # (check_job closes the handle: it drains the device, the stream is still there)
    finally:
        assert rt.hipStreamDestroy(stream) == 0
    assert st[2]["counted"] > 0, st
    never_forked(st)
