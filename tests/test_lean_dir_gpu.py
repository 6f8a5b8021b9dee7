"""The window directory ("the window directory"; RB2_LEAN_DIR, default 1): a lean round that may write compact windows keeps the
rank directory of the side it writes per window -- k_merge<.., LITE> leaves one record per window and window-relative RKREL, k_meta_win stands in for
k_meta_sb, k_advance<.., LITE> gathers the window's entry.  Every other round (the last of a batch, a round in front of a re-layout, every round that
is not lean) writes the per-leaf directory as before.

The jobs, their environment and the oracle cache are those of tests/test_lean_fork_gpu.py.  Ropes and count matrix are compared with the oracle after
every batch (S.check_job), and so is rank_batch on every rope: the last round of a batch left a full per-leaf directory behind LITE rounds.
rb2_hip_lean_dir_stats says which rounds ran LITE: every lean round that was allowed to write compact windows, and no round at all under
RB2_LEAN_DIR=0, RB2_COMPACT=0 or RB2_STEADY=0 -- each job runs under all four settings.
"""
import os

import numpy as np
import pytest

import helpers as H
import test_steady_round_gpu as S
from test_lean_fork_gpu import fork_env

pytestmark = pytest.mark.gpu

LEAF, WIN, SBSYM = 1024, 4096, 32768


def all_stats(g):
    return {"steady": g.steady_stats(), "lean": g.lean_stats(), "layout": g.layout_stats(), "window": g.window_stats(), "dir": g.lean_dir_stats()}


class RankChecked:
    """the handle S.check_job drives, with rank_batch compared against the oracle's ropes after every batch"""

    def __init__(self, g, want):
        self.g, self.want, self.batch = g, want, 0

    def __getattr__(self, name):
        return getattr(self.g, name)

    def insert_multi(self, buf):
        self.g.insert_multi(buf)
        for b, rope in enumerate(self.want[self.batch][1]):
            n = len(rope)
            xs = np.concatenate([np.linspace(0, n, 500).astype(np.int64)] + [np.arange(k, n + 1, k) + d for k in (LEAF, WIN, SBSYM) for d in (-1, 0, 1)])
            xs = np.unique(xs[(xs >= 0) & (xs <= n)])
            occ = np.concatenate([np.zeros((1, 6), np.int64), np.cumsum(rope[:, None] == np.arange(6)[None, :], axis=0)])
            assert np.array_equal(self.g.rank_batch(b, xs), occ[xs]), "rank_batch on rope %d after batch %d" % (b, self.batch)
        self.batch += 1


def run(key, hip, so, batches, env):
    want = S.oracle_of(key, so, batches)
    return S.check_job(key, lambda: RankChecked(hip.HipBwt(so), want), so, batches, env=env, stats=all_stats)


def lite_where_lean_and_compact(st, nbatches):
    d, lean, lay, win = st["dir"], st["lean"], st["layout"], st["window"]
    assert d["on"] == 1, st
    assert d["rounds"] > 0 and d["rounds"] == d["lean_compact"], st
    # the same from the other counters: a lean round may write compact windows unless it is the last of its batch or hands plain windows to a re-layout
    assert lean["rounds"] - nbatches - lay["plain_handovers"] <= d["rounds"] <= min(lean["rounds"], win["compact_rounds"]), st
    S.took_the_path(st["steady"])


def never_lite(st, on=1):
    assert st["dir"]["rounds"] == 0 and st["dir"]["on"] == on, st


def check_all_settings(key, hip, so, batches, exact=False, **more):
    """the job with the mode on and under each of the three switches that leave no LITE round; exact: one batch on the dense layout, so every lean round
    but the batch's last one runs LITE"""
    st = run(key, hip, so, batches, fork_env(**more))
    lite_where_lean_and_compact(st, len(batches))
    dense_only = st["layout"]["sparse_rounds"] == 0 and st["layout"]["plain_handovers"] == 0
    if exact and dense_only:
        assert st["dir"]["rounds"] == st["lean"]["rounds"] - 1, st
    off = run(key, hip, so, batches, fork_env(RB2_LEAN_DIR="0", **more))
    never_lite(off, on=0)
    assert off["dir"]["lean_compact"] > 0, off
    if dense_only:                                                  # (the same rounds, with the per-leaf directory; when a void in-place round is noticed depends on the host's timing)
        assert off["dir"]["lean_compact"] == st["dir"]["lean_compact"] and off["lean"] == st["lean"] and off["window"] == st["window"], (st, off)
    plain = run(key, hip, so, batches, fork_env(RB2_COMPACT="0", **more))
    never_lite(plain)
    assert plain["dir"]["lean_compact"] == 0 and plain["lean"]["rounds"] > 0, plain
    unsteady = run(key, hip, so, batches, fork_env(RB2_STEADY="0", **more))
    never_lite(unsteady)
    assert unsteady["lean"]["rounds"] == 0, unsteady
    return st


# ---- tile and window edges: more than 64 new symbols per window, windows of one to three leaves, pieces of less than a window ----------------------

@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("n", [40, 511, 513, 1025])
def test_tile_and_window_edges(hip, so, n):
    codes = H.splitmix_bases(n, 24, seed=300 + n)
    check_all_settings(("edges", n), hip, so, [H.encode_batch_fixed(codes)], exact=True)


# ---- strings that end in different rounds: the `$` piece grows, windows fill up leaf by leaf ---------------------------------------------------------

@pytest.mark.parametrize("so", [0, 1])
def test_strings_end_at_different_rounds(hip, so):
    check_all_settings("mixed", hip, so, [H.encode_batch(S.mixed_lengths())], exact=True)


# ---- a loaded index: `$` exceptions in the windows, compact old windows, both position widths of the LITE kernels ---------------------------------

@pytest.mark.parametrize("pos", ["0", "64"])
@pytest.mark.parametrize("so", [1, 2])
def test_second_batch_on_a_loaded_index(hip, so, pos):
    b0, b1 = S.two_batches()
    check_all_settings("two", hip, so, [b0, b1], RB2_POS=pos, **S.DENSE)


# ---- pieces that end just below and just above one superblock: the second superblock of a piece, superblocks of fewer than eight windows -----------

@pytest.mark.parametrize("n", [20000, 26000])
def test_pieces_around_one_superblock(hip, n, so=0):
    """input order: every round but the first few is lean.  20 000 strings: the sixteen large pieces end the batch with ~28 750 symbols, the last windows of
    their one superblock fill up round by round; 26 000 strings: the same pieces pass 32 768 symbols about three rounds before the batch ends"""
    buf = H.encode_batch_fixed(H.splitmix_bases(n, 24, seed=61))
    check_all_settings(("sb", n), hip, so, [buf], exact=True, **S.DENSE)
    acgt = S.oracle_of(("sb", n), so, [buf])[0][0][1:5, 1:5]         # rope x, symbol b: the size of piece (b, x) when the batch is through
    per_round = n // 16 + 200                                       # what such a piece takes per round, generously
    if n == 20000:
        assert SBSYM > acgt.max() > SBSYM - 3 * per_round, acgt       # within three rounds of a full superblock
    else:
        assert acgt.min() - 2 * per_round > SBSYM, acgt              # above one superblock two rounds before the end: in a LITE round


# ---- void in-place rounds and a re-layout behind LITE rounds: the plain hand-over writes a full directory ----------------------------------------

def test_void_rounds_and_relayout_behind_lite_rounds(hip):
    b0, b1 = S.hot_spot_batches()
    st = check_all_settings("hot", hip, 1, [b0, b1], **S.FORCED)
    assert st["layout"]["void_rounds"] > 0 and st["layout"]["sparse_rounds"] > 0 and st["layout"]["plain_handovers"] > 0, st


# ---- more than SCHUNK tiles, pieces of many superblocks: with and without the window directory, the same index ------------------------------------

def test_two_chunks_same_index_with_and_without(hip):
    n = 530000
    buf = H.encode_batch_fixed(H.splitmix_bases(n, 24, seed=77))

    def one(env):
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
    h1, c1, st1 = one(fork_env(RB2_LEAN_DIR="1", **S.DENSE))
    h0, c0, st0 = one(fork_env(RB2_LEAN_DIR="0", **S.DENSE))
    lite_where_lean_and_compact(st1, 1)
    never_lite(st0, on=0)
    assert st0["dir"]["lean_compact"] == st1["dir"]["lean_compact"] > 0, (st0, st1)
    assert h1 == h0 and np.array_equal(c1, c0)
    assert int(c1.sum()) == n * 25
