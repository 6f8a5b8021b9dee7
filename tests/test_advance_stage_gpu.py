"""k_advance's staged stores: the plain path (one engine, dense rounds) lays a tile's strings down in LDS run by run and writes whole
runs.  What can go wrong is the order inside the tile -- run starts, empty runs, strings that finish (not staged), a last tile with
one string -- so every job below is small, is built around one of those, and compares the six ropes and the 6x6 count matrix with
the oracle after EVERY batch.  The sharded branches of the kernel (PEER) keep the direct scatter and are run against the same oracle.
"""
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu


def check_job(make, so, batches, env=None, before=None):
    """insert the batches into make() and into the oracle; ropes and counts after every batch (before: what the oracle inserts first,
    for an index that make() loads)"""
    env = env or {}
    o = H.Oracle(so)
    if before is not None:
        o.insert_multi(before)
    os.environ.update(env)
    try:
        g = make()
        for i, buf in enumerate(batches):
            o.insert_multi(buf)
            g.insert_multi(buf)
            assert np.array_equal(o.counts(), g.counts()), "count matrix differs after batch %d" % i
            for b in range(6):
                ro, rg = o.rope(b), g.rope(b)
                assert len(ro) == len(rg), "rope %d length after batch %d" % (b, i)
                assert np.array_equal(ro, rg), "rope %d differs after batch %d at %s" % (b, i, np.flatnonzero(ro != rg)[:5])
    finally:
        for k in env:
            del os.environ[k]
    g.close()


def skewed_reads(n, length, major, seed):
    """random reads with symbol `major` at 97 %, the other five symbols of 1..5 sharing the rest"""
    rng = np.random.RandomState(seed)
    other = np.array([s for s in range(1, 6) if s != major], np.uint8)
    r = np.where(rng.rand(n, length) < 0.97, np.uint8(major), other[rng.randint(0, 4, size=(n, length))]).astype(np.uint8)
    return r


# ---- tile shapes: a last tile with one string (513, 1025: tiles of 512), a tile one short of full --------------------------------

@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("n", [511, 513, 1025])
def test_last_tile(hip, so, n):
    codes = H.splitmix_bases(n, 20, seed=90 + n)
    check_job(lambda: hip.HipBwt(so), so, [H.encode_batch_fixed(codes)])


# ---- symbol mixes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("so", [0, 1, 2])
def test_identical_homopolymers(hip, so):
    """every read A...A: one run of 512 per tile, the other runs empty; one group per bucket (the non-speculative path)"""
    check_job(lambda: hip.HipBwt(so), so, [H.encode_batch([[1] * 20] * 1100), H.encode_batch([[1] * 20] * 513)])


@pytest.mark.parametrize("so", [0, 1, 2])
def test_only_n(hip, so):
    """symbol 5 only: the last run, every run in front of it empty"""
    check_job(lambda: hip.HipBwt(so), so, [H.encode_batch([[5] * 17] * 700 + [[5] * 3] * 350)])


@pytest.mark.parametrize("so", [0, 1, 2])
def test_mixed_lengths(hip, so):
    """lengths 1..40: strings finish in every round (they insert the sentinel and are not staged), so the tile's record count
    falls below its string count in every round"""
    rng = np.random.RandomState(17 + so)
    reads = [rng.randint(1, 5, size=1 + i % 40).astype(np.uint8) for i in range(1400)]
    check_job(lambda: hip.HipBwt(so), so, [H.encode_batch(reads[:900]), H.encode_batch(reads[900:], True, True)])


@pytest.mark.parametrize("major", [1, 2, 3, 4, 5])
def test_skewed_composition(hip, major):
    """3 000 reads, one symbol at 97 %: its run crosses several 128-byte lines of every array, the other runs hold 0-2 strings"""
    codes = skewed_reads(3000, 24, major, seed=major)
    check_job(lambda: hip.HipBwt(1), 1, [H.encode_batch_fixed(codes)])


# ---- both instantiations, both widths, the untouched branches -------------------------------------------------------------------

@pytest.mark.parametrize("so", [0, 2])
@pytest.mark.parametrize("dense", [True, False])
def test_two_batches_on_a_loaded_index(hip, so, dense):
    """repetitive reads on top of a loaded index: intervals stay non-empty for many rounds (k_advance<false>: U is staged too).
    dense: the engine never leaves the dense layout (RB2_SPARSE_LAMBDA=0); else its own choice of in-place rounds, which keep the
    direct scatter"""
    from ropebwt2_amd.hipbwt import encode_runs
    reads = H.repetitive_reads(2600, seed=40 + so, genome_len=500, max_len=60)
    first = H.Oracle(so)
    first.insert_multi(H.encode_batch(reads[:1200]))
    ropes = [encode_runs(first.rope(b)) for b in range(6)]

    def make():
        g = hip.HipBwt(so)
        g.load_ropes(ropes)
        return g
    # the oracle is given the first batch as a batch of its own: batch 0 of the comparison is the loaded index itself
    batches = [H.encode_batch(reads[1200:1900]), H.encode_batch(reads[1900:], True, True)]
    check_job(make, so, batches, env={"RB2_SPARSE_LAMBDA": "0"} if dense else {}, before=H.encode_batch(reads[:1200]))


@pytest.mark.parametrize("so", [0, 1, 2])
def test_64_bit_positions(hip, so):
    """RB2_POS=64: positions never stored in 32 bits (the staged records of l and u are 8 bytes each)"""
    reads = H.repetitive_reads(1500, seed=70 + so, genome_len=400, max_len=50)
    codes = skewed_reads(1300, 30, 2, seed=9)
    check_job(lambda: hip.HipBwt(so), so, [H.encode_batch(reads), H.encode_batch_fixed(codes)], env={"RB2_POS": "64", "RB2_SPARSE_LAMBDA": "0"})


@pytest.mark.parametrize("so", [0, 2])
def test_two_peer_ranks_agree(hip, so):
    """two virtual ranks on one device over the PEER transport: k_advance's push branch, which is not staged"""
    from ropebwt2_amd import MultiBwt
    reads = H.repetitive_reads(1500, seed=80 + so, genome_len=400, max_len=50)
    codes = H.splitmix_bases(1025, 20, seed=8)
    check_job(lambda: MultiBwt(so, [0, 0], "peer"), so, [H.encode_batch(reads), H.encode_batch_fixed(codes)])
