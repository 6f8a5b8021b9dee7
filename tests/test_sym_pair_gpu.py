"""k_sym takes two string tiles per block on one engine.  What can go wrong is per-tile state inside a pair -- a second tile that does
not exist, a pair that straddles two buckets, a partial last tile, the string behind the pair's inner boundary, a group that crosses
it, one tile of a pair finished by k_sym itself (TILE_DONE) and the other left to k_prep.  Every job is small and built around one of
those; the six ropes and the 6 x 6 matrix are compared with the oracle after EVERY batch, once with the many-tiles counting tail
forced (RB2_TS_MAX=2: k_tscan1/3 + k_tfix read the tile records the pairs wrote) and once with the single-launch tail (k_tscan_setup).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from bcr_rounds_ref import RoundsModel

pytestmark = pytest.mark.gpu
STILE = 512
TAILS = [{"RB2_TS_MAX": "2"}, {}]
TAIL_IDS = ["tfix", "tscan_setup"]


def check_job(make, so, batches, env=None):
    """insert the batches into make() and into the oracle; ropes and counts after every batch.  Returns the engine (open)."""
    env = dict(env or {})
    old = {k: os.environ.get(k) for k in env}
    o = H.Oracle(so)
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
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    return g


def batch_of(syms):
    """the batch buffer of equally long reads given as the symbols they insert, round by round (row k = read k, column r = round r)"""
    a = np.asarray(syms, np.uint8)
    return np.concatenate([a, np.zeros((len(a), 1), np.uint8)], axis=1).reshape(-1)


# ---- tile-count edges -----------------------------------------------------------------------------------------------------------
# Round 2 of a batch sorts the strings into buckets by the symbols of rounds 0 and 1, so the number of reads that start (in insertion
# order) with a given pair IS a bucket size of round 2 -- whatever the sorting order, buckets depend on the symbols alone.
EDGE_SIZES = [({(1, 1): 1, (1, 2): 511, (1, 3): 512, (1, 4): 513, (2, 3): 1025}), ({(2, 1): 1023, (2, 2): 1024, (2, 4): 1537})]


def edge_batches():
    rng = np.random.RandomState(8)
    out = []
    for sizes in EDGE_SIZES:
        rows = []
        for (a0, a1), n in sizes.items():
            r = rng.randint(1, 5, size=(n, 24)).astype(np.uint8)
            r[:, 0], r[:, 1] = a0, a1
            rows.append(r)
        rows = np.concatenate(rows)
        out.append(batch_of(rows[rng.permutation(len(rows))]))
    return out


@pytest.fixture(scope="module")
def edge_job():
    """the two batches + what the model says about their rounds: the bucket sizes seen and the tile counts per round"""
    bufs = edge_batches()
    m = RoundsModel()
    sizes, ntiles = set(), []
    for buf in bufs:
        for rd in m.rounds(buf):
            ins = np.asarray(rd.ins)
            sizes.update(int(x) for x in ins if x)
            ntiles.append(int(((ins + STILE - 1) // STILE).sum()))
    return bufs, sizes, ntiles


def test_edge_job_has_the_shapes(edge_job):
    _, sizes, ntiles = edge_job
    for n in (1, 511, 512, 513, 1023, 1024, 1025, 1537):
        assert n in sizes, "no bucket of %d strings in any round" % n
    assert any(t % 2 == 1 and t > 1 for t in ntiles), "no round with an odd tile count: the second tile of the last block is never missing"
    assert any(t % 2 == 0 for t in ntiles)


@pytest.mark.parametrize("env", TAILS, ids=TAIL_IDS)
@pytest.mark.parametrize("so", [0, 1])
def test_tile_count_edges(hip, edge_job, so, env):
    """input order and RLO, two batches: the second runs on a loaded index (RLO: rounds with non-empty intervals, then all-empty ones)"""
    check_job(lambda: hip.HipBwt(so), so, edge_job[0], env=env).close()


# ---- groups across the pair -----------------------------------------------------------------------------------------------------

def group_reads():
    """2000 random reads of 24 whose symbols of rounds 10 and 11 are all A: round 12 has ONE bucket of all strings (tiles 0-3: a pair 0|1 and a
    pair 2|3), in RLO ordered by the symbols of rounds 9 .. 0.  The read at rank 500 of that order is there 40 times: ranks 500 .. 539, across
    the inner boundary of the first pair (512).  Returns the reads (shuffled) and the rank of the group's first member in round 12."""
    rng = np.random.RandomState(21)
    r = rng.randint(1, 5, size=(2000, 24)).astype(np.uint8)
    r[:, 10] = 1; r[:, 11] = 1
    key = lambda a: [tuple(int(x) for x in row[9::-1]) for row in a]
    order = sorted(range(len(r)), key=lambda k: key(r[k:k + 1])[0])
    dup = r[order[500]]
    allr = np.concatenate([r, np.tile(dup, (39, 1))])
    allr = allr[rng.permutation(len(allr))]
    keys = key(allr)
    kd = key(dup[None])[0]
    first = sum(k < kd for k in keys)
    assert sum(k == kd for k in keys) == 40
    return allr, first


@pytest.mark.parametrize("env", TAILS, ids=TAIL_IDS)
def test_group_across_the_pair(hip, env):
    reads, first = group_reads()
    assert first // STILE == 0 and (first + 39) // STILE == 1, "the group of 40 does not cross the boundary between tiles 0 and 1 (rank %d)" % first
    # a second batch on the loaded index: the same reads again, every interval non-empty at first
    check_job(lambda: hip.HipBwt(1), 1, [batch_of(reads), batch_of(reads[:1100])], env=env).close()


@pytest.mark.parametrize("env", TAILS, ids=TAIL_IDS)
def test_all_reads_identical(hip, env):
    """no tile is ever all-single: k_sym finishes no tile, every tile of every round is left to k_prep (2000 strings: four tiles, two pairs)"""
    rng = np.random.RandomState(3)
    one = rng.randint(1, 5, size=24).astype(np.uint8)
    check_job(lambda: hip.HipBwt(1), 1, [batch_of(np.tile(one, (2000, 1)))], env=env).close()


# ---- which tiles k_sym finishes itself: all of them, all but one ---------------------------------------------------------------

@pytest.mark.parametrize("env", TAILS, ids=TAIL_IDS)
def test_every_tile_done(hip, env):
    """random reads in RLO on an empty index: all-empty rounds, and from some round on every string is a group of its own -- k_sym finishes every tile"""
    codes = H.splitmix_bases(5000, 24, seed=31)
    check_job(lambda: hip.HipBwt(1), 1, [H.encode_batch_fixed(codes)], env=env).close()


@pytest.mark.parametrize("env", TAILS, ids=TAIL_IDS)
def test_one_tile_not_done(hip, env):
    """one read is there twice among 5000 random ones: in the late rounds exactly one tile of many holds a group of two -- its partner in the pair is
    finished by k_sym, it is not"""
    codes = H.splitmix_bases(5000, 24, seed=32)
    codes = np.concatenate([codes, codes[1234:1235]])
    check_job(lambda: hip.HipBwt(1), 1, [H.encode_batch_fixed(codes)], env=env).close()


# ---- the neighbour instantiations keep one tile per trip ---------------------------------------------------------------------------

@pytest.mark.parametrize("so", [0, 1])
def test_two_virtual_ranks(hip, edge_job, so):
    """k_sym<STRIDE>: one tile per trip"""
    from ropebwt2_amd import MultiBwt
    check_job(lambda: MultiBwt(so, [0, 0], "peer"), so, edge_job[0]).close()


@pytest.mark.parametrize("env", TAILS, ids=TAIL_IDS)
@pytest.mark.parametrize("so", [0, 1])
def test_forced_in_place_rounds(hip, edge_job, so, env):
    """every round in place where it can be: the counting phase rides behind the round before (k_sym<SPLIT>: one tile per block)"""
    e = dict(env); e.update({"RB2_SPARSE_LAMBDA": "1e18", "RB2_SPARSE_MAXPEN": "0"})
    check_job(lambda: hip.HipBwt(so), so, edge_job[0], env=e).close()


# ---- the build switch ---------------------------------------------------------------------------------------------------------------

CHILD = """
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_sym_pair_gpu as T
from ropebwt2_amd import HipBwt
g = HipBwt(1)
for buf in T.edge_batches(): g.insert_multi(buf)
print('HASH', g.counts().reshape(-1).tolist(), g.rope_hashes())
"""


def test_one_tile_per_block_build(hip, edge_job):
    """a library built with -DRB2_SYM_PAIR=0 (tools/build_variant.sh nopair -DRB2_SYM_PAIR=0) gives the same ropes.  Building one takes about a
    minute, too long for a test: it runs where the variant library is already there."""
    from ropebwt2_amd.build import lib_path
    var = lib_path("librb2hip_nopair.so")
    if not os.path.exists(var):
        pytest.skip("no ropebwt2_amd/lib/librb2hip_nopair.so (tools/build_variant.sh nopair -DRB2_SYM_PAIR=0; a build takes a minute)")
    g = hip.HipBwt(1)
    for buf in edge_job[0]:
        g.insert_multi(buf)
    want = "HASH %s %s" % (g.counts().reshape(-1).tolist(), g.rope_hashes())
    g.close()
    env = dict(os.environ, RB2_HIP_LIB=var)
    p = subprocess.run([sys.executable, "-c", CHILD % (H.ROOT, os.path.dirname(os.path.abspath(__file__)))], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = [l for l in p.stdout.splitlines() if l.startswith("HASH")]
    assert got == [want]
