"""What the jobs of tests/test_sharded_inplace_gpu.py reach, proved without a GPU (tests/sharded_void_jobs.py): which sub-rope -- and so
which rank of an owner map -- receives how many inserts in every round of a batch."""
import numpy as np
import pytest

import bcr_rounds_ref as R
import helpers as H
import sharded_void_jobs as J


def test_pieces_touched_matches_the_rounds_model():
    """pieces_touched (from the buffer alone) against the inserts the round model (so = 0) counts per piece, on a small job: repetitive
    reads with N, empty strings and both strands, then a small mixed batch of identical and random strings"""
    bufs = [H.encode_batch(H.repetitive_reads(300, seed=12, genome_len=200, max_len=30), True, True),
            np.concatenate([H.encode_batch([J._dups(J.DUP_LEN)] * 40), H.encode_batch_fixed(H.splitmix_bases(30, J.DUP_LEN, seed=3))])]
    m = R.RoundsModel()
    for i, buf in enumerate(bufs):
        want = J.pieces_touched(buf)
        got = [rd.ins for rd in m.rounds(buf)]
        assert len(got) == len(want), (i, len(got), len(want))
        for r, ins in enumerate(got):
            assert np.array_equal(ins, want[r]), (i, r, ins, want[r])


@pytest.fixture(scope="module")
def mixed():
    buf = J.mixed_batch()
    dup, rnd = J.split_dups(buf)
    return buf, J.pieces_touched(buf), J.pieces_touched(dup), J.pieces_touched(rnd)


def test_mixed_batch_shape(mixed):
    """the identical and the random strings all run DUP_LEN + 1 rounds; rounds 0 and 1 reach only rope `$` and the pieces (a, `$`)"""
    buf, ins, dup, rnd = mixed
    assert ins.shape == dup.shape == rnd.shape == (J.DUP_LEN + 1, R.NR)
    assert (dup.sum(1) == J.N_DUPS).all() and (rnd.sum(1) == J.N_RANDOM).all()
    assert np.flatnonzero(ins[0]).tolist() == [0]
    assert set(np.flatnonzero(ins[1]).tolist()) <= {H.rope_of(a, 0) for a in range(1, 5)}


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_identical_strings_insert_on_rank_0_only(mixed, n):
    """(i) every insert of an identical string lands on rank 0; (iii) in every round all 5000 of them land in ONE piece of rank 0 --
    more than a leaf holds"""
    buf, ins, dup, rnd = mixed
    own = J.void_owner_map(buf, n)
    assert len(own) == R.NR and own[0] == 0 and max(own) < n
    per = J.inserts_per_rank(dup, own, n)
    assert (per[:, 1:] == 0).all(), per
    assert (per[:, 0] == J.N_DUPS).all(), per[:, 0]
    assert (dup.max(1) == J.N_DUPS).all() and J.N_DUPS > J.LEAF


@pytest.mark.parametrize("n", [2, 3, 8])
def test_every_other_rank_has_inserts_in_every_round_from_2(mixed, n):
    """(ii) in every round r >= 2 of the mixed batch each rank 1 .. n-1 receives inserts (of random strings, by (i)): it takes its round
    in place while rank 0 is void"""
    buf, ins, dup, rnd = mixed
    own = J.void_owner_map(buf, n)
    per = J.inserts_per_rank(ins, own, n)
    print("n %d: fewest inserts per round on ranks 1..n-1: %s" % (n, per[2:, 1:].min(0).tolist()))
    assert (per[2:, 1:] > 0).all(), per[2:, 1:]
    assert len(set(own[p] for p in range(1, R.NR))) == n          # every rank owns a piece
