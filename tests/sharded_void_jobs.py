"""Jobs for the void in-place rounds of a sharded index (tests/test_sharded_inplace_gpu.py), and where their inserts land.

Which piece a string inserts into depends only on its own symbols, never on the sorting order (bcr_rounds_ref.py): with a_k the k-th
symbol it inserts (last symbol first), round 0 inserts into rope `$` (sub-rope 0), round 1 into piece (a_0, `$`) and round r >= 2 into
piece (a_{r-1}, a_{r-2}), sub-rope 1 + (b - 1) * 6 + x (include/rb2_hip.h).  So which rank takes how many inserts in which round follows
from a batch buffer and an owner map alone; tests/test_sharded_void_jobs.py proves on the CPU what the GPU tests rely on.

The mixed void batch: 5000 identical strings (test_inplace_paths_gpu._dups, 40 symbols) and 3000 random strings of the same length,
in one batch, on top of fixture a's 2000 x 120 base batch; then one more random batch.  void_owner_map gives rank 0 rope `$` and every
piece the identical strings touch -- their 5000 inserts of a round go to one place of one piece, more than a leaf holds, so every
in-place round of rank 0 there is void -- and deals the pieces the random strings reach out to ranks 1 .. n-1, which take their inserts
in place in the same rounds.
"""
import numpy as np

import helpers as H
from bcr_rounds_ref import NR, split_batch
from test_inplace_paths_gpu import _dups, fixture_a

LEAF = 1024                                     # symbols per leaf (rb2_device.h LEAF)
DUP_LEN = 40
N_DUPS, N_RANDOM = 5000, 3000


def base_batch():
    return fixture_a(DUP_LEN)[0][0]             # 2000 x 120 bp


def mixed_batch():
    return np.concatenate([H.encode_batch([_dups(DUP_LEN)] * N_DUPS), H.encode_batch_fixed(H.splitmix_bases(N_RANDOM, DUP_LEN, seed=31))])


def tail_batch():
    return H.encode_batch_fixed(H.splitmix_bases(2500, 90, seed=32))


def mixed_job():
    """the batches of the mixed void job; the mixed batch is the second"""
    return [base_batch(), mixed_batch(), tail_batch()]


def pieces_touched(buf):
    """ins[r, p]: the inserts sub-rope p receives in round r of the batch buffer buf (one row per round, max_len + 1 rows)"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    starts, lens = split_batch(buf)
    rounds = int(lens.max()) + 1 if len(lens) else 0
    ins = np.zeros((rounds, NR), np.int64)
    for r in range(rounds):
        s = starts[lens >= r]                   # strings still running: round r inserts their symbol r (their `$` when r == length)
        if r == 0:
            pc = np.zeros(len(s), np.int64)
        elif r == 1:
            pc = 1 + (buf[s].astype(np.int64) - 1) * 6
        else:
            pc = 1 + (buf[s + r - 1].astype(np.int64) - 1) * 6 + buf[s + r - 2]
        ins[r] = np.bincount(pc, minlength=NR)
    return ins


def split_dups(buf):
    """(the strings of buf that occur more than once, the others), each as a batch buffer"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    starts, lens = split_batch(buf)
    strs = [bytes(buf[s:s + n + 1]) for s, n in zip(starts.tolist(), lens.tolist())]
    seen = {}
    for s in strs:
        seen[s] = seen.get(s, 0) + 1
    dup = b"".join(s for s in strs if seen[s] > 1)
    rest = b"".join(s for s in strs if seen[s] == 1)
    return np.frombuffer(dup, np.uint8), np.frombuffer(rest, np.uint8)


def void_owner_map(batch, n):
    """rank 0: rope `$` and every piece the identical strings of batch touch; ranks 1 .. n-1, round-robin: the pieces (b, x), b and x
    in A..T, that the other strings reach in rounds >= 2; then the `$` and `N` pieces (and anything left), round-robin behind them"""
    own = [0] * NR
    if n == 1:
        return own
    dup, rnd = split_dups(batch)
    rank0 = set(np.flatnonzero(pieces_touched(dup).sum(0)).tolist()) | {0}
    reach = pieces_touched(rnd)[2:].sum(0)
    acgt = [H.rope_of(b, x) for b in range(1, 5) for x in range(1, 5)]
    order = [p for p in acgt if reach[p] > 0 and p not in rank0]
    order += [p for p in range(1, NR) if p not in rank0 and p not in order]
    for k, p in enumerate(order):
        own[p] = 1 + k % (n - 1)
    return own


def inserts_per_rank(ins, owner, n):
    """per round (the rows of pieces_touched): the inserts every rank receives"""
    out = np.zeros((ins.shape[0], n), np.int64)
    for p in range(NR):
        out[:, owner[p]] += ins[:, p]
    return out
