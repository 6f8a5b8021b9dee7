"""The hostile run streams of tests/fmd_streams.py through the device: rb2_hip_load_ropes (k_ld_*), rb2_hip_save_fmd (k_fmds_*) and
rb2_hip_load_fmd (fmd_runs), one test per stream.  What the streams exercise is asserted on the CPU (tests/test_fmd_streams_ref.py).

  handle A   load_ropes(cut(S)): counts() == counts(S); one rank_batch per rope at every run start, the row before and the row behind
             (2^20 rows at the most) == ranks(S, ..); below 2^27 symbols also rope_rle(b), merged into runs, == the stream, rope by rope
  encoder    A.save_fmd() == the host writer's image, byte for byte, with the default segments and batches, with RB2_FMDS_SEG=96
             RB2_FMDS_BATCH=2048, and with segments of 97 and of 128 runs; rope_hashes() and counts() are what they were.
             Streams with runs of 2^30 and more: the default and RB2_FMDS_SEG=96 only.  A batch of 2048 heads has room for ONE leaf of 1024
             symbols (fmds_encode: avail = (RCAP - ncur - 1) / LEAF), whether the leaf holds a head or not, so a run of 2^30 symbols
             alone would be 2^20 batches of a dozen launches and a wait each: head-less leaves do cost a batch of their own.
  handle B   load_fmd(image) == the symbol total; hashes, counts and the same ranks as A; B.save_fmd() == the image
  handle A'  load_ropes(cut(S, canonical=False)): the hashes and counts of A (include/rb2_hip.h: "any run width")
and, once, an index in the sparse layout.  A mismatch of images names the byte and, through events(), its block, word, run and segment.

Wall time per stream on one MI355X, by the clock around the whole test (CPU model, three handles, the encoder grid), and of the one
encoding with RB2_FMDS_BATCH=2048 in it, which takes a batch (49 us) per leaf of 1024 symbols:

  stream                  runs       symbols    test   of which BATCH=2048
  aligned_1_70_k7_12    520 696     3 099 829   2.5 s   0.26 s
  aligned_k13_15         53 253    16 739 484   1.5 s   0.93 s
  aligned_k16_17         35 502    57 247 848   3.3 s   2.9 s
  aligned_k18            17 751    76 301 364   4.2 s   3.8 s
  aligned_k19a           11 834   101 723 415   5.4 s   5.1 s
  aligned_k19b            5 917    50 861 853   2.8 s   2.5 s
  aligned_k20a, b, c      5 917   101 717 6..   5.4 s   5.1 s     (each)
  ones_2 .. ones_5000                           0.05 - 0.06 s
  ones_300000           300 000       300 000   1.1 s   0.03 s
  types_T_front (18)    310 - 390   2^31 - 2^32 0.26 - 0.57 s     (no BATCH=2048)
  gamma_edge                 23   6 442 450 964 0.64 s            (no BATCH=2048)
  random                 16 000    97 426 496   4.8 s   4.5 s
  test_sparse_layout                            0.85 s

The file: 38 tests in 51 s.  Two streams are smaller than the families of the plan check say, both because of the BATCH=2048 encoding:
the aligned family with k up to 20 is 610 M symbols (30 s) and is spread over nine streams of at most 102 M symbols, none left out; the
random stream has 16 000 runs, not 100 000 (614 M symbols: 30 s by the same 49 us per batch -- computed, not run)."""
import time

import numpy as np
import pytest

import fmd_streams as F
import helpers as H
from fmd_save_ref import fmd_of
from test_fmd_save_gpu import FORCED, SMALL, _Env, same, save_both

pytestmark = pytest.mark.gpu

GRID = [{}, SMALL, dict(RB2_FMDS_SEG="97"), dict(RB2_FMDS_SEG="128")]
GRID_HUGE = [{}, dict(RB2_FMDS_SEG="96")]


def same_image(got, want, what, seg):
    try:
        same(got, want, what)
    except AssertionError as e:
        byte = int(str(e).rsplit(" ", 1)[1])
        raise AssertionError("%s -- %s" % (e, F.locate(want, byte, seg))) from None


def rope_as_runs(g, b):
    """rope b of the handle as maximal runs (l, c): its one-byte codes merged"""
    rle = g.rope_rle(b)
    if len(rle) == 0:
        return []
    c, l = (rle & 7).astype(np.int64), (rle >> 3).astype(np.int64)
    first = np.flatnonzero(np.concatenate([[True], c[1:] != c[:-1]]))
    return list(zip(np.add.reduceat(l, first).tolist(), c[first].tolist()))


@pytest.mark.parametrize("name", F.NAMES)
def test_stream(hip, tmp_path, name):
    t0 = time.time()
    S, want = F.stream(name), F.image(name, tmp_path)
    n = int(F.totals(S).sum())
    R, M = F.Ranks(S), F.counts(S)
    xs = [R.probes(b) for b in range(6)]
    rk = [R.rope(b, xs[b]) for b in range(6)]
    t1 = time.time()

    def ranks_of(g, who):
        for b in range(6):
            if M[b].sum():
                got = g.rank_batch(b, xs[b])
                bad = np.flatnonzero((got != rk[b]).any(axis=1))
                assert len(bad) == 0, "%s %s: rank at row %d of rope %d is %s, not %s" % (name, who, xs[b][bad[0]], b, got[bad[0]], rk[b][bad[0]])

    A = hip.HipBwt(0)
    A.load_ropes(F.cut(S))
    assert np.array_equal(A.counts(), M), name
    ranks_of(A, "A")
    if n < 1 << 27:
        for b, runs in enumerate(F.rope_runs(S)):
            assert rope_as_runs(A, b) == runs, "%s: rope %d" % (name, b)
    hashes = A.rope_hashes()
    t2 = time.time()
    tg = []
    for env in GRID_HUGE if name in F.HUGE else GRID:
        ts = time.time()
        with _Env(**env):
            got = A.save_fmd()
        tg.append(time.time() - ts)
        same_image(got, want, "%s, encoder with %s" % (name, env or "defaults"), int(env.get("RB2_FMDS_SEG", 4096)))
        assert A.rope_hashes() == hashes and np.array_equal(A.counts(), M), "%s: the encoder changed the index (%s)" % (name, env)
    t3 = time.time()
    B = hip.HipBwt(0)
    assert B.load_fmd(want) == n
    assert B.rope_hashes() == hashes and np.array_equal(B.counts(), M), name
    ranks_of(B, "B")
    same_image(B.save_fmd(), want, "%s, loaded from the image and saved" % name, 4096)
    B.close()
    t4 = time.time()
    A2 = hip.HipBwt(0)
    A2.load_ropes(F.cut(S, canonical=False))
    assert A2.rope_hashes() == hashes and np.array_equal(A2.counts(), M), "%s: non-canonical run bytes" % name
    A2.close(); A.close()
    t5 = time.time()
    print("TIMING %s: %d runs, %d symbols, %.2f s: model %.2f, A %.2f, encoder %s, B %.2f, A' %.2f"
          % (name, len(S), n, t5 - t0, t1 - t0, t2 - t1, " ".join("%.2f" % t for t in tg), t4 - t3, t5 - t4))


def test_sparse_layout(hip, tmp_path):
    """the first runs of the random stream (below 2^24 symbols), then one small batch inserted in place: the image of an index in the
    sparse layout is the host writer's image of its ropes"""
    S = F.stream("random")
    S = S[:int(np.searchsorted(np.cumsum([l for l, _ in S]), 1 << 24))]
    assert 1 << 23 < sum(l for l, _ in S) < 1 << 24
    with _Env(**FORCED):
        g = hip.HipBwt(0)
        g.load_ropes(F.cut(S))
        g.insert_multi(H.encode_batch(H.repetitive_reads(150, seed=77, max_len=40), True, True))
        assert g.layout_stats()["sparse_now"]
        hashes = g.rope_hashes()
        got = save_both(g, "sparse")
    same_image(got, fmd_of(g, tmp_path / "sparse.fmd"), "random runs and a batch in place", 4096)
    assert g.rope_hashes() == hashes
    g.close()

