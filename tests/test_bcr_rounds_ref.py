"""The per-round numpy model (bcr_rounds_ref.py) against the oracle, its per-window figures against a count by hand, and the coverage
the designed inputs of compact_edge_jobs.py reach -- all without a GPU."""
import numpy as np
import pytest

import bcr_rounds_ref as R
import compact_edge_jobs as J
import helpers as H


def _against_oracle(batches):
    m, o = R.RoundsModel(), H.Oracle(0)
    for buf in batches:
        o.insert_multi(buf)
        m.insert_multi(buf)
        assert np.array_equal(m.bwt, o.bwt())
        assert np.array_equal(m.matrix(), o.counts())
    return m


@pytest.mark.parametrize("cuts", [(1500, 3000), (1000, 1800, 3000)])
def test_repetitive_reads(cuts):
    rr = H.repetitive_reads(3000)
    _against_oracle([H.encode_batch(rr[a:b]) for a, b in zip((0,) + cuts, cuts)])


@pytest.mark.parametrize("cuts", [(9000, 15000), (4096, 8192, 15000)])
def test_fixed_length_random_reads(cuts):
    b = H.splitmix_bases(15000, 37, seed=3)
    _against_oracle([H.encode_batch_fixed(b[a:c]) for a, c in zip((0,) + cuts, cuts)])


@pytest.mark.parametrize("nb", [2, 3])
def test_mixed_lengths_with_empty_strings(nb):
    rng = np.random.default_rng(77)
    batches = []
    for k in range(nb):
        reads = [rng.integers(1, 6, size=int(n)).astype(np.uint8) for n in rng.integers(0, 50, size=2500)]
        reads[0] = reads[7] = reads[-1] = np.zeros(0, np.uint8)
        batches.append(H.encode_batch(reads))
    batches.append(H.encode_batch([np.zeros(0, np.uint8)] * 3))    # a batch of nothing but empty strings: one round, no compact one
    m = _against_oracle(batches)
    assert m.stats["compact_rounds"] == sum(int(R.split_batch(b)[1].max()) for b in batches)


def test_format_thresholds():
    assert list(R.format_of([0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 4096])) == [R.C0] + [R.C1] * 3 + [R.C2] * 4 + [R.PLAIN] * 3


def test_window_figures_by_hand():
    """every figure of a Round that the coverage conditions rest on, counted again window by window from the two arrays"""
    rng = np.random.default_rng(5)
    reads = [rng.choice(np.array([1, 2, 5], np.uint8), size=int(n), p=[0.55, 0.43, 0.02]) for n in rng.integers(0, 14, size=9000)]
    m, rounds = R.RoundsModel(), []
    fmts = [np.zeros(0, np.uint8)] * R.NR
    for buf in (H.encode_batch(reads[:6000]), H.encode_batch(reads[6000:])):
        for rd in m.rounds(buf):
            new = m.bwt
            exc_old = (rd.old == 0) | (rd.old == 5)
            seen = 0
            for w in range(len(rd.piece)):
                p, j = int(rd.piece[w]), int(rd.j[w])
                lo = int(rd.start[p]) + j * R.WIN
                hi = min(lo + R.WIN, int(rd.start[p + 1]))
                assert hi > lo and rd.nvalid[w] == hi - lo
                sym, isn = new[lo:hi], rd.isnew[lo:hi]
                assert rd.xt[w] == ((sym == 0) | (sym == 5)).sum() and rd.ni[w] == isn.sum()
                assert rd.new_x[w] == (((sym == 0) | (sym == 5)) & isn).sum()
                i0 = j * R.WIN - int(rd.isnew[rd.start[p]:lo].sum())
                assert rd.i0[w] == i0 and rd.g0[w] == (i0 >> 6) & 63 and rd.sh0[w] == i0 & 63
                nold = hi - lo - int(rd.ni[w])
                op0, on = int(rd.old_start[p]), int(rd.old_start[p + 1] - rd.old_start[p])
                assert 0 <= i0 and i0 + nold <= on
                assert np.array_equal(sym[~isn], rd.old[op0 + i0:op0 + i0 + nold])       # the old symbols it takes are those from i0 on
                ow, g0 = i0 >> 12, (i0 >> 6) & 63
                assert rd.two[w] == (nold > 0 and (i0 + nold - 1) >> 12 > ow)
                assert rd.nwg[w] == (((i0 + nold - 1) >> 6) - (i0 >> 6) + 1 if nold else 0)
                for h, ln, k in ((rd.h0[w], rd.len0[w], ow), (rd.h1[w], rd.len1[w], ow + 1)):
                    if k * R.WIN < on:
                        x = exc_old[op0 + k * R.WIN:op0 + min((k + 1) * R.WIN, on)].sum()
                        assert h == fmts[p][k] and ln == x
                    else:
                        assert h == R.NONE and ln == -1
                if nold:
                    assert rd.x_front[w] == exc_old[op0 + ow * R.WIN:op0 + min(ow * R.WIN + g0 * 64, on)].sum()
                if rd.two[w]:
                    assert rd.x_behind[w] == exc_old[op0 + min((ow + 1) * R.WIN + (g0 + 1) * 64, on):op0 + min((ow + 2) * R.WIN, on)].sum()
                if rd.nwg[w] == 65:
                    assert rd.x_tail[w] == exc_old[op0 + min((ow + 1) * R.WIN + g0 * 64, on):op0 + min((ow + 1) * R.WIN + (g0 + 1) * 64, on)].sum()
                    seen += 1
                assert rd.fmt[w] == (R.format_of(rd.xt[w]) if rd.compact else R.PLAIN)
            fmts = [rd.fmt[rd.piece == p] for p in range(R.NR)]
            rounds.append(seen)
    assert sum(rounds) > 0                                         # (stages of 65 groups were among them)


def test_designed_windows_hold_what_they_were_designed_to_hold():
    """what compact_edge_jobs.py rests on: rope `$`, piece (A,$) and the rows `GCA$` of piece (G,C) take their symbols in read order"""
    m = R.RoundsModel()
    for rd in m.rounds(J.job("designed")[0]):
        for piece, first_round, want in ((0, 0, J.EDGE_COUNTS), (H.rope_of(1, 0), 1, J.EDGE_COUNTS), (H.rope_of(3, 2), 3, J.PAIR_COUNTS)):
            if rd.r >= first_round:
                sel = rd.piece == piece
                assert list(rd.xt[sel][:len(want)]) == want, (rd.r, piece)
                assert (rd.i0[sel][:len(want)] % R.WIN == 0).all()   # nothing is ever inserted in front of them in this batch


def test_designed_jobs_reach_every_case():
    """the coverage condition of tests/test_compact_edges_gpu.py, from the model alone: no case may be missing"""
    cov = R.Coverage()
    for name in J.JOBS:
        m = R.RoundsModel()
        for buf in J.job(name):
            m.insert_multi(buf, cov.add)
    assert cov.missing() == []


def test_compact_off_counts_plain_windows_only():
    m = R.RoundsModel(compact=False)
    for buf in J.job("graded"):
        m.insert_multi(buf)
    st = m.stats
    assert st["compact_rounds"] == 0 and st["compact0"] + st["compact1"] + st["compact2"] == 0 and st["plain"] > 0
