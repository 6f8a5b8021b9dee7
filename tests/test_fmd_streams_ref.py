"""The run streams of tests/fmd_streams.py on the CPU: the host writer's image of every stream decodes to the stream, the six ropes
cut from it hold its symbols in canonical and in non-canonical run bytes, the rank model agrees with a count by hand -- and the images
exercise what tests/test_fmd_streams_gpu.py is there for.  Those coverage conditions are computed from the reference images alone
(fmd_streams.events over fmd_ref.decode), so that an edit of a generator cannot quietly empty the GPU test."""
import numpy as np
import pytest

import fmd_streams as F


@pytest.fixture(scope="module")
def ev(tmp_path_factory):
    """events of every stream's image at seg = 96, batch = 2048 (decoded once)"""
    tmp = tmp_path_factory.mktemp("fmd_streams")
    return {n: F.events(F.image(n, tmp)) for n in F.NAMES}


@pytest.mark.parametrize("name", F.NAMES)
def test_image_decodes_to_the_stream(ev, name):
    S, E = F.stream(name), ev[name]
    assert max(l for l, _ in S) < F.RUN_MAX
    assert E["runs"] == S, "the image does not hold the runs of the stream"
    assert list(E["mcnt"]) == F.totals(S).tolist()
    assert sum(n for _, n, _ in E["blocks"]) == len(S), "a maximal run is one code"


@pytest.mark.parametrize("name", F.NAMES)
def test_cut_holds_the_symbols_of_the_stream(name):
    S = F.stream(name)
    C, M = F.borders(S), F.counts(S)
    assert M.sum(axis=0).tolist() == F.totals(S).tolist() and M.sum(axis=1).tolist() == np.diff(C).tolist()   # what rb2_hip_load_ropes requires
    for canonical in (True, False):
        ropes = F.cut(S, canonical=canonical)
        codes = [F.decode43(r) for r in ropes]
        assert all(l >= 1 and c <= 5 for rs in codes for l, c in rs)
        assert [sum(l for l, _ in rs) for rs in codes] == np.diff(C).tolist()
        assert F.merge([x for rs in codes for x in rs]) == S
        if canonical:
            assert all(F.merge(rs) == rs for rs in codes), "canonical: neighbouring codes differ"
            assert all(len(r) == sum(F.min_width(l) for l, _ in rs) for r, rs in zip(ropes, codes)), "canonical: least widths"
        elif len(S) >= 90:
            n = sum(len(rs) for rs in codes)
            wide = sum(len(r) for r in ropes) > sum(F.min_width(l) for rs in codes for l, _ in rs)
            assert wide, "non-canonical: wide codes"
            assert n > len(S) + 6 or sum(l >= 2 for l, _ in S) < 50, "non-canonical: split runs"


def test_non_canonical_bytes_use_every_width_for_short_runs():
    seen = set()
    for r in F.cut(F.stream("random"), canonical=False):
        i, r = 0, bytes(r)
        while i < len(r):
            h = r[i]
            n = 1 if h < 0x80 else 2 if h >> 5 == 6 else 4 if h >> 4 == 14 else 8
            l = F.decode43(r[i:i + n])[0][0]
            if l <= 3:
                seen.add(n)
            i += n
    assert seen == {1, 2, 4, 8}


def test_rank_model_against_a_count_by_hand():
    S = F.stream("random")[:300]
    sym = np.repeat([c for _, c in S], [l for l, _ in S])
    C, R = F.borders(S), F.Ranks(S)
    for b in range(6):
        xs = R.probes(b)
        rope = sym[C[b]:C[b + 1]]
        pre = np.concatenate([np.zeros((1, 6), np.int64), np.cumsum(rope[:, None] == np.arange(6), axis=0)])
        assert np.array_equal(F.ranks(S, b, xs), pre[xs])
        assert xs[0] == 0 and xs[-1] == len(rope)
    assert np.array_equal(F.counts(S), [[int((sym[C[b]:C[b + 1]] == a).sum()) for a in range(6)] for b in range(6)])


def test_the_images_exercise_the_encoder_and_the_loaders(ev):
    tally = {k: sum(int(E[k]) for E in ev.values()) for k in ("word_end", "bit_before", "exact", "refused_exact")}
    trans = sum(E["trans"] for E in ev.values())
    totals = {k: sum(E["totals"][k] for E in ev.values()) for k in (16383, 16384, (1 << 30) - 1, 1 << 30)}
    print("events", tally)
    print("transitions", trans.tolist())
    print("totals", totals)
    # A code ends on a block's last bit only from u == C - 64 (the fit rule, csrc/rb2_fmd_plan.h), so it is 64 bits wide: a run of 2^50
    # symbols and more.  Below 2^32 a code has 45 bits at the most: no stream a device can hold has the event, and the images must not.
    assert max(F.width(l) for l in (F.RUN_MAX - 1, 1 << 31)) == 45
    assert tally.pop("exact") == 0
    assert all(v > 0 for v in tally.values()), tally
    assert (trans > 0).all(), trans
    assert all(v > 0 for v in totals.values()), totals
    # segments: where the runs s * seg of the streams without huge runs lie
    for seg in F.SEGS:
        ent = [e for n in F.SEG_NAMES for e in F.entries(ev[n], seg)]
        offs, types = {o for o, _, _ in ent}, {t for _, t, _ in ent}
        print("seg %d: %d entries, %d offsets (max %d), block types %s" % (seg, len(ent), len(offs), max(offs), sorted(types)))
        assert 0 in offs and max(offs) >= 94 and len(offs) >= 64 and {0, 1} <= types
    ent = [e for n in F.TYPES_NAMES for e in ev[n]["seg_entry"]]
    print("types streams, seg 96: %d entries, %d in a type-2 block, %d right behind one" % (len(ent), sum(t == 2 for _, t, _ in ent), sum(p == 2 for _, _, p in ent)))
    assert any(t == 2 for _, t, _ in ent) and any(p == 2 for _, _, p in ent)
    ent = [e for n in F.NAMES for e in ev[n]["batch_entry"]]
    print("batch %d: %d entries, %d in a type-1 block" % (F.BATCH, len(ent), sum(t == 1 and o > 0 for o, t, _ in ent)))
    assert any(t == 1 and o > 0 for o, t, _ in ent), "no batch boundary inside a block with a type-1 header"


def test_a_wrong_image_is_named_by_byte_block_and_segment(tmp_path):
    """what tests/test_fmd_streams_gpu.py says when an image differs, on images spoilt by hand: the header of block 2 of ones_191 (the
    first block that starts in the second segment of 96 runs) with one count off by one, a payload bit, a rank frame, a short image"""
    from test_fmd_streams_gpu import same_image
    want = F.image("ones_191", tmp_path)
    same_image(want.copy(), want, "equal", 96)
    for byte, words in ((80 + 2 * 64 + 2, ("byte %d" % (80 + 2 * 64 + 2), "block 2 ", "word 0 (header)", "runs are 190 .. 190", "segment 1 of 96")),
                        (80 + 64 + 3 * 8 + 5, ("block 1 ", "word 3 (payload)", "runs are 95 .. 189", "segment 0 of 96")),
                        (len(want) - 56 + 9, ("word 1 of rank frame %d" % (F.fmd_ref.parse(want)["n_frames"] - 1),))):
        got = want.copy()
        got[byte] ^= 1
        with pytest.raises(AssertionError) as e:
            same_image(got, want, "ones_191, spoilt", 96)
        assert all(w in str(e.value) for w in ("ones_191", "byte %d" % byte) + words), str(e.value)
    with pytest.raises(AssertionError) as e:
        same_image(want[:-56], want, "ones_191, short", 96)
    assert "byte %d" % (len(want) - 56) in str(e.value) and "rank frame" in str(e.value)
