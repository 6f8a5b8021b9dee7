"""GPU tests of the .fmd encoder (include/rb2_hip.h: rb2_hip_save_fmd[_file]; kernels k_fmds_* in csrc/rb2_fmd_save.h): the image of a
device index must be, byte for byte, the file the reference wrote (tests/golden/fmd) or the one the host writer makes of the same ropes
(tests/fmd_save_ref.py) -- for loaded and built indexes, in both layouts, after a deletion, with the encoder's batches and segments at
their defaults and at the smallest sizes it accepts, across the end of a chunk of 2^23 words -- and the index must be what it was."""
import os

import numpy as np
import pytest

import fmd_ref
import helpers as H
from fmd_save_ref import fmd_of, write_fmd
from fmd_streams import run8
from ropebwt2_amd.hipbwt import encode_runs

pytestmark = pytest.mark.gpu
FORCED = dict(RB2_SPARSE_LAMBDA="1e18", RB2_SPARSE_MAXPEN="0")       # every batch in place: the sparse layout (test_fmd_load_gpu.py, test_inplace_paths_gpu.py)
SMALL = dict(RB2_FMDS_SEG="96", RB2_FMDS_BATCH="2048")               # the smallest segments and batches: a leaf per batch, a table per 96 runs


class _Env:
    def __init__(self, **kw):
        self.kw = kw
    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update({k: str(v) for k, v in self.kw.items()})
    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def same(a, b, what=""):
    a, b = np.frombuffer(bytes(a), np.uint8) if not isinstance(a, np.ndarray) else a, np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else b
    if len(a) != len(b) or not np.array_equal(a, b):
        n = min(len(a), len(b))
        d = np.flatnonzero(a[:n] != b[:n])
        raise AssertionError("%s: images of %d and %d bytes, first difference at byte %s" % (what, len(a), len(b), d[0] if len(d) else n))


def save_both(g, what):
    """save_fmd() with the default batches and segments and with the smallest ones: the same image"""
    a = g.save_fmd()
    with _Env(**SMALL):
        b = g.save_fmd()
    same(a, b, what + ": small segments against the default")
    return a


# ---- files the reference wrote ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixtures():
    return {n: fmd_ref.fixture(n) for n in fmd_ref.FIXTURES}


@pytest.mark.parametrize("name", fmd_ref.FIXTURES)
def test_reference_files(hip, fixtures, tmp_path, name):
    img, bwt = fixtures[name]
    mcnt = fmd_ref.parse(img)["mcnt"]
    cut = np.concatenate([[0], np.cumsum(mcnt)])
    g = hip.HipBwt(0)
    g.load_ropes([encode_runs(bwt[cut[b]:cut[b + 1]]) for b in range(6)])
    same(save_both(g, name), img, name + " from its BWT")
    assert g.load_fmd(img) == len(bwt)
    same(save_both(g, name), img, name + " loaded and saved")
    if name == "kat6":                                               # once through rb2_hip_save_fmd_file
        p = tmp_path / "kat6.fmd"
        assert g.save_fmd(str(p)) == len(img)
        same(np.fromfile(str(p), np.uint8), img, "kat6 by path")
    g.close()


# ---- built indexes ------------------------------------------------------------------------------------------------------------------

def _two_batches(seed):
    return [H.encode_batch(H.repetitive_reads(k, seed=seed + i, max_len=40), True, True) for i, k in enumerate((300, 200))]


@pytest.mark.parametrize("variant", ["dense", "sparse", "deleted"])
@pytest.mark.parametrize("so", [0, 1, 2])
def test_built_index(hip, tmp_path, so, variant):
    extra = H.encode_batch(H.repetitive_reads(150, seed=70 + so, max_len=40), True, True)
    with _Env(**(FORCED if variant == "sparse" else {})):
        g, twin = hip.HipBwt(so), hip.HipBwt(so)
        for b in _two_batches(50 + so):
            g.insert_multi(b); twin.insert_multi(b)
        if variant == "sparse":
            assert g.layout_stats()["sparse_now"]
        if variant == "deleted":
            ids = np.arange(0, int(g.counts()[0].sum()), 3)
            g.delete(ids); twin.delete(ids)
        hashes, counts = g.rope_hashes(), g.counts().copy()
        want = fmd_of(twin, tmp_path / "want.fmd")
        same(save_both(g, "%s so=%d" % (variant, so)), want, "%s so=%d" % (variant, so))
        assert g.rope_hashes() == hashes and np.array_equal(g.counts(), counts)
        g.insert_multi(extra); twin.insert_multi(extra)              # the index is what it was: it grows like a twin that never saved
        assert g.rope_hashes() == twin.rope_hashes() and np.array_equal(g.counts(), twin.counts())
        same(g.save_fmd(), fmd_of(twin, tmp_path / "want2.fmd"), "after one more batch")
    g.close(); twin.close()


# ---- merging across ropes, empty ropes, long runs -------------------------------------------------------------------------------------

def test_type2_header_and_a_run_over_2_20_leaves(hip, tmp_path):
    n = 1 << 30
    # one string of 2^30 A's: rope $ = A; rope A = 2^30 - 1 A's, then $ -- the A of rope $ and the A's of rope A are one run
    rles = [encode_runs([1]), np.concatenate([run8(n - 1, 1), encode_runs([0])])] + [np.zeros(0, np.uint8)] * 4
    g = hip.HipBwt(0)
    g.load_ropes(rles)
    want = write_fmd(tmp_path / "t2.fmd", pushes=[(1, 1), (n - 1, 1), (1, 0)])
    words = fmd_ref.parse(want.tobytes())["words"]
    assert len(words) == 8 + 7 and int(words[8]) >> 62 == 2
    same(g.save_fmd(), want, "2^30 A's")
    with _Env(RB2_FMDS_SEG="96"):                                    # the type-2 header opens a segment of its own kind, at the default batch
        same(g.save_fmd(), want, "2^30 A's, segments of 96 runs")
    g.close()


def test_runs_across_rope_boundaries_and_empty_ropes(hip, tmp_path):
    """strings over A and T only: ropes C, G and N are empty, and in the set chosen rope $ ends in the symbol rope A starts with and rope A
    ends in the symbol rope T starts with (the first seed for which the BWT does that)"""
    found = None
    for seed in range(200):
        rng = np.random.RandomState(seed)
        reads = [np.where(rng.randint(0, 2, size=int(rng.randint(5, 30))) == 1, 4, 1).astype(np.uint8) for _ in range(40)]
        g = hip.HipBwt(0)
        g.insert_multi(H.encode_batch(reads, True, False))
        r = g.ropes()
        if len(r[2]) == 0 and len(r[3]) == 0 and len(r[5]) == 0 and r[0][-1] == r[1][0] and r[1][-1] == r[4][0]:
            found = g
            break
        g.close()
    assert found is not None, "no seed gives the boundaries the test wants"
    g = found
    rles = [g.rope_rle(b) for b in range(6)]
    want = write_fmd(tmp_path / "at.fmd", rles)
    runs = fmd_ref.decode(want.tobytes())["runs"]
    assert sum(l for _, l in runs) == int(g.counts().sum())
    same(save_both(g, "built"), want, "A/T strings, built")
    l = hip.HipBwt(0)
    l.load_ropes(rles)
    same(save_both(l, "loaded"), want, "A/T strings, via load_ropes")
    g.close(); l.close()


def test_type1_headers(hip, tmp_path):
    """runs of 16384 symbols and more between short ones: blocks whose totals need 32-bit fields"""
    rng = np.random.RandomState(9)
    reads = [np.full(20000, 1, np.uint8), np.full(17000, 2, np.uint8), np.full(40000, 4, np.uint8)]
    reads += [rng.randint(1, 5, size=int(rng.randint(20, 60))).astype(np.uint8) for _ in range(60)]
    reads += [np.concatenate([np.full(16384 + k, 3, np.uint8), rng.randint(1, 5, size=10).astype(np.uint8)]) for k in range(3)]
    g = hip.HipBwt(0)
    g.insert_multi(H.encode_batch(reads, True, False))
    rles = [g.rope_rle(b) for b in range(6)]
    want = write_fmd(tmp_path / "t1.fmd", rles)
    types = {t for t, _, _ in fmd_ref.decode(want.tobytes())["blocks"]}
    assert 1 in types and 0 in types
    l = hip.HipBwt(0)
    l.load_ropes(rles)
    same(save_both(l, "type 1"), want, "type-1 headers")
    g.close(); l.close()


# ---- the chunk rule -------------------------------------------------------------------------------------------------------------------

CHUNK_READS = 1100000        # x 101 bp, i.i.d.: 61.4 bytes of stream per read (tests/test_fmd_load_gpu.py::test_chunk_boundary) -> 2^26 bytes at 1.093 M reads


def test_chunk_boundary(hip, tmp_path):
    g = hip.HipBwt(0)
    nbytes = CHUNK_READS * 102
    buf = g.dev_alloc(nbytes)
    g.synth_reads(buf, 0, CHUNK_READS, 101, seed=5)
    g.insert_multi_dev(buf, nbytes)
    g.sync()
    g.dev_free(buf)
    img = g.save_fmd()
    stream = int(np.frombuffer(img[16:24].tobytes(), "<u8")[0])       # n_bytes of the header
    print("stream of %d bytes (2^26 = %d)" % (stream, 1 << 26))
    assert stream > 1 << 26, "the stream must cross a chunk of 2^23 words"
    want = fmd_of(g, tmp_path / "big.fmd")
    assert len(img) == len(want) and H.md5(img.tobytes()) == H.md5(want.tobytes())
    g.close()


# ---- the sizing call, the empty index, a file that cannot be written ---------------------------------------------------------------------

def test_sizing_call(hip, tmp_path):
    g = hip.HipBwt(0)
    for b in _two_batches(5):
        g.insert_multi(b)
    want = fmd_of(g, tmp_path / "w.fmd")
    size = int(g.L.rb2_hip_save_fmd(g.h, None, 0))
    assert size == len(want)
    buf = np.full(size + 64, 0xA5, np.uint8)
    assert int(g.L.rb2_hip_save_fmd(g.h, buf.ctypes.data, size - 1)) == size
    assert (buf == 0xA5).all(), "a buffer that is too small must not be touched"
    assert int(g.L.rb2_hip_save_fmd(g.h, buf.ctypes.data, size)) == size
    same(buf[:size], want, "cap == SIZE")
    assert (buf[size:] == 0xA5).all()
    g.close()


def test_empty_index(hip, tmp_path):
    want = write_fmd(tmp_path / "empty.fmd")
    g = hip.HipBwt(0)
    same(g.save_fmd(), want, "empty index")
    assert g.save_fmd(str(tmp_path / "e2.fmd")) == len(want)
    same(np.fromfile(str(tmp_path / "e2.fmd"), np.uint8), want, "empty index by path")
    g.close()


def test_unwritable_path(hip, tmp_path):
    g = hip.HipBwt(0)
    for b in _two_batches(7):
        g.insert_multi(b)
    counts = g.counts().copy()
    bad = str(tmp_path / "no_such_directory" / "x.fmd")
    assert int(g.L.rb2_hip_save_fmd_file(g.h, os.fsencode(bad))) == -1
    with pytest.raises(OSError):
        g.save_fmd(bad)
    assert np.array_equal(g.counts(), counts)
    g.close()
