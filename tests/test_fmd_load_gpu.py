"""GPU tests of the .fmd loader (include/rb2_hip.h: rb2_hip_load_fmd[_file], rb2_hip_multi_load_fmd; kernels k_fmd_* in
csrc/rb2_fmd_load.h): files the reference wrote (tests/golden/fmd), files this project's writer makes from a device index, and
malformed images.  An index that was loaded must be the index that was written: checksums per rope, the count matrix, query results,
and what further inserts make of it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fmd_ref
import helpers as H
import query_ref as Q
from ropebwt2_amd.hipbwt import encode_runs
from test_query_gpu import _Env, _batches, _patterns
from test_smem_gpu import _queries

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FORCED = dict(RB2_SPARSE_LAMBDA="1e18", RB2_SPARSE_MAXPEN="0")       # every batch in place: the sparse layout (test_inplace_paths_gpu.py)


# ---- the host writer (libropebwt2.so: rb2_fmd_*, include/rb2_fmd.h), as tools/fuzz_host_writers.py drives it ----------------------

_host = None


def host_lib():
    global _host
    if _host is None:
        from ropebwt2_amd.build import lib_path
        L = C.CDLL(lib_path("libropebwt2.so"))
        L.rb2_fmd_init.restype = C.c_void_p
        L.rb2_fmd_push.argtypes = [C.c_void_p, C.c_int64, C.c_int]
        L.rb2_fmd_push_runs.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.rb2_fmd_finish.argtypes = [C.c_void_p]
        L.rb2_fmd_write_path.argtypes = [C.c_void_p, C.c_char_p]
        L.rb2_fmd_destroy.argtypes = [C.c_void_p]
        _host = L
    return _host


def write_fmd(path, rles=(), pushes=()):
    """an .fmd from six 43+3 run streams in rope order (and / or single runs (len, sym)); returns the file image"""
    L = host_lib()
    f = L.rb2_fmd_init()
    for r in rles:
        b = np.ascontiguousarray(r, dtype=np.uint8).tobytes()
        L.rb2_fmd_push_runs(f, b, len(b))
    for l, c in pushes:
        L.rb2_fmd_push(f, l, c)
    L.rb2_fmd_finish(f)
    assert L.rb2_fmd_write_path(f, str(path).encode()) == 0
    L.rb2_fmd_destroy(f)
    return np.fromfile(str(path), dtype=np.uint8)


def fmd_of(g, path):
    return write_fmd(path, [g.rope_rle(b) for b in range(6)])


def assert_same_index(a, b, what=""):
    assert a.rope_hashes() == b.rope_hashes(), what
    assert np.array_equal(a.counts(), b.counts()), what


# ---- files the reference wrote ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixtures():
    return {n: fmd_ref.fixture(n) for n in fmd_ref.FIXTURES}


@pytest.mark.parametrize("name", fmd_ref.FIXTURES)
def test_reference_files(hip, fixtures, name):
    img, bwt = fixtures[name]
    mcnt = fmd_ref.parse(img)["mcnt"]
    g = hip.HipBwt(0)
    if name == "kat6":                                               # once through rb2_hip_load_fmd_file, by path
        assert g.load_fmd(os.path.join(fmd_ref.GOLDEN_FMD, name + ".fmd")) == len(bwt)
    else:
        assert g.load_fmd(img) == len(bwt)
    assert np.array_equal(g.bwt(), bwt)
    assert g.counts().sum(1).tolist() == mcnt
    cut = np.concatenate([[0], np.cumsum(mcnt)])
    r = hip.HipBwt(0)
    r.load_ropes([encode_runs(bwt[cut[b]:cut[b + 1]]) for b in range(6)])
    assert_same_index(g, r, name)
    g.load_fmd(np.frombuffer(img, np.uint8))                         # again, over the index that is there
    assert_same_index(g, r, name + " (reloaded)")
    g.close(); r.close()


# ---- round trip through this project's writer -------------------------------------------------------------------------------------

@pytest.mark.parametrize("so", [0, 1, 2])
def test_round_trip(hip, tmp_path, so):
    batches, strings = _batches(40 + so, True)
    extra = H.encode_batch(H.repetitive_reads(150, seed=90 + so, max_len=40), True, True)
    g = hip.HipBwt(so)
    for b in batches:
        g.insert_multi(b)
    img = fmd_of(g, tmp_path / "rt.fmd")
    l = hip.HipBwt(so)
    assert l.load_fmd(img) == int(g.counts().sum())
    assert_same_index(g, l)
    pats = _patterns(strings, np.random.RandomState(so))
    for x, y in zip(g.backward_search(pats), l.backward_search(pats)):
        assert np.array_equal(x, y)
    qs = _queries(strings, np.random.RandomState(10 + so), k=200)
    for kw in (dict(min_len=1, min_occ=1), dict(min_len=5, min_occ=2)):
        (sa, ma, ca), (sb, mb, cb) = g.smem_raw(qs, **kw), l.smem_raw(qs, **kw)
        assert sa == sb and np.array_equal(ca, cb) and np.array_equal(ma, mb)
    g.insert_multi(extra); l.insert_multi(extra)                     # a loaded index is a full citizen
    assert_same_index(g, l, "after one more batch")
    g.close(); l.close()


@pytest.mark.parametrize("flags,so,rev", [("-LRs", 1, False), ("-Lr", 2, True)])
def test_file_made_by_the_reference_binary(hip, flags, so, rev):
    if not H.have_ref():
        pytest.skip("oracle/_ref/ropebwt2 is not built")
    reads = H.repetitive_reads(600, seed=33, max_len=40)
    img = H.run_ref([flags + "d"], H.lines_from_codes(reads))
    g = hip.HipBwt(so)
    g.insert_multi(H.encode_batch(reads, True, rev))                 # one batch, as the reference inserts them
    l = hip.HipBwt(so)
    assert l.load_fmd(img) == int(g.counts().sum())
    assert_same_index(g, l)
    pats = _patterns(Q.inserted_strings(reads, True, rev), np.random.RandomState(5))
    for x, y in zip(g.backward_search(pats), l.backward_search(pats)):
        assert np.array_equal(x, y)
    g.close(); l.close()


# ---- over an index in the sparse layout; sharded ----------------------------------------------------------------------------------

def test_load_over_a_sparse_index(hip, fixtures):
    rng = np.random.RandomState(3)
    reads = [rng.randint(1, 5, size=int(rng.randint(1500, 2600))).astype(np.uint8) for _ in range(80)]
    img, bwt = fixtures["cov3000"]
    with _Env(**FORCED):
        g = hip.HipBwt(1)
        for part in (reads[:40], reads[40:]):
            g.insert_multi(H.encode_batch(part, True, True))
        assert g.layout_stats()["sparse_now"]
        assert g.load_fmd(img) == len(bwt)
        assert not g.layout_stats()["sparse_now"]
        assert np.array_equal(g.bwt(), bwt)
        d = hip.HipBwt(1)
        d.load_fmd(img)
        assert_same_index(g, d)
        extra = H.encode_batch(H.repetitive_reads(100, seed=8, max_len=40), True, False)
        g.insert_multi(extra); d.insert_multi(extra)
        assert_same_index(g, d, "after one more batch")
    g.close(); d.close()


@pytest.mark.parametrize("n", [2, 3])
def test_sharded(hip, fixtures, n):
    m = hip.MultiBwt(0, [0] * n, "peer")
    g = hip.HipBwt(0)
    for name in ("cov3000", "longA", "rand300"):
        img, bwt = fixtures[name]
        assert m.load_fmd(img) == len(bwt) and g.load_fmd(img) == len(bwt)
        assert m.rope_hashes() == g.rope_hashes(), name
        assert np.array_equal(m.counts(), g.counts()), name
    m.close(); g.close()


# ---- header of type 2, the chunk rule, the empty file -----------------------------------------------------------------------------

def _run8(l, c):
    """one 8-byte run of the 43+3 codec (rle.h:53-75), as hipbwt.encode_runs writes runs of 2^19 symbols and more"""
    tail = [0x80 | (l >> (6 * k)) & 0x3f for k in range(7)]
    return np.array([0xF0 | (l >> 42) << 3 | c] + tail[::-1], np.uint8)


def test_type2_header(hip, tmp_path):
    n = 1 << 30
    small = (1 << 19) + 5
    assert np.array_equal(_run8(small, 1), encode_runs(np.full(small, 1, np.uint8)))
    # one string of 2^30 A's: rope $ = A; rope A = 2^30 - 1 A's, then $
    rles = [encode_runs([1]), np.concatenate([_run8(n - 1, 1), encode_runs([0])])] + [np.zeros(0, np.uint8)] * 4
    r = hip.HipBwt(0)
    r.load_ropes(rles)
    img = write_fmd(tmp_path / "t2.fmd", pushes=[(1, 1), (n - 1, 1), (1, 0)])
    words = fmd_ref.parse(img.tobytes())["words"]
    # both runs fit the first block, so the stream is that block and the closing header, which describes 2^30 + 1 symbols
    assert len(words) == 8 + 7 and int(words[8]) >> 62 == 2 and fmd_ref.header(words, 8)[1] == [n + 1, 1, n, 0, 0, 0, 0]
    g = hip.HipBwt(0)
    assert g.load_fmd(img) == n + 1
    assert_same_index(g, r)
    assert g.counts().tolist() == [[0, 1, 0, 0, 0, 0], [1, n - 1, 0, 0, 0, 0]] + [[0] * 6] * 4
    g.close(); r.close()


CHUNK_READS = 1100000        # x 101 bp, i.i.d.: 61.4 bytes of stream per read (measured: 1.15 M reads gave 70 633 040 bytes) -> 2^26 bytes at 1.093 M reads


def test_chunk_boundary(hip, tmp_path):
    g = hip.HipBwt(0)
    nbytes = CHUNK_READS * 102
    buf = g.dev_alloc(nbytes)
    g.synth_reads(buf, 0, CHUNK_READS, 101, seed=5)
    g.insert_multi_dev(buf, nbytes)
    g.sync()
    g.dev_free(buf)
    img = fmd_of(g, tmp_path / "big.fmd")
    stream = int(np.frombuffer(img[16:24].tobytes(), "<u8")[0])       # n_bytes of the header
    print("stream of %d bytes (2^26 = %d)" % (stream, 1 << 26))
    assert stream > 1 << 26, "the stream must cross a chunk of 2^23 words"
    l = hip.HipBwt(0)
    assert l.load_fmd(img) == nbytes
    assert_same_index(g, l)
    g.close(); l.close()


def test_empty_file(hip, tmp_path):
    img = write_fmd(tmp_path / "empty.fmd")
    assert fmd_ref.parse(img.tobytes())["mcnt"] == [0] * 6
    g = hip.HipBwt(0)
    g.insert_multi(H.encode_batch(H.repetitive_reads(50, seed=1), True, False))
    assert g.load_fmd(img) == 0
    assert g.counts().sum() == 0 and len(g.bwt()) == 0
    f = hip.HipBwt(0)
    b = H.encode_batch(H.repetitive_reads(80, seed=2), True, True)
    g.insert_multi(b); f.insert_multi(b)
    assert_same_index(g, f)
    g.close(); f.close()


# ---- malformed images: a message through the fatal handler, never a fault ---------------------------------------------------------

@pytest.mark.parametrize("case,message", [
    ("magic", "load_fmd: wrong magic"),
    ("sbits", "load_fmd: alphabet size 6 and block bits 4"),
    ("truncated", "load_fmd: the image is truncated"),
    ("bitflip", "load_fmd: a block's decoded symbols disagree with the counts in the next header"),
])
def test_malformed(hip, case, message):
    p = subprocess.run([sys.executable, os.path.join(HERE, "fmd_malformed_child.py"), case, "rand300"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 7, (p.returncode, p.stdout.decode()[-300:], p.stderr.decode()[-300:])
    assert ("handler: [rb2_hip] " + message) in p.stdout.decode(), p.stdout.decode()[-300:]
